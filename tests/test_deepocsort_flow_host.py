"""DeepOcSort in run_sequences, host side, no GPU: the batched engine is built with the drop-in's
parameters and never through create_tracker, per_class raises as the drop-in does, and
resident=True names itself where a tracker has no feeder."""
import inspect

import numpy as np
import pytest

import boxmot_amd._native as N
from boxmot_amd import motio


class Probe:
    """Stands in for DeepOcsortEngine: records what the runner builds it with."""

    seen = {}

    def __init__(self, **kw):
        Probe.seen = kw
        raise N.NativeUnavailable("no device")


@pytest.fixture
def probed(monkeypatch):
    from boxmot_amd import engine, tracker_zoo
    from boxmot_amd.trackers import deepocsort as mod

    Probe.seen = {}
    monkeypatch.setattr(engine, "DeepOcsortEngine", Probe)
    monkeypatch.setattr(mod, "DeepOcsortEngine", Probe)
    monkeypatch.setattr(tracker_zoo, "create_tracker",
                        lambda *a, **k: pytest.fail("create_tracker reached"))
    return Probe


def test_batched_engine_takes_the_dropins_parameters(probed):
    kw = dict(det_thresh=0.4, max_age=20, min_hits=2, iou_threshold=0.25, delta_t=2,
              asso_func="giou", inertia=0.3, w_association_emb=0.6, alpha_fixed_emb=0.9,
              aw_param=0.4, aw_off=True, Q_xy_scaling=0.02, Q_s_scaling=0.0002, track_cap=32,
              det_cap=16, reid_weights=None, device="cuda", half=False)
    with pytest.raises(N.NativeUnavailable):
        motio._batched_engine("deepocsort", 7, 48, kw)
    p = probed.seen["params"]
    assert (p.det_thresh, p.max_age, p.min_hits, p.iou_threshold, p.delta_t, p.asso_func) == \
        (0.4, 20, 2, 0.25, 2, "giou")
    assert (p.inertia, p.w_association_emb, p.alpha_fixed_emb, p.aw_param) == (0.3, 0.6, 0.9, 0.4)
    assert (p.embedding_off, p.aw_off, p.Q_xy_scaling, p.Q_s_scaling) == (False, True, 0.02, 0.0002)
    assert {k: probed.seen[k] for k in ("n_seq", "track_cap", "det_cap", "emb_dim")} == \
        {"n_seq": 7, "track_cap": 32, "det_cap": 16, "emb_dim": 48}


def test_empty_kwargs_are_the_constructor_defaults(probed):
    from boxmot_amd import DeepOcSort
    from boxmot_amd.engine import DeepOcsortParams

    with pytest.raises(N.NativeUnavailable):
        motio._batched_engine("deepocsort", 3, 20, {})
    assert probed.seen["params"] == DeepOcsortParams() == DeepOcSort()._params
    sig = inspect.signature(DeepOcSort.__init__).parameters
    assert (probed.seen["track_cap"], probed.seen["det_cap"]) == \
        (sig["track_cap"].default, sig["det_cap"].default)
    assert (probed.seen["n_seq"], probed.seen["emb_dim"]) == (3, 20)


def test_no_deepocsort_yaml():
    from boxmot_amd import _native

    assert not (_native.PKG / "configs" / "trackers" / "deepocsort.yaml").exists()


def test_per_class_raises(probed, tmp_path):
    with pytest.raises(NotImplementedError, match="per_class"):
        motio._batched_engine("deepocsort", 2, 20, {"per_class": True})
    with pytest.raises(NotImplementedError, match="per_class"):
        motio.run_sequences("deepocsort", {}, tmp_path, tracker_kwargs={"per_class": True})
    assert probed.seen == {}


@pytest.mark.parametrize("kind", ["bytetrack", "botsort", "ocsort", "boosttrack", "strongsort"])
def test_resident_names_itself_where_there_is_no_feeder(monkeypatch, tmp_path, kind):
    monkeypatch.setattr(motio, "_batched_engine",
                        lambda *a, **k: pytest.fail("an engine was built"))
    with pytest.raises(NotImplementedError, match="resident"):
        motio.run_sequences(kind, {}, tmp_path, resident=True)
    assert not list(tmp_path.iterdir())


def test_resident_is_a_public_switch_off_by_default():
    p = inspect.signature(motio.run_sequences).parameters["resident"]
    assert p.default is False and "deepocsort" in motio.RESIDENT_TRACKERS


def test_pack_arrays_keeps_the_values(tmp_path):
    """pack_arrays is pack_sequence without the text files: the float64 values as given."""
    rng = np.random.default_rng(3)
    fid = np.repeat([4, 1, 9], [3, 2, 4])
    dets = np.column_stack([fid, rng.uniform(0, 1000, (9, 4)), rng.uniform(0, 1, 9),
                            rng.integers(0, 3, 9)])
    embs = rng.standard_normal((9, 5))
    b = motio.BinSequence(motio.pack_arrays(dets, embs, tmp_path / "s.bxmot"))
    assert list(b.frame_ids) == [1, 4, 9] and b.emb_dim == 5
    for f in (1, 4, 9):
        d, e = b.frame(f)
        np.testing.assert_array_equal(d, dets[fid == f, 1:])
        np.testing.assert_array_equal(e, embs[fid == f])
    z = motio.BinSequence(motio.pack_arrays(np.empty((0, 7)), np.empty((0, 5)), tmp_path / "z"))
    assert z.rows == 0 and z.n_frames == 0 and z.emb_dim == 5

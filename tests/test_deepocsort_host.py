"""DeepOcSort's host side, no GPU: the import, the reference's constructor defaults, parameter
pass-through to the engine, loud failure without a device, input checks and the fixtures' form."""
import inspect
from pathlib import Path

import numpy as np
import pytest

import boxmot_amd._native as N

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = ["grid24_f20", "crowd40_f64", "crowd40_awoff", "crowd40_emboff", "crowd32_warp",
         "crowd96_f32", "giou_crowd40", "dt1_short", "dt7_warp", "params", "hmiou", "ciou", "diou",
         "centroid", "stop76"]
IMG = np.zeros((1080, 1920, 3), np.uint8)

# the reference signature's values (trackers/deepocsort/deepocsort.py:265-287)
REFERENCE_DEFAULTS = {
    "per_class": False, "det_thresh": 0.3, "max_age": 30, "min_hits": 3, "iou_threshold": 0.3,
    "delta_t": 3, "asso_func": "iou", "inertia": 0.2, "w_association_emb": 0.5,
    "alpha_fixed_emb": 0.95, "aw_param": 0.5, "embedding_off": False, "cmc_off": False,
    "aw_off": False, "Q_xy_scaling": 0.01, "Q_s_scaling": 0.0001,
}


class Probe:
    """Stands in for DeepOcsortEngine: records what the drop-in builds it with."""

    seen = {}

    def __init__(self, **kw):
        Probe.seen = kw
        raise N.NativeUnavailable("no device")


def test_import_and_reference_defaults():
    from boxmot_amd import DeepOcSort
    from boxmot_amd.trackers import DeepOcSort as same

    assert DeepOcSort is same
    params = inspect.signature(DeepOcSort.__init__).parameters
    assert list(params)[1:4] == ["reid_weights", "device", "half"]
    assert {k: params[k].default for k in REFERENCE_DEFAULTS} == REFERENCE_DEFAULTS
    assert "track_cap" in params and "det_cap" in params


def test_construction_passes_parameters_to_the_engine(monkeypatch):
    from boxmot_amd.trackers import deepocsort as mod

    monkeypatch.setattr(mod, "DeepOcsortEngine", Probe)
    with pytest.raises(N.NativeUnavailable):  # embedding_off: the engine is built at once
        mod.DeepOcSort(det_thresh=0.4, max_age=20, min_hits=2, iou_threshold=0.25, delta_t=2,
                       asso_func="giou", inertia=0.3, w_association_emb=0.6, alpha_fixed_emb=0.9,
                       aw_param=0.4, embedding_off=True, aw_off=True, Q_xy_scaling=0.02,
                       Q_s_scaling=0.0002, track_cap=32, det_cap=16)
    p = Probe.seen["params"]
    assert (p.det_thresh, p.max_age, p.min_hits, p.iou_threshold, p.delta_t, p.asso_func) == \
        (0.4, 20, 2, 0.25, 2, "giou")
    assert (p.inertia, p.w_association_emb, p.alpha_fixed_emb, p.aw_param) == (0.3, 0.6, 0.9, 0.4)
    assert (p.embedding_off, p.aw_off, p.Q_xy_scaling, p.Q_s_scaling) == (True, True, 0.02, 0.0002)
    assert (Probe.seen["track_cap"], Probe.seen["det_cap"], Probe.seen["n_seq"]) == (32, 16, 1)
    # with the embedding term on, the engine is built once the first embeddings give the width
    tr = mod.DeepOcSort()
    assert tr.engine is None and tr.active_tracks == []
    dets = np.array([[10, 10, 50, 90, 0.9, 0]], np.float64)
    with pytest.raises(N.NativeUnavailable):
        tr.update(dets, IMG, np.ones((1, 20), np.float32))
    assert Probe.seen["emb_dim"] == 20 and Probe.seen["params"].det_thresh == 0.3


def test_engine_without_gpu_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    N.build()
    from boxmot_amd.engine import DeepOcsortEngine

    with pytest.raises(N.NativeUnavailable):
        DeepOcsortEngine()


def test_per_class_is_not_implemented():
    from boxmot_amd import DeepOcSort

    with pytest.raises(NotImplementedError, match="per_class"):
        DeepOcSort(per_class=True)


def test_update_without_embs_raises(monkeypatch):
    from boxmot_amd.trackers import deepocsort as mod

    monkeypatch.setattr(mod, "DeepOcsortEngine", Probe)
    tr = mod.DeepOcSort()
    with pytest.raises(ValueError, match="needs `embs`"):
        tr.update(np.array([[10, 10, 50, 90, 0.9, 0]], np.float64), IMG)


def test_leading_empty_frames_wait_for_the_embedding_width(monkeypatch):
    """An empty first frame builds no engine (there is no width to build it with); the engine is
    built with the width of the first embeddings that arrive."""
    from boxmot_amd.trackers import deepocsort as mod

    monkeypatch.setattr(mod, "DeepOcsortEngine", Probe)
    Probe.seen = {}
    tr = mod.DeepOcSort()
    for _ in range(2):
        assert np.asarray(tr.update(np.empty((0, 6)), IMG)).size == 0
    assert tr.engine is None and Probe.seen == {} and tr.frame_count == 2
    with pytest.raises(N.NativeUnavailable):
        tr.update(np.array([[10, 10, 50, 90, 0.9, 0]], np.float64), IMG, np.ones((1, 128)))
    assert Probe.seen["emb_dim"] == 128


@pytest.mark.parametrize("name", CASES)
def test_fixture_form(name):
    path = GOLDEN / f"deepoc_{name}.npz"
    assert path.stat().st_size < 1 << 20  # the repository's limit for a committed file
    keys = {"outputs", "n_frames", "kind", "scene", "tracker_args", "lap_calls", "lap_degenerate",
            "lap_frames", "fast_frames", "ocr_rematches", "oru_unfreezes", "affine_frozen",
            "frames_gt64", "deaths", "births", "below_thresh_dets", "lookback_ge4", "ocr_big",
            "first_big", "needs", "state_frames", "state_off", "state_id", "state_x", "state_P"}
    with np.load(path) as fx:
        assert set(fx.files) - {"warp_seed", "scene_kind", "state_emb"} == keys
        assert ("warp_seed" in fx.files) == (name in ("crowd32_warp", "dt7_warp"))
        assert ("scene_kind" in fx.files) == (name == "stop76")
        assert ("state_emb" in fx.files) == (name != "crowd40_emboff")
        assert str(fx["kind"]) == "deepocsort" and int(fx["n_frames"]) <= 120
        assert fx["outputs"].shape[1] == 9
        assert "float64" in str(fx["scene"]) or name == "stop76"  # (StopScene: always float64)


def test_only_these_fixtures():
    assert sorted(p.stem for p in GOLDEN.glob("deepoc_*.npz")) == sorted(
        f"deepoc_{n}" for n in CASES)

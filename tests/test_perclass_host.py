"""CPU-side checks of the per_class mode of DeepOcSort / HybridSort: the classes that carry it,
the trackers the resident feeder drives, the engines run_sequences builds, and the per_class
fixtures' own coverage counters."""
import ast
from pathlib import Path

import numpy as np
import pytest

from boxmot_amd import motio

GOLDEN = Path(__file__).resolve().parent / "golden"
IMG = np.zeros((1080, 1920, 3), np.uint8)


def test_resident_trackers():
    assert motio.RESIDENT_TRACKERS == ("deepocsort", "hybridsort")


def test_public_names():
    import boxmot_amd
    from boxmot_amd import DeepOcSort, DeepOcSortPerClass, HybridSort, HybridSortPerClass

    assert issubclass(DeepOcSortPerClass, DeepOcSort) and issubclass(HybridSortPerClass, HybridSort)
    for n in ("DeepOcSortPerClass", "HybridSortPerClass"):
        assert n in boxmot_amd.__all__ and n in boxmot_amd.trackers.__all__


def test_per_class_subclasses_build_without_a_gpu():
    """No engine is built before the first detections (the embedding width is unknown);
    reid_weights / device / half are accepted and ignored."""
    from boxmot_amd import DeepOcSortPerClass, HybridSortPerClass

    d = DeepOcSortPerClass(reid_weights="w.pt", device="cpu", half=True, max_age=7)
    assert d.per_class and d.nr_classes == 80 and d.engine is None and d.max_age == 7
    assert DeepOcSortPerClass(nr_classes=3, per_class=False).per_class  # (the mode is the class)
    h = HybridSortPerClass("w.pt", "cpu", True, 0.4, nr_classes=5, min_hits=2)
    assert h.per_class and h.nr_classes == 5 and h.engine is None and h._params.min_hits == 2
    with pytest.raises(NotImplementedError, match="use_byte"):
        HybridSortPerClass(None, None, False, 0.4, use_byte=True)
    # an empty frame on an empty per-class tracker only counts the frame
    out = h.update(np.empty((0, 6)), IMG, None)
    assert out.shape == (0, 8) and h.frame_count == 1
    out = d.update(np.empty((0, 6)), IMG, None)  # the per_class decorator's np.empty((0, 8))
    assert out.shape == (0, 8) and d.frame_count == 1


def test_yaml_defaults_equal_the_reference():
    """configs/trackers/hybridsort.yaml against the captured defaults of the reference's YAML.
    (DeepOCSort's captured defaults are kept beside them; its YAML is not shipped yet.)"""
    import inspect
    import json

    import yaml

    from boxmot_amd import DeepOcSort, HybridSort, get_tracker_config

    ref = json.loads((GOLDEN / "tracker_yaml_defaults.json").read_text())
    cfg = yaml.safe_load(open(get_tracker_config("hybridsort")))
    got = {k: v["default"] for k, v in cfg.items()}
    assert got == ref["hybridsort"] and list(got) == list(ref["hybridsort"])
    assert all(type(got[k]) is type(ref["hybridsort"][k]) for k in got)
    assert set(got) <= set(inspect.signature(HybridSort.__init__).parameters)
    # the reference's deepocsort.yaml spells iou_threshold `iou_thresh`: it falls into **kwargs
    names = set(inspect.signature(DeepOcSort.__init__).parameters)
    assert set(ref["deepocsort"]) - names == {"iou_thresh"}
    assert HybridSort(None, None, False, **got)._params.asso_func == "hmiou"


def test_per_class_engine_has_one_sequence_per_class(monkeypatch):
    from boxmot_amd.trackers import deepocsort as dmod
    from boxmot_amd.trackers import hybridsort as hmod

    seen = []

    class Probe:
        def __init__(self, **kw):
            seen.append(kw)
            raise RuntimeError("probe")

    monkeypatch.setattr(dmod, "DeepOcsortEngine", Probe)
    monkeypatch.setattr(hmod, "HybridsortEngine", Probe)
    with pytest.raises(RuntimeError, match="probe"):
        dmod.DeepOcSortPerClass(embedding_off=True)
    with pytest.raises(RuntimeError, match="probe"):
        dmod.DeepOcSortPerClass(embedding_off=True, nr_classes=3)
    h = hmod.HybridSortPerClass(None, None, False, 0.3, nr_classes=5)
    with pytest.raises(RuntimeError, match="probe"):
        h.update(np.array([[0, 0, 9, 9, 0.9, 1]]), IMG, np.ones((1, 4)))
    assert [k["n_seq"] for k in seen] == [80, 3, 5] and seen[2]["emb_dim"] == 4


def test_batched_engine_of_the_flow(monkeypatch):
    """run_sequences builds HybridSort's engine from the drop-in's constructor; n_classes asks for
    that many class sequences per sequence."""
    import boxmot_amd.engine as E

    seen = []

    class Probe:
        def __init__(self, **kw):
            seen.append(kw)

    monkeypatch.setattr(E, "HybridsortEngine", Probe)
    monkeypatch.setattr(E, "DeepOcsortEngine", Probe)
    eng, dt, ncol = motio._batched_engine("hybridsort", 4, 16, {"max_age": 9})
    assert (dt, ncol, eng.n_classes) == (np.float32, 8, 0)
    assert seen[-1]["n_seq"] == 4 and seen[-1]["emb_dim"] == 16
    assert seen[-1]["params"].max_age == 9 and seen[-1]["params"].det_thresh == 0.3
    eng, _, _ = motio._batched_engine("hybridsort", 4, 16, {}, 3)
    assert seen[-1]["n_seq"] == 12 and eng.n_classes == 3
    eng, _, _ = motio._batched_engine("deepocsort", 2, 16, {"max_age": 9}, 5)
    assert seen[-1]["n_seq"] == 10 and eng.n_classes == 5 and seen[-1]["params"].max_age == 9
    n = len(seen)
    with pytest.raises(NotImplementedError, match="n_classes"):
        motio._batched_engine("ocsort", 2, 0, {}, 3)
    assert len(seen) == n
    eng, _, _ = motio._batched_engine("deepocsort", 2, 16, {})
    assert seen[-1]["n_seq"] == 2 and eng.n_classes == 0


@pytest.mark.parametrize("path", sorted(GOLDEN.glob("perclass_deepoc_*.npz")) + sorted(GOLDEN.glob("perclass_hybrid_*.npz")), ids=lambda p: p.stem)
def test_perclass_fixture_covers_its_branches(path):
    with np.load(path) as fx:
        for k in ast.literal_eval(str(fx["needs"])):
            assert int(fx[k]) > 0, k
        assert int(fx["lap_degenerate"]) == 0 and int(fx["nr_classes"]) == 3
        out = fx["outputs"]
        assert out.shape[1] == 9 and int(fx["n_frames"]) == 30
        assert set(out[:, 7].astype(int)) == {0, 1}  # class 2 never populated, class 4 dropped
        # rows of a frame come in class order
        for t in np.unique(out[:, 0]):
            c = out[out[:, 0] == t][:, 7]
            assert (np.diff(c) >= 0).all()
        assert path.stat().st_size < 64 * 1024


def test_split_scene_is_shared_by_maker_and_tests():
    from tests.perclass_util import CLASSES, NR_CLASSES, fixture_frames

    with np.load(GOLDEN / "perclass_deepoc_crowd24.npz") as fx:
        frames = fixture_frames(fx)
        blank = set(int(t) for t in fx["blank_frames"])
    assert len(frames) == 30 and NR_CLASSES == 3 and max(CLASSES) >= NR_CLASSES
    for t, d, e in frames:
        assert d.shape[0] == e.shape[0] and e.shape[1] == 16 and e.dtype == np.float64
        assert (t in blank) == (not (d[:, 5] == 1).any())

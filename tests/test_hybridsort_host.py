"""HybridSort's drop-in surface without a GPU: imports, the reference's constructor defaults,
parameters reaching the engine parameters, what is out of scope, input errors."""
import inspect

import numpy as np
import pytest

from boxmot_amd import HybridSort
from boxmot_amd.trackers import HybridSort as HybridSortFromTrackers

IMG = np.zeros((1080, 1920, 3), np.uint8)


def make(**kw):
    kw.setdefault("det_thresh", 0.3)
    return HybridSort(reid_weights=None, device="cpu", half=False, **kw)


def test_imports():
    import boxmot_amd
    import boxmot_amd.trackers

    assert HybridSort is HybridSortFromTrackers
    assert "HybridSort" in boxmot_amd.__all__ and "HybridSort" in boxmot_amd.trackers.__all__
    from boxmot_amd.engine import HybridsortEngine, HybridsortParams  # noqa: F401


def test_constructor_signature_and_defaults():
    """hybridsort.py:372-388, as literals."""
    sig = inspect.signature(HybridSort.__init__)
    names = list(sig.parameters)
    assert names[:16] == ["self", "reid_weights", "device", "half", "det_thresh", "per_class",
                          "max_age", "min_hits", "iou_threshold", "delta_t", "asso_func",
                          "inertia", "longterm_reid_weight", "TCM_first_step_weight", "use_byte",
                          "track_cap"]
    assert names[16:] == ["det_cap"]
    for required in ("reid_weights", "device", "half", "det_thresh"):
        assert sig.parameters[required].default is inspect.Parameter.empty
    defaults = {k: p.default for k, p in sig.parameters.items()
                if p.default is not inspect.Parameter.empty}
    assert defaults == dict(per_class=False, max_age=30, min_hits=3, iou_threshold=0.3, delta_t=3,
                            asso_func="iou", inertia=0.2, longterm_reid_weight=0,
                            TCM_first_step_weight=0, use_byte=False, track_cap=256, det_cap=256)
    tr = make()
    assert (tr.max_age, tr.min_hits, tr.iou_threshold, tr.delta_t, tr.inertia) == (30, 3, 0.3, 3,
                                                                                   0.2)
    assert tr.frame_count == 0 and tr.engine is None and tr.active_tracks == []


def test_parameters_reach_the_engine_parameters():
    tr = make(det_thresh=0.45, max_age=17, min_hits=2, iou_threshold=0.25, delta_t=2,
              asso_func="giou", inertia=0.15, longterm_reid_weight=0.5, TCM_first_step_weight=1.0,
              track_cap=64, det_cap=48)
    p = tr._params
    assert (p.det_thresh, p.max_age, p.min_hits, p.iou_threshold, p.delta_t, p.asso_func,
            p.inertia, p.longterm_reid_weight, p.TCM_first_step_weight) == (
                0.45, 17, 2, 0.25, 2, "giou", 0.15, 0.5, 1.0)
    assert tr._caps == (64, 48)
    from boxmot_amd.engine import HybridsortParams

    d = HybridsortParams()
    assert (d.max_age, d.min_hits, d.iou_threshold, d.delta_t, d.asso_func, d.inertia,
            d.longterm_reid_weight, d.TCM_first_step_weight) == (30, 3, 0.3, 3, "iou", 0.2, 0.0,
                                                                 0.0)


def test_out_of_scope_modes_raise():
    with pytest.raises(NotImplementedError, match="use_byte"):
        make(use_byte=True)
    with pytest.raises(NotImplementedError, match="per_class"):
        make(per_class=True)


def test_input_errors():
    tr = make()
    with pytest.raises(AssertionError):  # 5 columns: no class column
        tr.update(np.zeros((2, 5)), IMG, np.zeros((2, 8)))
    with pytest.raises(AssertionError):  # detection and embedding rows differ
        tr.update(np.zeros((2, 6)), IMG, np.zeros((3, 8)))
    with pytest.raises(AssertionError):
        tr.update([[0, 0, 1, 1, 0.9, 0]], IMG, np.zeros((1, 8)))
    # an empty frame before any detection needs no engine (and no GPU)
    out = tr.update(np.empty((0, 6)), IMG, None)
    assert out.shape == (0, 8) and tr.frame_count == 1


def test_create_tracker_still_raises():
    from boxmot_amd import create_tracker

    with pytest.raises(NotImplementedError):
        create_tracker("hybridsort", evolve_param_dict={})

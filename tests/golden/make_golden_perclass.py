#!/usr/bin/env python
"""Generate the per_class=True fixtures tests/golden/perclass_{deepoc,hybrid}_<name>.npz from the
Python reference (BaseTracker.per_class_decorator, boxmot/trackers/basetracker.py:155-201, over
DeepOcSort and HybridSort), on the CPU.

Same shim and run-time patches as make_golden_deepocsort.py and make_golden_hybridsort.py (their
functions are imported, nothing is edited): P1-P5 and the restated lapx for both, H1-H3 for
HybridSort.  Neither tracker needed a further patch for a class call without detections: both
run their update on an empty ``dets`` (the class's tracks age, none is born).

Scene (tests/perclass_util.py): 24 identities, classes 0 and 1 populated, class 2 never, two
identities of class 4 >= nr_classes = 3; 16-wide float64 embeddings; 30 frames; the rows of class
1 are taken out in a few frames.  ``tracker.nr_classes`` is set to 3 after construction (the
constructors do not take it).  A fixture is written only if the run contains
  both_births     a frame with births in two classes (the class-global id order),
  empty_calls     a class call without detections on a class that has live tracks,
  empty_deaths    a track dying in such a call,
  oru_class1      an ORU replay (a track found again after a gap) in class 1,
  dropped_rows    rows whose class is >= nr_classes.

The files are named ``perclass_*`` (not ``deepoc_*`` / ``hybrid_*``: the two trackers' own suites
glob those patterns and expect their makers' layout).

Usage: ``python tests/golden/make_golden_perclass.py [name ...]`` (no argument = all).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

import make_golden_deepocsort as mgd  # noqa: E402
import make_golden_hybridsort as mgh  # noqa: E402
from make_golden import (IdentityCMC, install_ocsort_patches, install_shim,  # noqa: E402
                         use_restated_lapx_jv)

from boxmot_amd.synth import SyntheticScene  # noqa: E402
from tests.perclass_util import CLASSES, NR_CLASSES, perclass_frames  # noqa: E402

SCENE = dict(n_obj=24, layout="crowded", emb_dim=16, emb_dtype="float64", conf_lo=0.31,
             jitter=6.0, p_det=0.8, classes=CLASSES)
NF = 30
BLANK = dict(blank_class=1, blank_frames=(12, 13, 14, 15, 16, 17))
# max_age 4: tracks of class 1 last seen at frame 12 or 13 die during the blank frames, the ones
# seen at frame 11 come back at 18 through ORU
T = dict(max_age=4, min_hits=2)

# name, kind, scene, tracker args
CASES = [
    ("perclass_deepoc_crowd24", "deepocsort", dict(SCENE, seed=90), dict(T, cmc_off=True)),
    ("perclass_hybrid_crowd24", "hybridsort", dict(SCENE, seed=91), dict(T, det_thresh=0.3)),
    ("perclass_hybrid_longterm", "hybridsort", dict(SCENE, seed=92),
     dict(T, det_thresh=0.3, longterm_reid_weight=0.5, TCM_first_step_weight=1.0)),
]
NEED = ["both_births", "empty_calls", "empty_deaths", "oru_class1", "dropped_rows"]


def instrument_classes(count, mods):
    """Counters of the per-class branches, on top of the makers' own."""
    from boxmot.motion.kalman_filters.aabb.xysr_kf import KalmanFilterXYSR
    from boxmot.trackers.basetracker import BaseTracker

    state = {"cls": -1, "births": {}}
    get = BaseTracker.get_class_dets_n_embs

    def get_counted(self, dets, embs, cls_id):
        state["cls"] = cls_id
        if cls_id == 0:
            if sum(1 for v in state["births"].values() if v) >= 2:
                count["both_births"] += 1
            state["births"] = {}
        d, e = get(self, dets, embs, cls_id)
        if len(d) == 0 and len(self.per_class_active_tracks[cls_id]):
            count["empty_calls"] += 1
            state["empty"] = True
        else:
            state["empty"] = False
        return d, e

    BaseTracker.get_class_dets_n_embs = get_counted
    for mod in mods:
        init = mod.KalmanBoxTracker.__init__

        def init_counted(self, *a, _init=init, **k):
            state["births"][state["cls"]] = state["births"].get(state["cls"], 0) + 1
            return _init(self, *a, **k)

        mod.KalmanBoxTracker.__init__ = init_counted
    unfreeze = KalmanFilterXYSR.unfreeze

    def unfreeze_counted(self):
        if self.attr_saved is not None and state["cls"] == 1:
            count["oru_class1"] += 1
        return unfreeze(self)

    KalmanFilterXYSR.unfreeze = unfreeze_counted
    return state


def run(tracker, frames, count, state, held):
    import lap

    lap.STATS["calls"] = 0
    lap.STATS["degenerate"] = 0
    img = np.zeros((1080, 1920, 3), np.uint8)
    rows = []
    for fno, dets, embs in frames:
        held["embs"] = None
        cls = np.asarray(dets, np.float32)[:, 5]
        count["dropped_rows"] += int((~((cls >= 0) & (cls < NR_CLASSES) & (cls == np.floor(cls)))).sum())
        before = {c: len(v) for c, v in tracker.per_class_active_tracks.items()}
        out = np.asarray(tracker.update(dets, img, embs), dtype=np.float64).reshape(-1, 8)
        for c in range(NR_CLASSES):
            n_c = int((cls == c).sum())
            if n_c == 0 and before[c] and len(tracker.per_class_active_tracks[c]) < before[c]:
                count["empty_deaths"] += before[c] - len(tracker.per_class_active_tracks[c])
        rows.append(np.concatenate([np.full((out.shape[0], 1), fno, np.float64), out], 1))
    return np.concatenate(rows, 0), dict(lap.STATS)


def main():
    only = set(sys.argv[1:])
    install_shim()
    install_ocsort_patches()
    use_restated_lapx_jv()
    import boxmot.motion.cmc  # noqa: F401  (so that the replacements below are not overwritten)

    mgh.install_h1()
    import boxmot.trackers.deepocsort.deepocsort as dmod
    import boxmot.trackers.hybridsort.hybridsort as hmod

    dmod.get_cmc_method = lambda name: IdentityCMC
    hmod.get_cmc_method = lambda name: IdentityCMC
    dcount = dict.fromkeys(mgd.COUNTERS, 0)
    hcount = dict.fromkeys(mgh.COUNTERS, 0)
    mgd.instrument(dcount)
    mgh.instrument(hcount)
    count = dict.fromkeys(NEED, 0)
    state = instrument_classes(count, [dmod, hmod])
    for name, kind, skw, tkw in CASES:
        if only and name not in only:
            continue
        for c in (count, dcount, hcount):
            for k in c:
                c[k] = 0
        state["births"] = {}
        scene = SyntheticScene(**skw)
        held = {}
        if kind == "deepocsort":
            tracker = dmod.DeepOcSort(reid_weights=None, device="cpu", half=False, per_class=True,
                                      **tkw)
        else:
            tracker = hmod.HybridSort(reid_weights=None, device="cpu", half=False, per_class=True,
                                      **tkw)
            # H2: the class call's own embeddings (update() ignores its ``embs`` argument)
            get = tracker.get_class_dets_n_embs

            def get_held(dets, embs, cls_id, _get=get):
                d, e = _get(dets, embs, cls_id)
                held["embs"] = e
                return d, e

            tracker.get_class_dets_n_embs = get_held
            tracker.model.get_features = lambda *a, **k: np.asarray(held["embs"], np.float64).copy()
        tracker.nr_classes = NR_CLASSES
        frames = perclass_frames(scene, NF, BLANK["blank_class"], BLANK["blank_frames"])
        outs, stats = run(tracker, frames, count, state, held)
        extra = dcount if kind == "deepocsort" else hcount
        print(f"{name}: rows={outs.shape[0]} lap={stats} {count} {extra}")
        for k in NEED:
            assert count[k] > 0, f"{name} never reached {k}: change the seed or the blank frames"
        assert stats["degenerate"] == 0, f"{name}: a LAP call ties: change the seed"
        np.savez_compressed(
            HERE / f"{name}.npz", outputs=outs, n_frames=NF, kind=kind, scene=repr(skw),
            tracker_args=repr(tkw), nr_classes=NR_CLASSES, blank_class=BLANK["blank_class"],
            blank_frames=np.array(BLANK["blank_frames"], np.int32), lap_calls=stats["calls"],
            lap_degenerate=stats["degenerate"], needs=repr(NEED), **count,
            **{f"ref_{k}": v for k, v in extra.items()})


if __name__ == "__main__":
    main()

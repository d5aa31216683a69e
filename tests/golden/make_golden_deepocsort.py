#!/usr/bin/env python
"""Generate the DeepOCSort fixtures tests/golden/deepoc_<name>.npz from the Python reference
(boxmot/trackers/deepocsort/deepocsort.py), on the CPU.

Same shim as make_golden.py (imported, not edited): the synthetic ``boxmot`` package over the
reference tree, the OCSort patches P1-P5 of ``utils/association.py`` / ``xyxy2xysr`` (installed
BEFORE the reference's deepocsort module is imported: it binds ``xyxy2xysr`` and ``associate`` by
name) and lapx's lapjv restated (``use_restated_lapx_jv``), so full-matching ties resolve in lapx's
published order.  The module's ``get_cmc_method`` is replaced so the constructor never touches
OpenCV; ``tracker.cmc`` is set afterwards.

Files are named ``deepoc_*`` (not ``trk_*``: the parity and oracle suites glob that pattern).
Each holds only the outputs, the scene/tracker arguments (scenes are regenerated from their seeds
at test time; all embeddings float64), ``warp_seed`` where a CMC warp is used, the LAP tie
statistics and coverage counters taken by wrapping the reference's own functions.  A case is
written only if every counter its row below names is > 0: a fixture that does not reach its
branch pins nothing.

Usage: ``python tests/golden/make_golden_deepocsort.py [name ...]`` (no argument = all).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

from make_golden import (IdentityCMC, install_ocsort_patches, install_shim,  # noqa: E402
                         run_tracker, synth_frames, use_restated_lapx_jv)

from boxmot_amd.synth import SyntheticCMC, SyntheticScene, synth_warp  # noqa: E402

F64 = "float64"  # SyntheticScene(emb_dtype=...) as it is stored in the fixture
# jitter 6 px: the velocity estimates get noisy enough that predictions drift off objects
# whose last observation still overlaps them, which is what reaches the OCR round
CROWD40 = dict(n_obj=40, layout="crowded", emb_dim=64, emb_dtype=F64, conf_lo=0.31, jitter=6.0)

# name, scene, tracker args, frames, warp seed or None, counters that must be > 0
CASES = [
    ("grid24_f20", dict(n_obj=24, seed=70, emb_dim=20, emb_dtype=F64), dict(cmc_off=True), 60,
     None, ["fast_frames"]),
    ("crowd40_f64", dict(CROWD40, seed=71), dict(cmc_off=True), 100, None,
     ["lap_frames", "ocr_rematches", "oru_unfreezes"]),
    ("crowd40_awoff", dict(CROWD40, seed=72), dict(cmc_off=True, aw_off=True,
                                                   w_association_emb=0.75), 100, None,
     ["lap_frames"]),
    ("crowd40_emboff", dict(CROWD40, seed=72), dict(cmc_off=True, embedding_off=True), 100, None,
     ["lap_frames"]),
    ("crowd32_warp", dict(n_obj=32, seed=73, layout="crowded", emb_dim=48, emb_dtype=F64,
                          conf_lo=0.31), {}, 100, 73,
     ["lap_frames", "oru_unfreezes", "affine_frozen"]),
    ("crowd96_f32", dict(n_obj=96, seed=74, layout="crowded", emb_dim=32, emb_dtype=F64,
                         conf_lo=0.31, p_det=0.8), dict(cmc_off=True), 40, None,
     ["lap_frames", "frames_gt64"]),
    ("giou_crowd40", dict(CROWD40, seed=75), dict(cmc_off=True, asso_func="giou"), 100, None,
     ["lap_frames", "ocr_rematches"]),
]

COUNTERS = ["lap_frames", "fast_frames", "ocr_rematches", "oru_unfreezes", "affine_frozen",
            "frames_gt64"]


def instrument(count):
    """Wrap the reference's functions so that `count` sees which branches a run takes."""
    import boxmot.trackers.deepocsort.deepocsort as mod
    import boxmot.utils.association as assoc
    from boxmot.motion.kalman_filters.aabb.xysr_kf import KalmanFilterXYSR

    state = {"ocr": False, "lap": False}

    first_lap = assoc.linear_assignment  # the LAP branch of enhanced_associate (P4)

    def lap_first(cost):
        state["lap"] = True
        return first_lap(cost)

    assoc.linear_assignment = lap_first

    associate = mod.associate

    def associate_counted(dets, trks, *a, **k):
        state["lap"] = False
        state["ocr"] = False
        out = associate(dets, trks, *a, **k)
        if len(trks) > 64:
            count["frames_gt64"] += 1
        if len(trks) and len(dets):
            count["lap_frames" if state["lap"] else "fast_frames"] += 1
        return out

    mod.associate = associate_counted

    ocr_lap = mod.linear_assignment  # deepocsort.py:438

    def lap_ocr(cost):
        state["ocr"] = True
        return ocr_lap(cost)

    mod.linear_assignment = lap_ocr

    trk_update = mod.KalmanBoxTracker.update

    def update(self, det):
        if det is not None and state["ocr"]:
            count["ocr_rematches"] += 1
        return trk_update(self, det)

    mod.KalmanBoxTracker.update = update

    unfreeze = KalmanFilterXYSR.unfreeze

    def unfreeze_counted(self):
        if self.attr_saved is not None:
            count["oru_unfreezes"] += 1
        return unfreeze(self)

    KalmanFilterXYSR.unfreeze = unfreeze_counted

    affine = KalmanFilterXYSR.apply_affine_correction

    def affine_counted(self, m, t):
        if not self.observed and self.attr_saved is not None:
            count["affine_frozen"] += 1
        return affine(self, m, t)

    KalmanFilterXYSR.apply_affine_correction = affine_counted
    return mod


def run_warped(tracker, cmc, frames):
    import lap

    lap.STATS["calls"] = 0
    lap.STATS["degenerate"] = 0
    img = np.zeros((1080, 1920, 3), np.uint8)
    rows = []
    for fno, dets, embs in frames:
        cmc.t = fno
        out = np.asarray(tracker.update(dets, img, embs), dtype=np.float64).reshape(-1, 8)
        rows.append(np.concatenate([np.full((out.shape[0], 1), fno, np.float64), out], 1))
    return np.concatenate(rows, 0), dict(lap.STATS)


def main():
    only = set(sys.argv[1:])
    install_shim()
    install_ocsort_patches()
    use_restated_lapx_jv()
    import boxmot.motion.cmc  # noqa: F401  (so that the replacement below is not overwritten)

    count = dict.fromkeys(COUNTERS, 0)
    import boxmot.trackers.deepocsort.deepocsort as mod

    mod.get_cmc_method = lambda name: IdentityCMC
    instrument(count)
    for name, skw, tkw, nf, wseed, need in CASES:
        if only and name not in only:
            continue
        for k in count:
            count[k] = 0
        scene = SyntheticScene(**skw)
        assert nf <= 120 and scene.emb_dtype == F64
        tracker = mod.DeepOcSort(reid_weights=None, device="cpu", half=False, **tkw)
        if wseed is None:
            outs, stats = run_tracker(tracker, synth_frames(scene, nf))
        else:
            cmc = SyntheticCMC(lambda t, s=wseed: synth_warp(s, t))
            tracker.cmc = cmc
            outs, stats = run_warped(tracker, cmc, synth_frames(scene, nf))
        print(f"{name}: rows={outs.shape[0]} lap={stats} {count}")
        for k in need:
            assert count[k] > 0, f"{name} never reached {k}: change the seed or p_det"
        extra = {} if wseed is None else {"warp_seed": wseed}
        np.savez_compressed(
            HERE / f"deepoc_{name}.npz", outputs=outs, n_frames=nf, kind="deepocsort",
            scene=repr(skw), tracker_args=repr(tkw), lap_calls=stats["calls"],
            lap_degenerate=stats["degenerate"], **count, **extra)


if __name__ == "__main__":
    main()

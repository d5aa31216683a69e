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
Each holds the outputs, the reference's per-track state after four of its frames (``state_*``:
ids, kf.x, kf.P and, unless ``embedding_off``, the embedding, in list order: the layout of
``DeepOcsortEngine.tracks()``), the scene/tracker arguments as ``repr`` (scenes are regenerated
from them at test time, tests/scenes.py; all embeddings float64), ``warp_seed`` where a CMC warp
is used, the LAP tie statistics, coverage counters taken by wrapping the reference's own
functions, and ``needs``: the counters the case is there for.  A case is written only if every
counter in ``needs`` is > 0 (a fixture that does not reach its branch pins nothing), only if no
LAP call of it ties (five captures older than that rule are listed in TIED), and, where the file
exists, only if its ``outputs`` are the file's byte for byte: a regeneration adds to a fixture
and replaces nothing.

Usage: ``python tests/golden/make_golden_deepocsort.py [name ...]`` (no argument = all).
``name@seed`` runs the case with another scene seed and prints its counters without writing:
how the seeds below were chosen.
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
from tests.scenes import DEEPOC_TIED as TIED, LDS_COST_MAX, StopScene  # noqa: E402

F64 = "float64"  # SyntheticScene(emb_dtype=...) as it is stored in the fixture
# jitter 6 px: the velocity estimates get noisy enough that predictions drift off objects
# whose last observation still overlaps them, which is what reaches the OCR round
CROWD40 = dict(n_obj=40, layout="crowded", emb_dim=64, emb_dtype=F64, conf_lo=0.31, jitter=6.0)

# The scene seeds of the cases added off the defaults: for each the first seed, counting up
# from its first try, at which the reference alone reaches the case's counters without a tied
# LAP call and, for a case in TWIN, runs differently than under the twin function (``name@seed``
# prints a try).  The OCR round's -iou cost ties on its exact zeros: with IoU, dt7_warp tied at
# seeds 110-120 and params at 120-130; dt1_short tied at every seed 100-130 and runs on GIoU,
# which has no such zeros, as HybridSort's noisy cases do (so delta_t = 1 with a short max_age
# is pinned for GIoU only).  hmiou on the ASSO32 scene ran exactly as iou does (seeds 130-132)
# and runs with 7 px of jitter: seed 132 tied, 133 is taken.  ciou on ASSO32 ran exactly as diou
# does (seed 140) and runs on HARD40: seeds 140-143 still did, 144 is taken.
SEEDS = dict(dt1_short=100, dt7_warp=121, params=131, hmiou=133, ciou=144, diou=150, centroid=160,
             stop76=170)

# A crowded scene whose detections come and go (p_det 0.6): ages have gaps, tracks are lost and
# found again (ORU), and with max_age 5 they die
GAPPY32 = dict(n_obj=32, layout="crowded", emb_dim=32, emb_dtype=F64, conf_lo=0.31, jitter=4.0,
               p_det=0.6)
# 40 frames of a crowded 32-object scene for the association functions
ASSO32 = dict(n_obj=32, layout="crowded", emb_dim=32, emb_dtype=F64, conf_lo=0.31, jitter=4.0,
              p_det=0.8)
# ciou: 40 objects and 10 px of jitter, so that heights and aspect ratios of a pair
# differ and pairs sit near the threshold; with ASSO32 it ran exactly as diou does
HARD40 = dict(ASSO32, n_obj=40, jitter=10.0)
STOP76 = dict(n_obj=76, emb_dim=32)  # tests/scenes.py: StopScene

# name, scene, tracker args, frames, warp seed or None, counters that must be > 0
CASES = [
    ("grid24_f20", dict(n_obj=24, seed=70, emb_dim=20, emb_dtype=F64), dict(cmc_off=True), 60,
     None, ["fast_frames", "births"]),
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
     ["lap_frames", "frames_gt64", "first_big"]),
    ("giou_crowd40", dict(CROWD40, seed=75), dict(cmc_off=True, asso_func="giou"), 100, None,
     ["lap_frames", "ocr_rematches"]),
    # ---- off the defaults (every parameter below is at its default in the cases above)
    ("dt1_short", dict(GAPPY32, seed=SEEDS["dt1_short"]),
     dict(cmc_off=True, delta_t=1, max_age=5, min_hits=1, inertia=0.4, iou_threshold=0.2,
          asso_func="giou"), 100,
     None, ["deaths", "births", "oru_unfreezes"]),
    # delta_t 7: the look-backs and the affine correction touch all eight slots of the ring
    ("dt7_warp", dict(GAPPY32, seed=SEEDS["dt7_warp"]), dict(delta_t=7), 100, 76,
     ["affine_frozen", "oru_unfreezes", "lookback_ge4"]),
    ("params", dict(n_obj=32, seed=SEEDS["params"], layout="crowded", emb_dim=32, emb_dtype=F64,
                    conf_lo=0.35, jitter=4.0, p_det=0.8),
     dict(cmc_off=True, Q_xy_scaling=0.02, Q_s_scaling=0.0002, alpha_fixed_emb=0.8, aw_param=0.3,
          w_association_emb=0.6, det_thresh=0.5), 100, None, ["below_thresh_dets", "lap_frames"]),
    ("hmiou", dict(ASSO32, jitter=7.0, seed=SEEDS["hmiou"]), dict(cmc_off=True, asso_func="hmiou"), 40, None,
     ["lap_frames"]),
    ("ciou", dict(HARD40, seed=SEEDS["ciou"]), dict(cmc_off=True, asso_func="ciou"), 40, None,
     ["lap_frames"]),
    ("diou", dict(ASSO32, seed=SEEDS["diou"]), dict(cmc_off=True, asso_func="diou"), 40, None,
     ["lap_frames"]),
    # 1 - distance / frame diagonal (of the 1920 x 1080 image the runs pass): a threshold near 1
    ("centroid", dict(ASSO32, seed=SEEDS["centroid"]),
     dict(cmc_off=True, asso_func="centroid", iou_threshold=0.97), 40, None, ["lap_frames"]),
    # the OCR round's cost matrix in global memory (tests/scenes.py)
    ("stop76", dict(STOP76, seed=SEEDS["stop76"]), dict(cmc_off=True), 12, None,
     ["ocr_big", "ocr_rematches"]),
]
# A case named for an association function is run a second time with the nearest other function
# (IoU without the height ratio; DIoU, which is CIoU without the aspect-ratio term; ...) and is
# written only if outputs or state differ: otherwise a kernel that falls through to the other
# function would pass it
TWIN = {"hmiou": "iou", "ciou": "diou", "diou": "iou", "centroid": "iou"}


def same_capture(a, b):
    """Two captures (outputs, state dict) are the same bytes."""
    return a[0].tobytes() == b[0].tobytes() and a[1].keys() == b[1].keys() and all(
        a[1][k].tobytes() == b[1][k].tobytes() for k in a[1])


COUNTERS = ["lap_frames", "fast_frames", "ocr_rematches", "oru_unfreezes", "affine_frozen",
            "frames_gt64", "deaths", "births", "below_thresh_dets", "lookback_ge4", "ocr_big",
            "first_big"]


def count_lookback(count, observations, cur_age, k, got):
    """`got` is what a look-back over ages cur_age-k .. cur_age-1 returned: counted where it is
    the entry of an age in that window at least 4 back (the far slots of the engine's ring)."""
    for a, o in observations.items():
        if o is got and 4 <= cur_age - a <= k:
            count["lookback_ge4"] += 1


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
        if len(trks) * len(dets) > LDS_COST_MAX:
            count["first_big"] += 1
        if len(trks) and len(dets):
            count["lap_frames" if state["lap"] else "fast_frames"] += 1
        return out

    mod.associate = associate_counted

    ocr_lap = mod.linear_assignment  # deepocsort.py:438

    def lap_ocr(cost):
        state["ocr"] = True
        if cost.shape[0] * cost.shape[1] > LDS_COST_MAX:
            count["ocr_big"] += 1
        return ocr_lap(cost)

    mod.linear_assignment = lap_ocr

    previous = mod.k_previous_obs

    def previous_counted(observations, cur_age, k):
        got = previous(observations, cur_age, k)
        count_lookback(count, observations, cur_age, k, got)
        return got

    mod.k_previous_obs = previous_counted

    trk_init, trk_update = mod.KalmanBoxTracker.__init__, mod.KalmanBoxTracker.update

    def init(self, *a, **k):
        count["births"] += 1
        return trk_init(self, *a, **k)

    def update(self, det):
        if det is not None and state["ocr"]:
            count["ocr_rematches"] += 1
        if det is not None and any(self.age - dt in self.observations
                                   for dt in range(4, self.delta_t + 1)):
            count["lookback_ge4"] += 1  # update()'s own look-back starts at the oldest age
        return trk_update(self, det)

    mod.KalmanBoxTracker.__init__, mod.KalmanBoxTracker.update = init, update

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


def snapshot(tracker):
    """The reference's per-track state in list order, as tracks() of the engine reports it."""
    tr = tracker.active_tracks
    snap = dict(
        id=np.array([t.id for t in tr], np.int32),
        x=np.array([t.kf.x[:, 0] for t in tr], np.float64).reshape(-1, 7),
        P=np.array([t.kf.P for t in tr], np.float64).reshape(-1, 7, 7))
    if not tracker.embedding_off:
        F = tr[0].emb.shape[0] if tr else 0
        snap["emb"] = np.array([t.emb for t in tr], np.float64).reshape(-1, F)
    return snap


def run(tracker, frames, count, snap_at=(), cmc=None):
    import lap

    lap.STATS["calls"] = 0
    lap.STATS["degenerate"] = 0
    img = np.zeros((1080, 1920, 3), np.uint8)
    rows, snaps = [], {}
    for fno, dets, embs in frames:
        if cmc is not None:
            cmc.t = fno
        scores = np.asarray(dets, np.float32)[:, 4]
        count["below_thresh_dets"] += int((~(scores > tracker.det_thresh)).sum())
        before, born = len(tracker.active_tracks), count["births"]
        out = np.asarray(tracker.update(dets, img, embs), dtype=np.float64).reshape(-1, 8)
        count["deaths"] += before + (count["births"] - born) - len(tracker.active_tracks)
        rows.append(np.concatenate([np.full((out.shape[0], 1), fno, np.float64), out], 1))
        if fno in snap_at:
            snaps[fno] = snapshot(tracker)
    return np.concatenate(rows, 0), dict(lap.STATS), snaps


def pack_state(snaps, snap_at):
    state = {f"state_{k}": np.concatenate([snaps[f][k] for f in snap_at], 0)
             for k in snaps[snap_at[-1]]}
    state["state_frames"] = np.array(snap_at, np.int32)
    state["state_off"] = np.concatenate(
        [[0], np.cumsum([snaps[f]["id"].shape[0] for f in snap_at])]).astype(np.int32)
    return state


def main():
    only = {}
    for a in sys.argv[1:]:
        name, _, seed = a.partition("@")
        only[name] = int(seed) if seed else None
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
        probe = only.get(name)
        if probe is not None:
            skw = dict(skw, seed=probe)
        stop = name.startswith("stop")
        scene = StopScene(**skw) if stop else SyntheticScene(**skw)
        assert nf <= 120 and (stop or scene.emb_dtype == F64)
        snap_at = [nf // 4, nf // 2, 3 * nf // 4, nf]

        def capture(args, into):
            for k in into:
                into[k] = 0
            tracker = mod.DeepOcSort(reid_weights=None, device="cpu", half=False, **args)
            cmc = None
            if wseed is not None:
                cmc = tracker.cmc = SyntheticCMC(lambda t, s=wseed: synth_warp(s, t))
            o, st, sn = run(tracker, synth_frames(scene, nf), into, snap_at, cmc)
            return o, st, pack_state(sn, snap_at)

        differs = ""
        if name in TWIN:
            twin = capture(dict(tkw, asso_func=TWIN[name]), count)
        outs, stats, state = capture(tkw, count)
        if name in TWIN:
            differs = f" differs from {TWIN[name]}: {not same_capture((outs, state), (twin[0], twin[2]))}"
        print(f"{name}: rows={outs.shape[0]} lap={stats} {count}{differs}")
        if probe is not None:
            continue
        assert name not in TWIN or not same_capture((outs, state), (twin[0], twin[2])), \
            f"{name}: the run is the same under {TWIN[name]}: change the seed or the scene"
        for k in need:
            assert count[k] > 0, f"{name} never reached {k}: change the seed or p_det"
        assert stats["degenerate"] == 0 or name in TIED, f"{name}: a LAP call ties: change the seed"
        if stop:  # (nearly) every object is found again by the OCR round in one frame
            assert count["ocr_rematches"] >= 72
        path = HERE / f"deepoc_{name}.npz"
        if path.exists():
            with np.load(path) as old:
                assert old["outputs"].tobytes() == outs.tobytes(), f"{name}: the outputs changed"
        extra = {} if wseed is None else {"warp_seed": wseed}
        if stop:
            extra["scene_kind"] = "stop"
        np.savez_compressed(
            path, outputs=outs, n_frames=nf, kind="deepocsort",
            scene=repr(skw), tracker_args=repr(tkw), lap_calls=stats["calls"],
            lap_degenerate=stats["degenerate"], needs=repr(need), **count,
            **state, **extra)


if __name__ == "__main__":
    main()

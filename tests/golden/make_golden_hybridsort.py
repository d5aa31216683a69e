#!/usr/bin/env python
"""Generate the HybridSort fixtures tests/golden/hybrid_<name>.npz from the Python reference
(boxmot/trackers/hybridsort/{hybridsort,association}.py), on the CPU.

Same shim as make_golden.py (imported, not edited): the synthetic ``boxmot`` package over the
reference tree and lapx's lapjv restated (``use_restated_lapx_jv``), so that LAP ties would
resolve in lapx's published order.  The reference's HybridSort does not run as it stands, so it
is patched at run time (nothing of it is copied here):

H1  ORU for a 5-vector.  ``KalmanFilterXYSR.unfreeze`` unpacks ``x1, y1, s1, r1 = box1`` and so
    crashes on HybridSort's 5x1 measurements [x, y, s, c, r] as soon as a lost track is found
    again.  For a filter with ``dim_z == 5`` the reference's own ``unfreeze`` is run on the two
    anchor measurements with the score row taken out, so position and w, h are interpolated by
    exactly its code for four values, and every virtual box it replays is handed on as the 5x1
    column [x, y, s, c, r] with the score interpolated linearly, ``c = c1 + (i+1)*(c2-c1)/
    time_gap`` (the original Hybrid-SORT's behaviour).  Filters with ``dim_z == 4`` are untouched.
H2  Embeddings passed in.  ``update`` ignores ``embs`` and calls the ReID model;
    ``tracker.model.get_features`` returns a copy of the frame's ``embs``.
H3  The ``print("correction...")`` calls of association.py are silenced (and counted).
Also: the module's ``get_cmc_method`` is replaced so OpenCV is never touched (``ECC`` is False in
the reference: no warp is ever applied).  ``use_byte=True`` (the BYTE round calls ``update`` with
the wrong arguments) and per-class mode are out of scope.

Files are named ``hybrid_*`` (not ``trk_*``: the parity and oracle suites glob that pattern).
Each holds the outputs, the reference's per-track state after four of its frames (``state_*``:
ids, kf.x, kf.P, the four corner velocities, smooth_feat, the feature-bank mean and the number of
features pushed, in list order), the scene/tracker arguments as ``repr`` (scenes are regenerated from
their arguments at test time, tests/scenes.py; all embeddings float64), the frame count, the LAP
call and degenerate counts and branch counters taken by wrapping the reference's own functions.
A case is written only if every counter its row below names is > 0 and no LAP call was
degenerate (a fixture that does not reach its branch pins nothing), and, where the file exists,
only if its outputs and state are the file's: a regeneration adds to a fixture and replaces
nothing.

Usage: ``python tests/golden/make_golden_hybridsort.py [name ...]`` (no argument = all).
``name@seed`` runs the case with another scene seed and prints its counters without writing:
how the seeds of the cases off the defaults were chosen.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

from make_golden_deepocsort import TWIN, count_lookback, same_capture  # noqa: E402
from make_golden import IdentityCMC, install_shim, synth_frames, use_restated_lapx_jv  # noqa: E402

from boxmot_amd.synth import SyntheticScene  # noqa: E402
from tests.scenes import LDS_COST_MAX, StopScene  # noqa: E402

F64 = "float64"  # SyntheticScene(emb_dtype=...) as it is stored in the fixture
# jitter 6 px: the velocity estimates get noisy enough that predictions drift off objects whose
# last observation still overlaps them, which is what reaches the OCR round
CROWD40 = dict(n_obj=40, layout="crowded", emb_dim=64, emb_dtype=F64, conf_lo=0.31, jitter=6.0)
# The embeddings separate identities so well that the first round alone pairs every object it
# has a track for.  Seen one frame in eight, tracks do run out their max_age of 30 (deaths), and
# an object that comes back without a track of its own can only be caught by the OCR round
SPARSE40 = dict(CROWD40, seed=74, p_det=0.12)
NOISY40 = dict(CROWD40, emb_noise=3.0)
LO = dict(det_thresh=0.3)  # under the scenes' confidence range: every detection is kept

# Off the defaults (every parameter below is at its default in the cases before them): the noisy
# scene, so that motion decides, seen six frames in ten, so that ages have gaps; GIoU as in the
# noisy cases above.  40 frames of a crowded 32-object scene for the association functions.
GAPPY40 = dict(NOISY40, p_det=0.6)
ASSO32 = dict(n_obj=32, layout="crowded", emb_dim=32, emb_dtype=F64, conf_lo=0.31, jitter=4.0,
              p_det=0.8)
# ciou: 40 objects and 10 px of jitter, so that heights and aspect ratios of a pair
# differ and pairs sit near the threshold; with ASSO32 it ran exactly as diou does
HARD40 = dict(ASSO32, n_obj=40, jitter=10.0)
# The scene seeds of those cases: for each the first seed, counting up from its first try, at
# which the reference alone reaches the case's counters without a tied LAP call and, for a case
# in TWIN, runs differently than under the twin function.  The appearance term decides these
# runs: hmiou ran exactly as iou does on ASSO32 and on HARD40 (seeds 220-231), and with
# emb_noise 0.35 and 0.6 (220-233); at 1.0 and more it differs but the OCR round's cost ties
# (220-235); at 0.8 with 7 px of jitter seeds 220-229 tied and 230 is taken.  ciou on ASSO32 ran
# exactly as diou does (seed 230) and runs on HARD40: seeds 230-235 still did, 236 is taken.
SEEDS = dict(dt1_short=200, dt7=210, hmiou=230, ciou=236, centroid=240, stop76=250)

# name, scene, tracker args, frames, counters that must be > 0
CASES = [
    ("grid24_f20", dict(n_obj=24, seed=70, emb_dim=20, emb_dtype=F64), dict(LO), 60,
     ["lap_frames", "first_matches", "births"]),
    ("crowd40_f64", dict(SPARSE40), dict(LO), 120,
     ["oru_unfreezes", "ocr_rematches", "corrections", "deaths"]),
    ("crowd40_longterm", dict(SPARSE40), dict(LO, longterm_reid_weight=0.5,
                                              TCM_first_step_weight=1.0), 120,
     ["oru_unfreezes", "corrections"]),
    ("crowd40_giou", dict(SPARSE40), dict(LO, asso_func="giou"), 120, ["lap_frames"]),
    # the same objects seen every other frame: ten times the output rows of the sparse run
    ("crowd40_dense", dict(CROWD40, seed=71), dict(LO), 100,
     ["oru_unfreezes", "corrections", "bank_wraps"]),
    ("crowd96_f32", dict(n_obj=96, seed=74, layout="crowded", emb_dim=32, emb_dtype=F64,
                         conf_lo=0.31, p_det=0.8), dict(LO), 40, ["frames_gt64", "first_big"]),
    ("grid16_long", dict(n_obj=16, seed=76, emb_dim=24, emb_dtype=F64, p_det=0.9), dict(LO), 60,
     ["bank_wraps"]),
    # The cases above are decided by the appearance term alone (1.3 * emb separates identities)
    # and their output boxes are observations, so on their own they pin little of the filter.
    # With emb_noise 3 the features hardly tell identities apart: the IoU, the corner directions
    # and the score difference decide the LAP and the correction rule drops every low-IoU pair.
    # That sends a hundred pairs and more through the OCR round, whose -iou cost ties on its
    # exact zeros in every seed tried; GIoU and DIoU have no such zeros.
    ("noisy40_motion", dict(NOISY40, seed=80), dict(LO, asso_func="giou"), 80,
     ["oru_unfreezes", "ocr_rematches", "corrections", "deaths", "bank_wraps"]),
    ("noisy40_tcm_longterm", dict(NOISY40, seed=81, p_det=0.7),
     dict(LO, asso_func="diou", longterm_reid_weight=0.5, TCM_first_step_weight=1.0), 80,
     ["oru_unfreezes", "ocr_rematches", "corrections", "bank_wraps"]),
    ("crowd24_thresh", dict(n_obj=24, seed=77, layout="crowded", emb_dim=32, emb_dtype=F64,
                            conf_lo=0.35, p_det=0.8), dict(det_thresh=0.5), 60,
     ["below_thresh_dets", "births"]),
    ("dt1_short", dict(GAPPY40, seed=SEEDS["dt1_short"]),
     dict(LO, asso_func="giou", delta_t=1, max_age=5, min_hits=1, inertia=0.4, iou_threshold=0.2),
     100, ["ocr_rematches", "corrections", "deaths"]),
    # delta_t 7: the look-backs touch all eight slots of the ring
    ("dt7", dict(GAPPY40, seed=SEEDS["dt7"]), dict(LO, asso_func="giou", delta_t=7, max_age=5),
     100, ["ocr_rematches", "corrections", "deaths", "lookback_ge4"]),
    ("hmiou", dict(ASSO32, jitter=7.0, emb_noise=0.8, seed=SEEDS["hmiou"]),
     dict(LO, asso_func="hmiou"), 40, ["lap_frames"]),
    ("ciou", dict(HARD40, seed=SEEDS["ciou"]), dict(LO, asso_func="ciou"), 40, ["lap_frames"]),
    # 1 - distance / frame diagonal (of the 1920 x 1080 image the runs pass): a threshold near 1
    ("centroid", dict(ASSO32, seed=SEEDS["centroid"]),
     dict(LO, asso_func="centroid", iou_threshold=0.97), 40, ["lap_frames"]),
    # The OCR round's cost matrix in global memory (tests/scenes.py: StopScene, and why its
    # embeddings turn noisy at the stop)
    ("stop76", dict(n_obj=76, emb_dim=32, emb_noise_stopped=3.0, seed=SEEDS["stop76"]), dict(LO),
     12, ["ocr_big", "ocr_rematches"]),
]

COUNTERS = ["lap_frames", "first_matches", "births", "deaths", "ocr_rematches", "oru_unfreezes",
            "corrections", "frames_gt64", "bank_wraps", "below_thresh_dets", "lookback_ge4",
            "ocr_big", "first_big"]


def install_h1():
    """H1 (see the module docstring)."""
    from boxmot.motion.kalman_filters.aabb.xysr_kf import KalmanFilterXYSR

    reference_unfreeze = KalmanFilterXYSR.unfreeze

    def unfreeze(self):
        if self.dim_z != 5 or self.attr_saved is None:
            return reference_unfreeze(self)
        hist = self.history_obs
        seen = [k for k, z in enumerate(hist) if z is not None]
        k1, k2 = seen[-2], seen[-1]
        c1, c2 = hist[k1][3], hist[k2][3]
        time_gap = k2 - k1
        for k in (k1, k2):  # the anchors without their score row: [x, y, s, r]
            hist[k] = np.delete(hist[k], 3, axis=0)
        step = {"i": 0}
        update = KalmanFilterXYSR.update

        def update_with_score(box):
            i = step["i"]
            step["i"] += 1
            c = c1 + (i + 1) * (c2 - c1) / time_gap
            update(self, np.array([box[0], box[1], box[2], c, box[3]]).reshape((5, 1)))

        # unfreeze() swaps self.__dict__ for attr_saved before it replays: the hook rides in it
        self.attr_saved["update"] = update_with_score
        try:
            reference_unfreeze(self)
        finally:
            self.__dict__.pop("update", None)

    KalmanFilterXYSR.unfreeze = unfreeze


def instrument(count):
    """Wrap the reference's functions so that `count` sees which branches a run takes."""
    import boxmot.trackers.hybridsort.association as assoc
    import boxmot.trackers.hybridsort.hybridsort as mod
    from boxmot.motion.kalman_filters.aabb.xysr_kf import KalmanFilterXYSR

    state = {"ocr": False, "lap": False}

    def quiet_print(*a, **k):  # H3
        if a and a[0] == "correction:":
            count["corrections"] += 1

    assoc.print = quiet_print
    mod.print = quiet_print

    first_lap = assoc.linear_assignment  # the first round's (association.py:597)

    def lap_first(cost, *a, **k):
        state["lap"] = True
        return first_lap(cost, *a, **k)

    assoc.linear_assignment = lap_first

    associate = mod.associate_4_points_with_score_with_reid

    def associate_counted(dets, trks, *a, **k):
        state["lap"] = False
        state["ocr"] = False
        out = associate(dets, trks, *a, **k)
        if len(trks) > 64:
            count["frames_gt64"] += 1
        if len(trks) * len(dets) > LDS_COST_MAX:
            count["first_big"] += 1
        if state["lap"]:
            count["lap_frames"] += 1
        count["first_matches"] += len(out[0])
        return out

    mod.associate_4_points_with_score_with_reid = associate_counted

    ocr_lap = mod.linear_assignment  # hybridsort.py:679

    def lap_ocr(cost, *a, **k):
        state["ocr"] = True
        if cost.shape[0] * cost.shape[1] > LDS_COST_MAX:
            count["ocr_big"] += 1
        return ocr_lap(cost, *a, **k)

    mod.linear_assignment = lap_ocr

    previous = mod.k_previous_obs

    def previous_counted(observations, cur_age, k):
        got = previous(observations, cur_age, k)
        count_lookback(count, observations, cur_age, k, got)
        return got

    mod.k_previous_obs = previous_counted

    KBT = mod.KalmanBoxTracker
    trk_init, trk_update, trk_feat = KBT.__init__, KBT.update, KBT.update_features

    def init(self, *a, **k):
        count["births"] += 1
        self._bx_pushes = 0
        return trk_init(self, *a, **k)

    def update(self, bbox, *a, **k):
        if bbox is not None and state["ocr"]:
            count["ocr_rematches"] += 1
        if bbox is not None and any(self.age - dt in self.observations
                                    for dt in range(4, self.delta_t + 1)):
            count["lookback_ge4"] += 1  # update() sums over every age of the window
        return trk_update(self, bbox, *a, **k)

    def update_features(self, *a, **k):
        self._bx_pushes += 1
        if self._bx_pushes == 31:  # the 30-deep bank wraps
            count["bank_wraps"] += 1
        return trk_feat(self, *a, **k)

    KBT.__init__, KBT.update, KBT.update_features = init, update, update_features

    unfreeze = KalmanFilterXYSR.unfreeze  # (H1's)

    def unfreeze_counted(self):
        if self.attr_saved is not None:
            count["oru_unfreezes"] += 1
        return unfreeze(self)

    KalmanFilterXYSR.unfreeze = unfreeze_counted
    return mod


def snapshot(tracker):
    """The reference's per-track state in list order, as tracks() of the engine reports it."""
    tr = tracker.active_tracks
    F = tr[0].smooth_feat.shape[0] if tr else 0
    vel = np.zeros((len(tr), 4, 2))
    for k, t in enumerate(tr):
        for c, v in enumerate((t.velocity_lt, t.velocity_rt, t.velocity_lb, t.velocity_rb)):
            if v is not None:
                vel[k, c] = v
    vel32 = vel.astype(np.float32)  # the reference holds them in float32: stored as that
    assert np.array_equal(vel32, vel)
    vel = vel32
    return dict(
        id=np.array([t.id + 1 for t in tr], np.int32),
        x=np.array([t.kf.x[:, 0] for t in tr], np.float64).reshape(-1, 9),
        P=np.array([t.kf.P for t in tr], np.float64).reshape(-1, 9, 9),
        vel=vel,
        emb=np.array([t.smooth_feat for t in tr], np.float64).reshape(-1, F),
        bank_mean=np.array([np.vstack(list(t.features)).mean(0) for t in tr],
                           np.float64).reshape(-1, F),
        bank_count=np.array([t._bx_pushes for t in tr], np.int32))


def run(tracker, frames, count, snap_at=()):
    import lap

    lap.STATS["calls"] = 0
    lap.STATS["degenerate"] = 0
    img = np.zeros((1080, 1920, 3), np.uint8)
    held = {}
    tracker.model.get_features = lambda *a, **k: held["embs"].copy()  # H2
    rows, snaps = [], {}
    for fno, dets, embs in frames:
        held["embs"] = np.asarray(embs, np.float64)
        scores = np.asarray(dets, np.float32)[:, 4]
        count["below_thresh_dets"] += int((~(scores > tracker.det_thresh)).sum())
        before, born = len(tracker.active_tracks), count["births"]
        out = np.asarray(tracker.update(dets, img, embs), dtype=np.float64).reshape(-1, 8)
        count["deaths"] += before + (count["births"] - born) - len(tracker.active_tracks)
        rows.append(np.concatenate([np.full((out.shape[0], 1), fno, np.float64), out], 1))
        if fno in snap_at:
            snaps[fno] = snapshot(tracker)
    return np.concatenate(rows, 0), dict(lap.STATS), snaps


def main():
    only = {}
    for a in sys.argv[1:]:
        name, _, seed = a.partition("@")
        only[name] = int(seed) if seed else None
    install_shim()
    use_restated_lapx_jv()
    import boxmot.motion.cmc  # noqa: F401  (so that the replacement below is not overwritten)

    install_h1()
    count = dict.fromkeys(COUNTERS, 0)
    import boxmot.trackers.hybridsort.hybridsort as mod

    mod.get_cmc_method = lambda name: IdentityCMC
    instrument(count)
    for name, skw, tkw, nf, need in CASES:
        if only and name not in only:
            continue
        probe = only.get(name)
        if probe is not None:
            skw = dict(skw, seed=probe)
        stop = name.startswith("stop")
        scene = StopScene(**skw) if stop else SyntheticScene(**skw)
        assert nf <= 120 and (stop or scene.emb_dtype == F64) and scene.n_obj <= 96
        snap_at = [nf // 4, nf // 2, 3 * nf // 4, nf]

        def capture(args):
            for k in count:
                count[k] = 0
            tracker = mod.HybridSort(reid_weights=None, device="cpu", half=False, **args)
            o, st, snaps = run(tracker, synth_frames(scene, nf), count, snap_at)
            state = {f"state_{k}": np.concatenate([snaps[f][k] for f in snap_at], 0)
                     for k in snaps[nf]}
            state["state_frames"] = np.array(snap_at, np.int32)
            state["state_off"] = np.concatenate(
                [[0], np.cumsum([snaps[f]["id"].shape[0] for f in snap_at])]).astype(np.int32)
            return o, st, state

        differs = ""
        if name in TWIN:  # (make_golden_deepocsort.py: TWIN)
            twin = capture(dict(tkw, asso_func=TWIN[name]))
        outs, stats, state = capture(tkw)
        if name in TWIN:
            differs = f" differs from {TWIN[name]}: {not same_capture((outs, state), (twin[0], twin[2]))}"
        print(f"{name}: rows={outs.shape[0]} lap={stats} {count}{differs}")
        if probe is not None:
            continue
        assert name not in TWIN or not same_capture((outs, state), (twin[0], twin[2])), \
            f"{name}: the run is the same under {TWIN[name]}: change the seed or the scene"
        for k in need:
            assert count[k] > 0, f"{name} never reached {k}: change the seed, jitter or p_det"
        assert stats["degenerate"] == 0, f"{name}: a LAP call ties: change the seed"
        if stop:  # (nearly) every object is found again by the OCR round in one frame
            assert count["ocr_rematches"] >= 72
        extra = {"scene_kind": "stop"} if stop else {}
        path = HERE / f"hybrid_{name}.npz"
        if path.exists():
            with np.load(path) as old:
                for k, v in dict(state, outputs=outs).items():
                    assert np.array_equal(old[k], v), f"{name}: {k} changed"
        np.savez_compressed(
            path, outputs=outs, n_frames=nf, kind="hybridsort",
            scene=repr(skw), tracker_args=repr(tkw), lap_calls=stats["calls"],
            lap_degenerate=stats["degenerate"], needs=repr(need), **count, **state, **extra)


if __name__ == "__main__":
    main()

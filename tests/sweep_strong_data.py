"""The small sweep case of tests/test_seqparams_ss_gpu.py, tests/test_sweep_strong_gpu.py and
tests/test_sweep_strong_host.py: the two scenes of tests/tune_data.py with the F = 20 embeddings
and the non-identity warps of tests/sweep_reid_data.py and the doubled detection of
tests/sweep_boost_data.py (40 and 33 frames, one frame without any detection), every detection
value rounded to float32 (what the shared feeder holds; StrongSort itself takes float64), and
seven StrongSort configs.

Sequence 1 begins with a crowd stretch: in ``CROWD_FRAMES`` its detections are replaced by three
large objects near the image's top-left corner (``CROWD_TLWH``).  detect_crowd_situations reads the
tracks' tlwh rows as corner boxes, so only boxes with x < w and y < h count at all (the scene's
own, 60 x 150 far from the corner, never do); read that way the first overlaps each of the other
two by about 0.4 of either box, so two of the three pairs pass the crowd test's 0.3 and crowd
mode is entered with the second frame.  The tracks born at the first frame after the stretch are
still born in crowd mode, on int(1.5 * max_age); then the scene's own tracks dilute the pairs,
crowd mode is left and the adapted values are restored.  The occlusion handler reads the boxes
the same way and raises where two of similar area overlap above its threshold, so the
occlusion-on configs run on ``occlusion_threshold`` 0.5 (``OCC_KW``), above the stretch's 0.4: the
whole scene runs with occlusion on, through crowd mode, without a raise (``scene(seq,
crowd=False)`` is the scene without the stretch).  ``crowd_detection`` shows in a result file
through config 5, the twin of config 3 (``nn_budget`` 2, doubled in crowd mode).

Sequence 0 holds, in ``PAIR_FRAMES``, two more objects 300 px wide and high with their top-left
corners near (10, 10) and (150, 150).  The occlusion handler reads tlwh rows as corner boxes too:
as such the second lies inside the first (overlap 1, above either threshold) at about a quarter of
its area, a size ratio outside [0.8, 1.2], so the handler takes the first for the occluder and
edits the second track (a ratio inside that band raises the reference's TypeError instead).

The configs are what ``run_sequences("strongsort", ..., tracker_kwargs=cfg)`` takes, with
``handle_occlusions`` added by ``configs(occ)``; ``born_confirmed`` is not a constructor argument
(the drop-in reads it from the environment) and is covered on the engine."""
import numpy as np

from tests import sweep_boost_data as BD
from tests import sweep_reid_data as RD
from tests import tune_data as TD

S, F = TD.S, RD.F
# vec_cap: the drop-in's default (a 40-frame track fills 32 vectors).  track_cap: 64 slots run
# out (listed tracks plus the lost buffer's 30); 256 is the next size tried, not a measured minimum
CAPS = dict(track_cap=256, det_cap=32, vec_cap=64)
N_FRAMES = TD.N_FRAMES
CROWD_SEQ, CROWD_FRAMES, CROWD_N = 1, range(1, 9), 3
OCC_KW = dict(occlusion_threshold=0.5)  # the occlusion-on configs' threshold
PAIR_SEQ, PAIR_FRAMES = 0, range(6, 31)  # the occluding pair

CONFIGS = [
    dict(),
    dict(min_conf=0.3, max_cos_dist=0.05),
    dict(max_iou_dist=0.3, conf_thresh_high=0.9, conf_thresh_low=0.5),
    dict(max_age=1, nn_budget=2, ema_alpha=0.1),
    dict(mc_lambda=0.2, id_preservation_weight=0.9),
    dict(max_age=1, nn_budget=2, ema_alpha=0.1, crowd_detection=False),  # config 3's twin
    dict(max_age=3, max_cos_dist=0.3, crowd_detection=False, conf_thresh_high=0.5, n_init=1000),
]
K = len(CONFIGS)
FIELDS = ("min_conf", "max_cos_dist", "max_iou_dist", "max_age", "n_init", "nn_budget",
          "mc_lambda", "ema_alpha", "conf_thresh_high", "conf_thresh_low",
          "id_preservation_weight", "crowd_detection")
# field -> the config that changes it
FIELD_CONFIG = dict(min_conf=1, max_cos_dist=1, n_init=6, max_iou_dist=2, conf_thresh_high=2,
                    conf_thresh_low=2, max_age=3, nn_budget=3, ema_alpha=3, mc_lambda=4,
                    id_preservation_weight=4, crowd_detection=5)


def configs(occ: bool, **extra) -> list:
    return [dict(c, handle_occlusions=occ, **CAPS, **(OCC_KW if occ else {}), **extra)
            for c in CONFIGS]


def defaults() -> dict:
    from boxmot_amd.engine import SsParams

    return {k: getattr(SsParams(), k) for k in FIELDS}


def resolved(cfg: dict) -> dict:
    """The SsParams fields (born_confirmed apart) the drop-in makes of cfg."""
    out = defaults()
    out.update({k: v for k, v in cfg.items() if k in FIELDS})
    return out


def params_of(cfg: dict, born_confirmed: bool = False):
    from boxmot_amd.engine import SsParams

    return SsParams(**resolved(cfg), born_confirmed=born_confirmed)


# the crowd stretch's boxes as tlwh: read as corner boxes, A overlaps B and C by 0.38 - 0.40 of
# either box (above the crowd test's 0.3, below OCC_KW's threshold) and B and C barely overlap
CROWD_TLWH = np.array([[10.0, 10.0, 400.0, 400.0], [200.0, 10.0, 700.0, 300.0],
                       [10.0, 200.0, 300.0, 700.0]])


def _crowd_rows(t: int):
    """The crowd stretch's detections and embeddings at frame t."""
    rng = np.random.default_rng([t, 0xC20D])
    b = CROWD_TLWH.copy()
    b[:, :2] += rng.normal(0.0, 0.5, (CROWD_N, 2))
    d = np.column_stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3],
                         np.full(CROWD_N, 0.9), np.zeros(CROWD_N)])
    base = np.random.default_rng(0xC20E).standard_normal((CROWD_N, F))
    e = base + RD.NOISE * rng.standard_normal((CROWD_N, F))
    return d, e / np.linalg.norm(e, axis=1, keepdims=True)


def _pair_rows(t: int):
    """The occluding pair's detections and embeddings at frame t."""
    rng = np.random.default_rng([t, 0x0CC1])
    tl = np.array([[10.0, 10.0], [150.0, 150.0]]) + rng.normal(0.0, 0.5, (2, 2))
    d = np.column_stack([tl, tl + 300.0, [0.92, 0.88], [0.0, 0.0]])
    base = np.random.default_rng(0x0CC2).standard_normal((2, F))
    e = base + RD.NOISE * rng.standard_normal((2, F))
    return d, e / np.linalg.norm(e, axis=1, keepdims=True)


def scene(seq: int, crowd: bool = True) -> list:
    """(dets [n, 6] float64 holding float32 values, embs [n, F] float64) per frame."""
    out = []
    for t, (d, e) in enumerate(BD.scene(seq), 1):
        if seq == PAIR_SEQ and t in PAIR_FRAMES and d.shape[0]:
            pd, pe = _pair_rows(t)
            d, e = np.vstack([d, pd]), np.vstack([e, pe])
        if crowd and seq == CROWD_SEQ and t in CROWD_FRAMES and d.shape[0]:
            cd, ce = _crowd_rows(t)
            d, e = cd, ce
        assert d.shape[0] <= CAPS["det_cap"]
        out.append((d.astype(np.float32).astype(np.float64), e))
    return out


packed_rows = RD.packed_rows
warps = RD.frame_warps        # [N_FRAMES[seq], 6] float64, none the identity


def crowd_fraction(tlwh: np.ndarray) -> float:
    """detect_crowd_situations' figure for tracks whose tlwh rows are read as xyxy: the fraction
    of pairs whose intersection exceeds 30 % of either box (crowd mode: > 0.3, >= 3 tracks)."""
    n, high = tlwh.shape[0], 0
    for i in range(n):
        for j in range(i + 1, n):
            a, b = tlwh[i], tlwh[j]
            w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
            h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
            if w * h > 0:
                ai, aj = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
                high += max(w * h / ai, w * h / aj) > 0.3
    return high / max(n * (n - 1) // 2, 1)


def oracle_rows(params: dict, seq: int, with_warps: bool = False, crowd: bool = True,
                born_confirmed: bool = False) -> np.ndarray:
    """The C oracle's rows [n, 11] (frame first) of sequence seq under ``params``; a frame
    without detections is not an update."""
    from oracle import pyoracle as po

    tr = po.OracleTracker("strongsort", **params, born_confirmed=born_confirmed)
    w = warps(seq)
    rows = [np.empty((0, 11))]
    for t, (d, e) in enumerate(scene(seq, crowd), 1):
        if d.shape[0]:
            o = tr.update(d, e, w[t - 1].reshape(2, 3) if with_warps else None)
            rows.append(np.column_stack([np.full(o.shape[0], float(t)), o]))
    return np.concatenate(rows)

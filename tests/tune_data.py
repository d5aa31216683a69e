"""The small sweep case of tests/test_tune_host.py and tests/test_tune_gpu.py: two sequences from
boxmot_amd.synth.SyntheticScene (10 objects, at most 12 detections per frame, about 40 frames),
shaped so that OCSort's parameters matter, and the three configs A, B, C.

Each scene is a SyntheticScene whose first two objects are put on a collision course (same height,
15 px per frame towards each other: they cross around frame 20, which is where ``asso_func`` and
``inertia`` decide), whose object 2 is not detected for ``GAP`` (``max_age`` 2 loses it, 30 keeps it
and re-updates it through the gap), and where every fourth detection's confidence is redrawn from
U(0.11, 0.55): below config A's det_thresh 0.6, on both sides of C's 0.4, and partly below B's 0.2,
where its BYTE round picks them up.
"""
import inspect

import numpy as np
import yaml

from boxmot_amd.synth import SyntheticScene

S, K, CAPS = 2, 3, dict(track_cap=32, det_cap=32)
N_FRAMES = (40, 33)     # the sequences differ in length
GAP = range(14, 19)     # frames in which object 2 is not detected
EMPTY = (1, 9)          # (sequence, frame): a frame without any detection
A = {}
B = dict(use_byte=True, min_hits=1, max_age=2, delta_t=1)
C = dict(asso_func="giou", det_thresh=0.4, inertia=0.3, asso_threshold=0.2)
CONFIGS = [A, B, C]


def resolved(cfg: dict) -> dict:
    """The OcSort parameters run_sequences makes of tracker_kwargs=cfg, without an engine: the
    YAML defaults when cfg is empty, else the drop-in constructor's defaults under cfg."""
    from boxmot_amd import OcSort, get_tracker_config

    if not cfg:
        with open(get_tracker_config("ocsort")) as f:
            return {k: v["default"] for k, v in yaml.safe_load(f).items()}
    sig = inspect.signature(OcSort.__init__).parameters
    out = {k: p.default for k, p in sig.items()
           if k not in ("self", "per_class", "track_cap", "det_cap")}
    out.update({k: v for k, v in cfg.items() if k not in CAPS})
    return out


def params_of(cfg: dict):
    from boxmot_amd.engine import OcsortParams

    return OcsortParams(**resolved(cfg))


def _scene(seq: int) -> SyntheticScene:
    sc = SyntheticScene(n_obj=10, seed=40 + seq, layout="crowded", p_det=0.9)
    sc.size[:2] = (60.0, 150.0)
    sc.c0[0], sc.vel[0] = (400.0, 500.0 + 200.0 * seq), (15.0, 0.0)
    sc.c0[1], sc.vel[1] = (1000.0, 506.0 + 200.0 * seq), (-15.0, 0.0)
    return sc


def scene_frames(seq: int) -> list:
    """dets [n, 6] float64 of frames 1..N_FRAMES[seq] of sequence seq."""
    sc = _scene(seq)
    frames = []
    for t in range(1, N_FRAMES[seq] + 1):
        d, _, ids = sc.frame(t)
        if t in GAP:
            d = d[ids != 2]
        rng = np.random.default_rng([seq, t, 0x70E])
        low = np.arange(d.shape[0]) % 4 == (t % 4)
        d[low, 4] = rng.uniform(0.11, 0.55, int(low.sum()))
        if (seq, t) == EMPTY:
            d = d[:0]
        assert d.shape[0] <= 12
        frames.append(d)
    return frames


def packed_rows(frames: list) -> np.ndarray:
    """[rows, 7] (frame, x1, y1, x2, y2, conf, cls) for motio.pack_arrays."""
    return np.concatenate([np.column_stack([np.full(d.shape[0], t + 1.0), d])
                           for t, d in enumerate(frames)])


def synthetic_gt(seq: int) -> np.ndarray:
    """gt rows [n, 9] (frame, id, x, y, w, h, 1, 1, 1) of the scene's objects, every frame, from
    the same motion model without the jitter and the misses."""
    sc = _scene(seq)
    rows = []
    for t in range(1, N_FRAMES[seq] + 1):
        c = sc.c0 + sc.vel * float(t)
        tl = c - sc.size * 0.5
        for k in range(sc.n_obj):
            rows.append([t, k + 1, tl[k, 0], tl[k, 1], sc.size[k, 0], sc.size[k, 1], 1, 1, 1])
    return np.asarray(rows, np.float64)

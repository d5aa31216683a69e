"""The small sweep case of tests/test_seqparams_reid_gpu.py, tests/test_sweep_reid_gpu.py and
tests/test_sweep_reid_host.py: the two scenes of tests/tune_data.py (40 and 33 frames, at most 12
detections, one frame without any) with an embedding per detection, and three configs
per appearance tracker.

Embeddings (F = 20, float64): every object identity has a seeded unit row; a detection's row is its
object's plus noise, renormalised.  The two objects on the collision course (0 and 1) get
near-equal rows, so around the crossing the appearance term cannot tell them apart by itself and
its weight against IoU and direction decides the pairing.

Capacities: det_cap 32 as in tests/tune_data.py, track_cap 128.  DeepOCSort's third config
(``asso_func="giou"`` under the unscaled ``iou_threshold`` 0.3) rejects the pairs of three fast
objects of the second scene frame after frame, so each of them is born again every frame and the
sequence holds 67 tracks at its peak (measured on a plain engine): tune_data's 32 slots latch
BX_ERR_TRACK_OVERFLOW there.  It also puts that sequence past the 64 lanes of its wave.

The configs are what ``run_sequences(tracker, ..., tracker_kwargs=cfg)`` takes.  The CPU oracle
under oracle/ restates neither DeepOCSort nor HybridSort, so that the configs tell themselves apart
is asserted where they run, on the engines (``test_table_matches_separate_engines``)."""
import inspect

import numpy as np

from tests import tune_data as TD

S, K, CAPS, F = TD.S, 3, dict(track_cap=128, det_cap=32), 20
N_FRAMES = TD.N_FRAMES
NOISE = 0.05

DEEPOC = [
    {},
    dict(w_association_emb=0.0, aw_off=True, max_age=2, delta_t=1),
    dict(alpha_fixed_emb=0.5, aw_param=1.0, det_thresh=0.4, asso_func="giou"),
]
HYBRID = [
    {},
    dict(TCM_first_step_weight=1.0, longterm_reid_weight=0.5, max_age=2, delta_t=1),
    dict(longterm_reid_weight=1.5, det_thresh=0.4, asso_func="giou", inertia=0.05, min_hits=1),
]
CONFIGS = {"deepocsort": DEEPOC, "hybridsort": HYBRID}


def frames_with_ids(seq: int) -> list:
    """(dets [n, 6] float64, object ids [n]) of frames 1..N_FRAMES[seq]: TD.scene_frames with the
    identities kept."""
    sc = TD._scene(seq)
    frames = []
    for t in range(1, N_FRAMES[seq] + 1):
        d, _, ids = sc.frame(t)
        if t in TD.GAP:
            d, ids = d[ids != 2], ids[ids != 2]
        rng = np.random.default_rng([seq, t, 0x70E])
        low = np.arange(d.shape[0]) % 4 == (t % 4)
        d[low, 4] = rng.uniform(0.11, 0.55, int(low.sum()))
        if (seq, t) == TD.EMPTY:
            d, ids = d[:0], ids[:0]
        frames.append((d, np.asarray(ids, np.int64)))
    return frames


def identity_rows(seq: int, n_obj: int = 10) -> np.ndarray:
    """[n_obj, F] unit rows, object 1's within NOISE of object 0's."""
    rng = np.random.default_rng([seq, 0xE3B])
    base = rng.standard_normal((n_obj, F))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    base[1] = base[0] + NOISE * rng.standard_normal(F)
    base[1] /= np.linalg.norm(base[1])
    return base


def scene(seq: int) -> list:
    """(dets [n, 6] float64, embs [n, F] float64) per frame of sequence seq."""
    base = identity_rows(seq)
    out = []
    for t, (d, ids) in enumerate(frames_with_ids(seq), 1):
        rng = np.random.default_rng([seq, t, 0xE3B])
        e = base[ids] + NOISE * rng.standard_normal((d.shape[0], F))
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        out.append((d, e))
    return out


def packed_rows(frames: list):
    """([rows, 7] (frame, x1, y1, x2, y2, conf, cls), [rows, F]) for motio.pack_arrays."""
    return TD.packed_rows([d for d, _ in frames]), np.concatenate([e for _, e in frames])


def frame_warps(seq: int) -> np.ndarray:
    """[N_FRAMES[seq], 6] float64 warps, none the identity: a small rotation, scale and shift that
    change from frame to frame, exactly representable in float32 (what the flow rounds to)."""
    t = np.arange(N_FRAMES[seq], dtype=np.float64)
    a = 0.002 * np.sin(0.7 * t + seq)
    w = np.column_stack([1.0 + 0.001 * np.cos(t), -a, 1.5 * np.sin(0.3 * t) + 0.25 * (seq + 1),
                         a, 1.0 - 0.001 * np.cos(t), -1.0 * np.cos(0.2 * t) - 0.5])
    return w.astype(np.float32).astype(np.float64)


def resolved(tracker: str, cfg: dict) -> dict:
    """The constructor parameters run_sequences makes of tracker_kwargs=cfg, without an engine:
    the drop-in constructor's defaults under cfg (HybridSort's det_thresh, which has no default,
    is the engine parameters' 0.3, as in motio._batched_engine)."""
    from boxmot_amd.engine import DeepOcsortParams, HybridsortParams
    from boxmot_amd.trackers.deepocsort import DeepOcSort
    from boxmot_amd.trackers.hybridsort import HybridSort

    cls, par = (DeepOcSort, DeepOcsortParams) if tracker == "deepocsort" else \
        (HybridSort, HybridsortParams)
    names = [f for f in par.__dataclass_fields__ if f not in ("frame_w", "frame_h")]
    sig = inspect.signature(cls.__init__).parameters
    out = {k: sig[k].default for k in names}
    if tracker == "hybridsort":
        out["det_thresh"] = HybridsortParams().det_thresh
    out.update({k: v for k, v in cfg.items() if k in names})
    return out


def params_of(tracker: str, cfg: dict):
    from boxmot_amd.engine import DeepOcsortParams, HybridsortParams

    par = DeepOcsortParams if tracker == "deepocsort" else HybridsortParams
    return par(**resolved(tracker, cfg))

"""The small sweep case of tests/test_seqparams_bot_gpu.py, tests/test_sweep_bot_gpu.py and
tests/test_sweep_bot_host.py: the two scenes of tests/tune_data.py with the embeddings of
tests/sweep_reid_data.py (40 and 33 frames, at most 12 detections, one frame without any, objects 0
and 1 on a collision course with near-equal embeddings), and three configs per tracker.

``scene(seq, F)`` is ``sweep_reid_data.scene`` with the identity rows and the noise drawn at width
F; at F = 20 it is that scene itself.  The noise per element is scaled by sqrt(20 / F), so that a
detection's row lies as far from its identity's as it does at F = 20: unscaled, the noise of a
512-wide row is longer than the row, every embedding distance is above every config's
``appearance_thresh``, and the appearance term would decide nothing.

The configs are what ``run_sequences(tracker, ..., tracker_kwargs=cfg)`` takes; ``configs(kind)``
adds the capacities (track_cap 128, det_cap 32).  They were picked on the CPU oracle so that the
K * S result sets are pairwise different (tests/test_sweep_bot_host.py asserts it): ByteTrack's B
raises the detection split and drops lost tracks after 2 frames, its C lowers the split into the
redrawn confidences U(0.11, 0.55) and derives max_time_lost from frame_rate; BoT-SORT's B gates on
almost any overlap but accepts only near-equal embeddings and drops lost tracks after 2 frames, its
C lowers the thresholds, fuses the score into the first association and tightens the match."""
import inspect

import numpy as np
import yaml

from tests import sweep_reid_data as RD
from tests import tune_data as TD

S, K, CAPS = TD.S, 3, dict(track_cap=128, det_cap=32)
N_FRAMES = TD.N_FRAMES
KINDS = ("bytetrack", "botsort")

BYTE = [
    {},
    dict(track_thresh=0.6, match_thresh=0.6, track_buffer=2),
    dict(min_conf=0.3, track_thresh=0.35, frame_rate=10),
]
BOT = [
    {},
    dict(appearance_thresh=0.05, proximity_thresh=0.9, track_buffer=2),
    dict(track_high_thresh=0.35, new_track_thresh=0.4, fuse_first_associate=True,
         match_thresh=0.6),
]
CONFIGS = {"bytetrack": BYTE, "botsort": BOT}


def configs(kind: str, **extra) -> list:
    return [dict(c, **CAPS, **extra) for c in CONFIGS[kind]]


def scene(seq: int, F: int = RD.F) -> list:
    """(dets [n, 6] float64, embs [n, F] float64) per frame of sequence seq."""
    if F == RD.F:
        return RD.scene(seq)
    noise = RD.NOISE * np.sqrt(RD.F / F)
    rng = np.random.default_rng([seq, 0xE3B])
    base = rng.standard_normal((10, F))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    base[1] = base[0] + noise * rng.standard_normal(F)
    base[1] /= np.linalg.norm(base[1])
    out = []
    for t, (d, ids) in enumerate(RD.frames_with_ids(seq), 1):
        rng = np.random.default_rng([seq, t, 0xE3B])
        e = base[ids] + noise * rng.standard_normal((d.shape[0], F))
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        out.append((d, e))
    return out


def resolved(kind: str, cfg: dict) -> dict:
    """The EngineParams fields run_sequences makes of tracker_kwargs=cfg, without an engine: the
    YAML defaults when cfg is empty, else the drop-in constructor's defaults under cfg."""
    from boxmot_amd import get_tracker_config
    from boxmot_amd.engine import EngineParams
    from boxmot_amd.trackers import BotSort, ByteTrack

    sig = inspect.signature((ByteTrack if kind == "bytetrack" else BotSort).__init__).parameters
    names = [f for f in EngineParams.__dataclass_fields__ if f in sig]
    out = {k: sig[k].default for k in names}
    if not cfg:
        with open(get_tracker_config(kind)) as f:
            out.update({k: v["default"] for k, v in yaml.safe_load(f).items() if k in names})
    out.update({k: v for k, v in cfg.items() if k in names})
    return out


def params_of(kind: str, cfg: dict):
    """The EngineParams an engine of ``kind`` runs on under ``cfg`` (the fields the tracker does
    not have stay at EngineParams' defaults, as the drop-ins leave them)."""
    from boxmot_amd.engine import EngineParams

    return EngineParams(**resolved(kind, cfg))

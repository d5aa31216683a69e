"""The small sweep case of tests/test_seqparams_boost_gpu.py, tests/test_sweep_boost_gpu.py and
tests/test_sweep_boost_host.py: the two scenes of tests/tune_data.py with the F = 20 embeddings
and the non-identity warps of tests/sweep_reid_data.py (40 and 33 frames, at most 12 detections,
one frame without any, objects 0 and 1 on a collision course with near-equal embeddings), and six
BoostTrack configs.

The configs are what ``run_sequences("boosttrack", ..., tracker_kwargs=cfg)`` takes.  A non-empty
``tracker_kwargs`` goes through the drop-in's constructor, whose flag defaults are the plain
BoostTrack's, so every config spells out what it switches on: ``PP`` is the YAML's BoostTrack++
(``engine.BoostParams()``, "the default" below), and ``configs(reid)`` adds ``with_reid`` and the
capacities (track_cap 128, det_cap 32).

They were picked on the CPU oracle (tests/test_sweep_boost_host.py asserts both properties):
the K * S result sets are pairwise different, and each of the 17 per-sequence fields is changed by
some config whose oracle result differs from the same config with that one field back at the
default (``FIELD_CONFIG`` names the config per field), so a field that is not wired into the
kernel's table cannot pass:
  0  the default, BoostTrack++
  1  the plain BoostTrack (use_rich_s, use_sb, use_vt off: the only build of the DLO boost that
     reads dlo_boost_coef) with another dlo_boost_coef
  2  BoostTrack++ without the DLO and DUO boosts
  3  s_sim_corr on and other lambda weights
  4  short track lifetime and other thresholds (max_age, min_hits, det_thresh, iou_threshold)
  5  use_ecc off and output filters (min_box_area, aspect_ratio_thresh) that cut into the scene's
     boxes
``use_ecc`` matters under the warps of ``warps(seq)`` only, which the oracle runs and the GPU
warp cases apply."""
import numpy as np

from tests import sweep_reid_data as RD
from tests import tune_data as TD

S, F, CAPS = TD.S, RD.F, dict(track_cap=128, det_cap=32)
N_FRAMES = TD.N_FRAMES

PP = dict(use_rich_s=True, use_sb=True, use_vt=True)  # BoostTrack++ over the constructor's flags
CONFIGS = [
    dict(PP),
    dict(dlo_boost_coef=1.3),
    dict(PP, use_dlo_boost=False, use_duo_boost=False),
    dict(PP, s_sim_corr=True, lambda_iou=2.0, lambda_mhd=1.0, lambda_shape=2.0),
    dict(PP, max_age=2, min_hits=1, det_thresh=0.4, iou_threshold=0.6),
    dict(PP, use_ecc=False, min_box_area=9500, aspect_ratio_thresh=0.45),
]
K = len(CONFIGS)
FIELDS = ("max_age", "min_hits", "det_thresh", "iou_threshold", "min_box_area",
          "aspect_ratio_thresh", "lambda_iou", "lambda_mhd", "lambda_shape", "dlo_boost_coef",
          "use_ecc", "use_dlo_boost", "use_duo_boost", "s_sim_corr", "use_rich_s", "use_sb",
          "use_vt")
# field -> the config that exercises it (the flags of the variants: the plain BoostTrack, which
# has them off where the default has them on)
FIELD_CONFIG = dict(
    max_age=4, min_hits=4, det_thresh=4, iou_threshold=4, min_box_area=5, aspect_ratio_thresh=5,
    lambda_iou=3, lambda_mhd=3, lambda_shape=3, dlo_boost_coef=1, use_ecc=5, use_dlo_boost=2,
    use_duo_boost=2, s_sim_corr=3, use_rich_s=1, use_sb=1, use_vt=1)


def configs(reid: bool = True, **extra) -> list:
    return [dict(c, with_reid=reid, **CAPS, **extra) for c in CONFIGS]


def defaults() -> dict:
    """The default of every field: engine.BoostParams(), which is the YAML's."""
    from boxmot_amd.engine import BoostParams

    return {k: getattr(BoostParams(), k) for k in FIELDS}


def resolved(cfg: dict) -> dict:
    """The BoostParams fields run_sequences makes of tracker_kwargs=cfg, without an engine: the
    YAML defaults when cfg is empty, else the drop-in constructor's defaults under cfg."""
    import inspect

    import yaml

    from boxmot_amd import get_tracker_config
    from boxmot_amd.engine import BoostParams
    from boxmot_amd.trackers import BoostTrack

    names = list(BoostParams.__dataclass_fields__)
    if not cfg:
        with open(get_tracker_config("boosttrack")) as f:
            return {k: v["default"] for k, v in yaml.safe_load(f).items() if k in names}
    sig = inspect.signature(BoostTrack.__init__).parameters
    out = {k: sig[k].default for k in names}
    out.update({k: v for k, v in cfg.items() if k in names})
    return out


def params_of(cfg: dict):
    from boxmot_amd.engine import BoostParams

    return BoostParams(**resolved(cfg))


DUP = 3                       # the object detected twice
DUP_FRAMES = range(4, 31)


def scene(seq: int) -> list:
    """(dets [n, 6] float64, embs [n, F] float64) per frame of sequence seq: RD.scene with a
    second detection of object DUP appended in DUP_FRAMES, wider, lower and shifted, its
    confidence alternating above and below the first one's, its embedding the first one's plus
    noise.  Two detections then compete for one track (and the loser's newborn track for the next
    frame's detections), which is where the cost's weights decide: on the scenes without it
    ``lambda_iou`` and ``lambda_shape`` change no pairing (tried on the oracle from 0 to 50)."""
    out = []
    for t, ((d, e), (_, ids)) in enumerate(zip(RD.scene(seq), RD.frames_with_ids(seq)), 1):
        k = np.flatnonzero(ids == DUP)
        if t in DUP_FRAMES and k.size:
            rng = np.random.default_rng([seq, t, 0xD0B])
            x1, y1, x2, y2 = d[k[0], :4]
            sx, sy = rng.normal(0.0, 3.0, 2)
            cx, cy = (x1 + x2) / 2 + sx, (y1 + y2) / 2 + sy
            w, h = (x2 - x1) * rng.uniform(0.9, 1.2), (y2 - y1) * rng.uniform(0.85, 1.1)
            row = d[k[0]].copy()
            row[:4] = (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)
            row[4] = 0.99 if t % 2 else 0.61
            v = e[k[0]] + RD.NOISE * rng.standard_normal(F)
            d, e = np.vstack([d, row]), np.vstack([e, v / np.linalg.norm(v)])
        assert d.shape[0] <= 13
        out.append((d, e))
    return out


def packed_rows(frames: list):
    """([rows, 7] (frame, x1, y1, x2, y2, conf, cls), [rows, F]) for motio.pack_arrays."""
    return RD.packed_rows(frames)


warps = RD.frame_warps        # [N_FRAMES[seq], 6] float64, none the identity


def oracle_rows(params: dict, seq: int, with_warps: bool = True) -> np.ndarray:
    """The C oracle's rows [n, 9] (frame first) of sequence seq under the resolved parameters
    ``params``, frame by frame; a frame without detections is not an update."""
    from oracle import pyoracle as po

    tr = po.OracleTracker("boosttrack", **params)
    w = warps(seq)
    rows = [np.empty((0, 9))]
    for t, (d, e) in enumerate(scene(seq), 1):
        if d.shape[0]:
            o = tr.update(d, e if params["with_reid"] else None,
                          w[t - 1].reshape(2, 3) if with_warps else None)
            rows.append(np.column_stack([np.full(o.shape[0], float(t)), o]))
    return np.concatenate(rows)

"""Scenes the fixture generators (tests/golden/make_golden_*.py) and the GPU tests both build from
their arguments, so that a fixture stores the arguments and never the frames.

``StopScene``: objects that move a full box width per frame and then all stop in the same frame.
(They reach that speed over two frames, 0.4 and 0.8 of a width: from a standing start a box a full
width away overlaps neither the prediction nor the last observation and every frame would only give
birth to new tracks.)  A track's prediction then lands a box width past its object, so the first
association matches nothing, while every detection overlaps its own track's last observation: the
OCR round takes all detections x all tracks in one problem. With 76 objects that is 76 * 76 = 5776
costs, more than 5120 doubles, the most the frame kernels ever keep of a cost matrix in the LDS
whatever the capacities (ocs_lds_budget: 40 KiB less the fixed part, in doubles), so the OCR round's
matrix lies in global memory. SyntheticScene never gets there: its crowded scenes send the first
association to global memory, not the second.
"""
from __future__ import annotations

import ast
import math
from dataclasses import dataclass

import numpy as np

LDS_COST_MAX = 5120  # doubles: 40 KiB / 8, the upper bound of cost_lds
# DeepOcSort captures older than the rule that a tied LAP call refuses a case: resolved by the
# restated lapjv, they pin less (the generator keeps them, the GPU test names them in their ids)
DEEPOC_TIED = frozenset({"crowd40_f64", "crowd40_awoff", "crowd40_emboff", "crowd32_warp",
                         "crowd96_f32"})


@dataclass
class StopScene:
    n_obj: int = 76
    seed: int = 0
    emb_dim: int = 0
    move_frames: int = 6  # frames 2..move_frames move; every later frame repeats the last place
    jitter: float = 0.25  # uniform +-jitter px on every corner: IoUs are generic floats
    conf_lo: float = 0.65
    conf_hi: float = 1.0
    emb_noise: float = 0.1
    # the embedding noise of the frames after move_frames (None: emb_noise).  HybridSort keeps a
    # low-IoU pair whose appearance distance is under 0.4 (its correction rule), so with clean
    # embeddings its OCR round is never called, and with noisy ones from the start the objects
    # are lost while they move: clean until the stop, noisy after it
    emb_noise_stopped: float = None
    cols: int = 19  # a 19 x 4 grid of 100 x 250 px cells inside 1920 x 1080

    def __post_init__(self):
        rng = np.random.default_rng([self.seed, 0x570B])
        n = self.n_obj
        idx = np.arange(n)
        col, row = idx % self.cols, idx // self.cols
        w = rng.uniform(10.0, 13.0, n)
        h = w * rng.uniform(2.0, 3.0, n)
        # even rows move right, odd rows left; an object stays inside its own 100 px cell
        # (at most 6 * 13 + 13 px), so boxes of different objects never overlap
        self.dirn = np.where(row % 2 == 0, 1.0, -1.0)
        travel = self.moved(self.move_frames) * w
        x0 = 100.0 * col + 4.0 + w / 2 + np.where(self.dirn > 0, 0.0, travel)
        assert n <= self.cols * 4 and (travel + w + 8.0 < 100.0).all()
        self.c0 = np.stack([x0, 125.0 + 250.0 * row], 1)
        self.size = np.stack([w, h], 1)
        if self.emb_dim:
            base = rng.standard_normal((n, self.emb_dim))
            self.base_emb = base / np.linalg.norm(base, axis=1, keepdims=True)
        else:
            self.base_emb = None

    def moved(self, t: int) -> float:
        """Box widths travelled by frame t: steps of 0.4, 0.8, 1, 1, ... until move_frames."""
        k = min(int(t), self.move_frames) - 1
        return sum((0.4, 0.8)[:k]) + max(k - 2, 0)

    def frame(self, t: int):
        """SyntheticScene.frame's contract: ``(dets[N,6] float64, embs[N,F] float64 or None,
        ids[N])``; every object is detected, in a seeded random order."""
        rng = np.random.default_rng([self.seed, int(t)])
        ids = rng.permutation(self.n_obj)
        steps = self.moved(t)
        c = self.c0[ids].copy()
        c[:, 0] += self.dirn[ids] * self.size[ids, 0] * steps
        half = self.size[ids] * 0.5
        box = np.concatenate([c - half, c + half], 1) + rng.uniform(-self.jitter, self.jitter,
                                                                    (ids.size, 4))
        dets = np.zeros((ids.size, 6), np.float64)
        dets[:, :4] = box
        dets[:, 4] = rng.uniform(self.conf_lo, self.conf_hi, ids.size)
        embs = None
        if self.base_emb is not None:
            noise = self.emb_noise
            if int(t) > self.move_frames and self.emb_noise_stopped is not None:
                noise = self.emb_noise_stopped
            e = self.base_emb[ids] + noise * rng.standard_normal(
                (ids.size, self.emb_dim)) / math.sqrt(self.emb_dim)
            embs = e / np.linalg.norm(e, axis=1, keepdims=True)
        return dets, embs, ids


def scene_of(fx):
    """The scene of a fixture: ``scene`` holds the constructor arguments as ``repr``;
    ``scene_kind`` (absent: SyntheticScene) names the class."""
    from boxmot_amd.synth import SyntheticScene

    kw = ast.literal_eval(str(fx["scene"]))
    kind = str(fx["scene_kind"]) if "scene_kind" in fx.files else "synthetic"
    return {"synthetic": SyntheticScene, "stop": StopScene}[kind](**kw)

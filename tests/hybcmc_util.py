"""Helpers of the HybridSort camera-motion tests: a cmc that replays a warp table, and
KalmanBoxTracker.camera_update (hybridsort.py:237-249) restated in numpy from its formula, one
rounding per operation, with the 2x3 product's row sum in the order the fixtures pin:
fma(m0, x, m1 * y) + m2."""
from fractions import Fraction

import numpy as np


class ReplayCMC:
    """``tracker.cmc``: frame k's warp (row k of ``warps`` [n, 2, 3]) at its k-th call."""

    def __init__(self, warps):
        self.warps, self.calls = np.asarray(warps, np.float64).reshape(-1, 2, 3), 0

    def apply(self, img, dets=None):
        self.calls += 1
        return self.warps[self.calls - 1].astype(np.float32)


def fma(a, b, c) -> float:
    """a * b + c rounded once (finite arguments)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def camera_update(x, warp):
    """x [n, 9] -> (x after camera_update under the 2x3 ``warp``, the number of rows left as they
    were for a score of exactly 0)."""
    m = np.asarray(warp, np.float64).reshape(2, 3)
    out, skipped = np.array(x, np.float64), 0
    for k, s in enumerate(out):
        if s[3] == 0.0:
            skipped += 1
            continue
        w = np.sqrt(s[2] * s[4])
        h = s[2] / w
        x1, y1, x2, y2 = s[0] - w / 2.0, s[1] - h / 2.0, s[0] + w / 2.0, s[1] + h / 2.0
        a1 = fma(m[0, 0], x1, m[0, 1] * y1) + m[0, 2]
        b1 = fma(m[1, 0], x1, m[1, 1] * y1) + m[1, 2]
        a2 = fma(m[0, 0], x2, m[0, 1] * y2) + m[0, 2]
        b2 = fma(m[1, 0], x2, m[1, 1] * y2) + m[1, 2]
        bw, bh = a2 - a1, b2 - b1
        out[k, 0], out[k, 1] = a1 + bw / 2.0, b1 + bh / 2.0
        out[k, 2], out[k, 4] = bw * bh, bw / (bh + 1e-6)
    return out, skipped

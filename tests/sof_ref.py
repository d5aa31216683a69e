"""A float64 numpy restatement of the sparse-optical-flow contract (DESIGN.md 2.17,
include/bxsof.h): the oracle of tests/test_sof_host.py and tests/test_sof_gpu.py.

Written the textbook way: whole derivative planes, explicit windows cut out of them, ``np.linalg``
for the 2x2 Lucas-Kanade system and for the final least squares, a plain sort for the keypoint
selection.  Window sums are ``np.sum`` (not the device's lane order), so positions and warps agree
with the device to reduction-order level, while everything integer (pyramid, structure tensor)
and every per-pixel float64 formula (lambda, the hypotheses' residuals) agrees bit for bit.
OpenCV is not involved anywhere.
"""
from __future__ import annotations

import numpy as np

from tests import ecc_ref as E

OK, FIRST_FRAME, TOO_FEW, NO_MODEL, NO_KEYPOINTS = 0, 1, 2, 3, 4
HYPOTHESES = 256
EYE = np.array([[1.0, 0, 0], [0, 1.0, 0]])


# ------------------------------------------------------------------------------------ pyramid
def prep(img: np.ndarray, scale) -> np.ndarray:
    """The working image (int64 [h, w]): ECC's grey and resize rule."""
    g = E.grey(img)
    if scale is not None and scale < 1:
        g = E.resize(g, float(scale))
    return g


def pad101(a: np.ndarray, r: int) -> np.ndarray:
    return np.pad(a, r, mode="reflect")


def pyr_down(g: np.ndarray) -> np.ndarray:
    k = np.array([1, 4, 6, 4, 1], np.int64)
    p = pad101(g.astype(np.int64), 2)
    h, w = g.shape
    rows = sum(k[j] * p[:, j: j + w] for j in range(5))        # horizontal pass, every column
    full = sum(k[i] * rows[i: i + h, :] for i in range(5))     # vertical pass, every row
    return (full[::2, ::2] + 128) >> 8


def pyramid(g: np.ndarray, win: int, max_level: int):
    levels = [g.astype(np.int64)]
    while len(levels) <= max_level:
        h, w = levels[-1].shape
        if not ((h + 1) // 2 > win and (w + 1) // 2 > win):
            break
        levels.append(pyr_down(levels[-1]))
    return levels


# ---------------------------------------------------------------------------------- keypoints
def lam_plane(g: np.ndarray) -> np.ndarray:
    """Shi-Tomasi minimum eigenvalue of the 3x3 structure tensor (float64 [h, w])."""
    p = pad101(g.astype(np.int64), 1)
    h, w = g.shape

    def at(dy, dx):
        return p[1 + dy: 1 + dy + h, 1 + dx: 1 + dx + w]

    Dx = (at(-1, 1) - at(-1, -1)) + 2 * (at(0, 1) - at(0, -1)) + (at(1, 1) - at(1, -1))
    Dy = (at(1, -1) - at(-1, -1)) + 2 * (at(1, 0) - at(-1, 0)) + (at(1, 1) - at(-1, 1))

    def box(q):  # the derivative products' plane is what is reflected
        pq = pad101(q, 1)
        return sum(pq[i: i + h, j: j + w] for i in range(3) for j in range(3))

    a, b, c = (box(q).astype(np.float64) for q in (Dx * Dx, Dx * Dy, Dy * Dy))
    return 0.5 * (a + c) - np.sqrt(0.25 * ((a - c) * (a - c)) + b * b)


def candidates(lam: np.ndarray, quality: float) -> np.ndarray:
    """Boolean plane of the candidate pixels."""
    h, w = lam.shape
    ok = np.zeros((h, w), bool)
    if h < 3 or w < 3:
        return ok
    lmax = max(float(lam.max()), 0.0)
    c = lam[1:-1, 1:-1]
    m = (c > 0) & (c >= quality * lmax)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                m &= c >= lam[1 + dy: h - 1 + dy, 1 + dx: w - 1 + dx]
    ok[1:-1, 1:-1] = m
    return ok


def keypoints(g: np.ndarray, max_corners: int, quality: float) -> np.ndarray:
    """float64 [n, 2] (x, y): lambda descending, then pixel index ascending."""
    lam = lam_plane(g)
    idx = np.flatnonzero(candidates(lam, quality).ravel())
    order = sorted(idx.tolist(), key=lambda i: (-lam.ravel()[i], i))[:max_corners]
    w = g.shape[1]
    return np.array([[i % w, i // w] for i in order], np.float64).reshape(-1, 2)


# ----------------------------------------------------------------------------------- tracking
def scharr(g: np.ndarray):
    p = pad101(g.astype(np.int64), 1)
    h, w = g.shape

    def at(dy, dx):
        return p[1 + dy: 1 + dy + h, 1 + dx: 1 + dx + w]

    Ix = 3 * (at(-1, 1) - at(-1, -1)) + 10 * (at(0, 1) - at(0, -1)) + 3 * (at(1, 1) - at(1, -1))
    Iy = 3 * (at(1, -1) - at(-1, -1)) + 10 * (at(1, 0) - at(-1, 0)) + 3 * (at(1, 1) - at(-1, 1))
    return Ix, Iy


def window(plane: np.ndarray, tx: float, ty: float, win: int):
    """The win x win bilinear samples of the window anchored at (tx, ty), or None when it is not
    inside the plane."""
    h, w = plane.shape
    fx, fy = np.floor(tx), np.floor(ty)
    if not (fx >= 0 and fx + win <= w - 1 and fy >= 0 and fy + win <= h - 1):
        return None
    ax, ay = tx - fx, ty - fy
    x0, y0 = int(fx), int(fy)
    v = plane[y0: y0 + win + 1, x0: x0 + win + 1].astype(np.float64)
    w00, w01, w10, w11 = (1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay
    return ((w00 * v[:-1, :-1] + w01 * v[:-1, 1:]) + w10 * v[1:, :-1]) + w11 * v[1:, 1:]


def min_eig2(gxx, gxy, gyy):
    return 0.5 * (gxx + gyy) - np.sqrt(0.25 * ((gxx - gyy) * (gxx - gyy)) + gxy * gxy)


def track_point(prev_levels, cur_levels, derivs, p, win: int, max_iter: int, eps: float):
    """(q [2], tracked, iterations summed over the levels) of one keypoint p."""
    half = float((win - 1) // 2)
    nl = len(prev_levels)
    q = np.zeros(2)
    iters, lost = 0, False
    for l in range(nl - 1, -1, -1):
        pl = p * (1.0 / (1 << l))
        q = pl.copy() if l == nl - 1 else 2.0 * q
        Ix, Iy = derivs[l]
        fail = False
        I = window(prev_levels[l], pl[0] - half, pl[1] - half, win)
        if I is None:
            fail = True
        else:
            Dx = window(Ix, pl[0] - half, pl[1] - half, win)
            Dy = window(Iy, pl[0] - half, pl[1] - half, win)
            G = np.array([[np.sum(Dx * Dx), np.sum(Dx * Dy)], [np.sum(Dx * Dy), np.sum(Dy * Dy)]])
            det = G[0, 0] * G[1, 1] - G[0, 1] * G[0, 1]
            if min_eig2(G[0, 0], G[0, 1], G[1, 1]) / (1048576.0 * win * win) < 1e-4 or not det > 0:
                fail = True
        if not fail:
            pd = np.zeros(2)
            for j in range(max_iter):
                J = window(cur_levels[l], q[0] - half, q[1] - half, win)
                if J is None:
                    fail = True
                    break
                df = 32.0 * (J - I)  # the Scharr kernel sums to 32 per unit of slope
                b = np.array([np.sum(df * Dx), np.sum(df * Dy)])
                delta = np.linalg.solve(G, -b)
                q = q + delta
                iters += 1
                if delta @ delta <= eps * eps:
                    break
                if j > 0 and abs(delta[0] + pd[0]) < 0.01 and abs(delta[1] + pd[1]) < 0.01:
                    q = q - 0.5 * delta
                    break
                pd = delta
        if fail and l == 0:
            lost = True
    h, w = prev_levels[0].shape
    if not lost and not (0 <= q[0] <= w - 1 and 0 <= q[1] <= h - 1):
        lost = True
    return q, not lost, iters


# ---------------------------------------------------------------------------------------- fit
def mix(x: int) -> int:
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def hypothesis(P, Q, k: int):
    """(a, b, tx, ty) of hypothesis k, or None when it is skipped."""
    m = len(P)
    i, j = mix(2 * k) % m, mix(2 * k + 1) % m
    d, e = P[j] - P[i], Q[j] - Q[i]
    if d[0] == 0 and d[1] == 0:
        return None
    n2 = d[0] * d[0] + d[1] * d[1]
    with np.errstate(all="ignore"):
        a = (d[0] * e[0] + d[1] * e[1]) / n2
        b = (d[0] * e[1] - d[1] * e[0]) / n2
        tx = Q[i, 0] - (a * P[i, 0] - b * P[i, 1])
        ty = Q[i, 1] - (b * P[i, 0] + a * P[i, 1])
    return a, b, tx, ty


def inliers(model, P, Q, thr: float):
    a, b, tx, ty = model
    with np.errstate(all="ignore"):
        rx = ((a * P[:, 0] - b * P[:, 1]) + tx) - Q[:, 0]
        ry = ((b * P[:, 0] + a * P[:, 1]) + ty) - Q[:, 1]
        return rx * rx + ry * ry <= thr * thr


def lstsq_similarity(P, Q):
    """Least-squares [a -b tx; b a ty] taking P to Q, or None when P has no spread."""
    if len(P) < 1 or not np.sum((P - P.mean(0)) ** 2) > 0:
        return None
    n = len(P)
    A = np.zeros((2 * n, 4))
    A[:n, 0], A[:n, 1], A[:n, 2] = P[:, 0], -P[:, 1], 1.0
    A[n:, 0], A[n:, 1], A[n:, 3] = P[:, 1], P[:, 0], 1.0
    # centred columns keep the normal equations well conditioned (the fit is translation-covariant)
    a, b, tx, ty = np.linalg.lstsq(A, np.concatenate([Q[:, 0], Q[:, 1]]), rcond=None)[0]
    return np.array([[a, -b, tx], [b, a, ty]])


def fit(P, Q, thr: float = 3.0):
    """(warp [2, 3], code, winner index, inlier mask) of the tracked pairs P -> Q."""
    m = len(P)
    none = np.zeros(m, bool)
    if m < 4:
        return EYE.copy(), TOO_FEW, -1, none
    best, bk, bin_ = -1, -1, none
    for k in range(HYPOTHESES):
        model = hypothesis(P, Q, k)
        if model is None:
            continue
        inl = inliers(model, P, Q, thr)
        if int(inl.sum()) > best:
            best, bk, bin_ = int(inl.sum()), k, inl
    if bk < 0:
        return EYE.copy(), NO_MODEL, -1, none
    M = lstsq_similarity(P[bin_], Q[bin_])
    if M is None:
        return EYE.copy(), NO_MODEL, -1, none
    return M, OK, bk, bin_


# -------------------------------------------------------------------------------------- state
class SofRef:
    """One camera: the state and the exits of SOF.apply (the reference's settings as defaults)."""

    def __init__(self, scale=0.15, max_corners: int = 1000, quality_level: float = 0.01,
                 win_size: int = 21, max_level: int = 3, max_iter: int = 30, eps: float = 0.01,
                 threshold: float = 3.0):
        self.scale, self.max_corners, self.quality = scale, max_corners, quality_level
        self.win, self.max_level, self.max_iter, self.eps = win_size, max_level, max_iter, eps
        self.threshold = threshold
        self.levels = None   # previous pyramid
        self.kp = None       # keypoints held
        self.record = None   # the last tracking record

    def apply(self, img: np.ndarray):
        """(warp [2, 3] float64, code, n_keypoints, n_tracked, n_inliers)"""
        cur = pyramid(prep(img, self.scale), self.win, self.max_level)
        first = (self.levels is None or len(self.levels) != len(cur)
                 or self.levels[0].shape != cur[0].shape)
        new_kp = keypoints(cur[0], self.max_corners, self.quality)
        if first:
            self.record = None
            if len(new_kp) == 0:
                self.levels, self.kp = None, None
                return EYE.copy(), NO_KEYPOINTS, 0, 0, 0
            self.levels, self.kp = cur, new_kp
            return EYE.copy(), FIRST_FRAME, len(new_kp), 0, 0
        derivs = [scharr(g) for g in self.levels]
        res = [track_point(self.levels, cur, derivs, p, self.win, self.max_iter, self.eps)
               for p in self.kp]
        nxt = np.array([r[0] for r in res]).reshape(-1, 2)
        ok = np.array([r[1] for r in res], bool)
        its = np.array([r[2] for r in res], np.int32)
        P, Q = self.kp[ok], nxt[ok]
        M, code, winner, inl = fit(P, Q, self.threshold)
        full = np.zeros(len(ok), bool)
        full[np.flatnonzero(ok)[inl]] = True
        self.record = {"prev": self.kp.copy(), "next": nxt, "tracked": ok, "iterations": its,
                       "inlier": full, "winner": winner}
        if code == OK and self.scale is not None and self.scale < 1:
            M = M.copy()
            M[0, 2] = M[0, 2] / self.scale
            M[1, 2] = M[1, 2] / self.scale
        self.levels = cur
        self.kp = new_kp if len(new_kp) else Q.copy()
        return M, code, len(self.kp), int(ok.sum()), int(inl.sum()) if code == OK else 0


# ------------------------------------------------------------------------------ test textures
def texture(h: int, w: int, seed: int, A=None):
    """ecc_ref's analytic texture (24 sinusoids of period 8 to 16 px) seen through the warp A."""
    return E.texture(h, w, seed, A)


def sim_warp(deg: float, zoom: float, dx: float, dy: float, cx: float = 0.0, cy: float = 0.0):
    """Rotation by deg and zoom about (cx, cy), then a shift."""
    t = np.deg2rad(deg)
    a, b = zoom * np.cos(t), zoom * np.sin(t)
    return np.array([[a, -b, cx - (a * cx - b * cy) + dx], [b, a, cy - (b * cx + a * cy) + dy]])


def two_motion_frame(h: int, w: int, seed: int, A_bg, A_patch, box):
    """The texture seen through A_bg, except inside box = (x0, y0, x1, y1) where it is seen
    through A_patch (a foreground that moves on its own)."""
    f = texture(h, w, seed, A_bg)
    g = texture(h, w, seed, A_patch)
    x0, y0, x1, y1 = box
    f[y0:y1, x0:x1] = g[y0:y1, x0:x1]
    return f

"""A float64 numpy restatement of the ECC camera-motion contract (DESIGN.md 2.14,
include/bxcmc.h): the oracle of tests/test_cmc_host.py and tests/test_cmc_gpu.py.

The preprocessing is the header's integer arithmetic.  The iteration is written the textbook way
(Evangelidis & Psarakis 2008): warp the image and its gradients, zero-mean image and template
under the mask, build the Jacobian, the Hessian and the two projections from them, then lambda
and the parameter step.  It does not go through expanded raw moments, so it checks the kernel's
algebra and not only its sums.  OpenCV is not involved anywhere.
"""
from __future__ import annotations

import numpy as np

TRANSLATION, EUCLIDEAN, AFFINE = 0, 1, 2
OK, FIRST_FRAME, NOT_CONVERGED = 0, 1, 2


# ------------------------------------------------------------------------------ preprocessing
def work_size(H: int, W: int, scale):
    if scale is None or scale >= 1:
        return H, W
    return int(np.rint(H * scale)), int(np.rint(W * scale))  # np.rint: half to even


def grey(img: np.ndarray) -> np.ndarray:
    """BGR uint8 [H, W, 3] -> grey int64 [H, W] (a grey [H, W] input passes through)."""
    if img.ndim == 2:
        return img.astype(np.int64)
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14


def axis_taps(n_out: int, scale: float, L: int):
    """(s0, s1, q) of every output index of an axis of source length L."""
    f = (np.arange(n_out, dtype=np.float64) + 0.5) / scale - 0.5
    fl = np.floor(f)
    a = f - fl
    lo, hi = fl < 0, fl >= L - 1
    s0 = np.where(lo, 0, np.where(hi, L - 1, fl)).astype(np.int64)
    a = np.where(lo | hi, 0.0, a)
    s1 = np.minimum(s0 + 1, L - 1)
    return s0, s1, np.rint(a * 2048.0).astype(np.int64)


def resize(g: np.ndarray, scale: float) -> np.ndarray:
    H, W = g.shape
    h, w = work_size(H, W, scale)
    x0, x1, qx = axis_taps(w, scale, W)
    y0, y1, qy = axis_taps(h, scale, H)
    qx, qy = qx[None, :], qy[:, None]
    g00, g01 = g[y0][:, x0], g[y0][:, x1]
    g10, g11 = g[y1][:, x0], g[y1][:, x1]
    v = (g00 * (2048 - qx) * (2048 - qy) + g01 * qx * (2048 - qy) + g10 * (2048 - qx) * qy
         + g11 * qx * qy + (1 << 21)) >> 22
    return v


def gradients(g: np.ndarray):
    """Central differences with reflect-101 borders, float32 (exact: multiples of 0.5)."""
    h, w = g.shape
    f = g.astype(np.float64)
    px = np.pad(f, ((0, 0), (1, 1)), mode="reflect") if w > 1 else np.repeat(f, 3, axis=1)
    py = np.pad(f, ((1, 1), (0, 0)), mode="reflect") if h > 1 else np.repeat(f, 3, axis=0)
    gx = 0.5 * (px[:, 2:] - px[:, :-2])
    gy = 0.5 * (py[2:, :] - py[:-2, :])
    return gx.astype(np.float32), gy.astype(np.float32)


def prep(img: np.ndarray, scale):
    """(grey uint8 [h, w], gx, gy float32 [h, w]) of a frame."""
    g = grey(img)
    if scale is not None and scale < 1:
        g = resize(g, float(scale))
    gx, gy = gradients(g)
    return g.astype(np.uint8), gx, gy


# ---------------------------------------------------------------------------------- iteration
def sample(plane: np.ndarray, xs: np.ndarray, ys: np.ndarray) -> np.ndarray:
    """Bilinear samples with a zero border."""
    h, w = plane.shape
    fx, fy = np.floor(xs), np.floor(ys)
    ax, ay = xs - fx, ys - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    p = np.pad(plane.astype(np.float64), 1)  # index + 1: taps -1 and w read zeros

    def at(x, y):
        return p[y + 1, x + 1]

    return ((1 - ax) * (1 - ay) * at(x0, y0) + ax * (1 - ay) * at(x0 + 1, y0)
            + (1 - ax) * ay * at(x0, y0 + 1)) + ax * ay * at(x0 + 1, y0 + 1)


def mask_count(M, h: int, w: int) -> int:
    """Template pixels whose nearest source pixel under the warp M lies inside the h x w image."""
    M = np.asarray(M, np.float64).reshape(2, 3)
    Y, X = np.mgrid[0:h, 0:w].astype(np.float64)
    nx = np.floor(M[0, 0] * X + M[0, 1] * Y + M[0, 2] + 0.5)
    ny = np.floor(M[1, 0] * X + M[1, 1] * Y + M[1, 2] + 0.5)
    return int(((nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)).sum())


def ecc_solve(T: np.ndarray, I: np.ndarray, gx: np.ndarray, gy: np.ndarray, mode: int,
              eps: float, max_iter: int, init=None):
    """Align image I (with gradients gx, gy) to template T.  Returns (warp [2, 3], rho,
    iterations, code); the warp takes template coordinates to image coordinates and is the
    identity unless code is OK."""
    h, w = T.shape
    eye = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    M = eye.copy() if init is None else np.asarray(init, np.float64).reshape(2, 3).copy()
    theta = np.arcsin(M[1, 0])
    Y, X = np.mgrid[0:h, 0:w].astype(np.float64)
    Tf = T.astype(np.float64)
    rho, last_rho, it = -1.0, -eps, 0
    with np.errstate(all="ignore"):
        while it + 1 <= max_iter and abs(rho - last_rho) >= eps:
            it += 1
            last_rho = rho
            xs = M[0, 0] * X + M[0, 1] * Y + M[0, 2]
            ys = M[1, 0] * X + M[1, 1] * Y + M[1, 2]
            nx, ny = np.floor(xs + 0.5), np.floor(ys + 0.5)  # nearest source pixel
            mask = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
            xm, ym = np.where(mask, xs, 0.0), np.where(mask, ys, 0.0)
            Iw, gxw, gyw = (sample(p, xm, ym)[mask] for p in (I, gx, gy))
            Tm, Xm, Ym = Tf[mask], X[mask], Y[mask]
            if Iw.size == 0:
                return eye, float("nan"), it, NOT_CONVERGED
            Izm, Tzm = Iw - Iw.mean(), Tm - Tm.mean()
            if mode == TRANSLATION:
                J = np.stack([gxw, gyw], 1)
            elif mode == EUCLIDEAN:
                c, s = M[0, 0], M[1, 0]
                J = np.stack([gxw * (-Xm * s - Ym * c) + gyw * (Xm * c - Ym * s), gxw, gyw], 1)
            else:
                J = np.stack([gxw * Xm, gyw * Xm, gxw * Ym, gyw * Ym, gxw, gyw], 1)
            H = J.T @ J
            ip, tp = J.T @ Izm, J.T @ Tzm
            corr = float(Tzm @ Izm)
            nI, nT = np.linalg.norm(Izm), np.linalg.norm(Tzm)
            rho = corr / (nI * nT)
            if np.isnan(rho):
                return eye, rho, it, NOT_CONVERGED
            try:
                np.linalg.cholesky(H)
                hi = np.linalg.solve(H, ip)
            except np.linalg.LinAlgError:
                return eye, rho, it, NOT_CONVERGED
            ln, ld = nI * nI - ip @ hi, corr - tp @ hi
            if not ld > 0:
                return eye, rho, it, NOT_CONVERGED
            dp = np.linalg.solve(H, (ln / ld) * tp - ip)
            if mode == TRANSLATION:
                M[0, 2] += dp[0]
                M[1, 2] += dp[1]
            elif mode == EUCLIDEAN:
                theta += dp[0]
                M[0, 2] += dp[1]
                M[1, 2] += dp[2]
                M[0, 0] = M[1, 1] = np.cos(theta)
                M[1, 0] = np.sin(theta)
                M[0, 1] = -M[1, 0]
            else:
                M[0, 0] += dp[0]
                M[1, 0] += dp[1]
                M[0, 1] += dp[2]
                M[1, 1] += dp[3]
                M[0, 2] += dp[4]
                M[1, 2] += dp[5]
    return M, float(rho), it, OK


class EccRef:
    """One camera: the state and the exits of ECC.apply (the reference's settings as defaults)."""

    def __init__(self, warp_mode: int = TRANSLATION, eps: float = 1e-5, max_iter: int = 100,
                 scale=0.15):
        self.mode, self.eps, self.max_iter, self.scale = warp_mode, eps, max_iter, scale
        self.prev = None

    def apply(self, img: np.ndarray, init=None):
        """(warp [2, 3] float64, rho, iterations, code)"""
        g, gx, gy = prep(img, self.scale)
        prev, self.prev = self.prev, g
        if prev is None or prev.shape != g.shape:
            return np.array([[1.0, 0, 0], [0, 1.0, 0]]), 0.0, 0, FIRST_FRAME
        M, rho, it, code = ecc_solve(prev, g.astype(np.float64), gx, gy, self.mode, self.eps,
                                     self.max_iter, init)
        if code == OK and self.scale is not None and self.scale < 1:
            M = M.copy()
            M[0, 2] = M[0, 2] / self.scale
            M[1, 2] = M[1, 2] / self.scale
        return M, rho, it, code


# ------------------------------------------------------------------------------ test textures
def texture(h: int, w: int, seed: int, A=None, n_waves: int = 24, amp: float = 12.0):
    """An analytic texture f (a sum of sinusoids of period 8 to 16 px around 128) seen through the
    2x3 warp A, rounded to uint8: the image I with I(A x) = f(x), so that aligning it to the
    unwarped texture recovers A.  A None is the identity."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n_waves)
    freq = 1.0 / rng.uniform(8.0, 16.0, n_waves)
    ph = rng.uniform(0, 2 * np.pi, n_waves)
    Y, X = np.mgrid[0:h, 0:w].astype(np.float64)
    if A is not None:
        A = np.asarray(A, np.float64).reshape(2, 3)
        Li = np.linalg.inv(A[:, :2])
        U, V = X - A[0, 2], Y - A[1, 2]
        X, Y = Li[0, 0] * U + Li[0, 1] * V, Li[1, 0] * U + Li[1, 1] * V
    f = np.full((h, w), 128.0)
    for a, k, p in zip(ang, freq, ph):
        f += amp * np.sin(2 * np.pi * k * (np.cos(a) * X + np.sin(a) * Y) + p)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def shift_warp(dx: float, dy: float):
    return np.array([[1.0, 0, dx], [0, 1.0, dy]])


def rot_warp(deg: float, dx: float, dy: float):
    t = np.deg2rad(deg)
    return np.array([[np.cos(t), -np.sin(t), dx], [np.sin(t), np.cos(t), dy]])


# ---------------------------------------------------------------------------------- test cases
AFFINE_A = np.array([[1.01, 0.004, 0.6], [-0.006, 0.99, -0.4]])
# name: (h, w, seed, mode, true warp A, initial warp or None, max_iter); the first frame is the
# texture, the second the texture seen through A.  Periods of 8 to 16 px make the two large
# shifts leave the basin of convergence (the non-positive-denominator exit).
CASES = {
    "shift_a": (48, 64, 1, TRANSLATION, shift_warp(1.3, -0.7), None, 100),
    "shift_b": (48, 64, 2, TRANSLATION, shift_warp(-0.4, 0.15), None, 100),
    "shift_c": (48, 64, 3, TRANSLATION, shift_warp(0.6, 1.1), None, 100),
    "euclidean": (48, 64, 1, EUCLIDEAN, rot_warp(0.4, 0.5, -0.3), None, 100),
    "affine": (48, 64, 1, AFFINE, AFFINE_A, None, 100),
    "large_a": (48, 64, 1, TRANSLATION, shift_warp(3.25, 2.5), None, 100),
    "large_b": (48, 64, 1, TRANSLATION, shift_warp(6.0, -4.0), None, 100),
    # shapes: fewer pixels than a wave; a partial last wave; the real working size; a third of
    # the template outside the image; the loop's count exits
    "tiny": (5, 7, 5, TRANSLATION, shift_warp(0.3, -0.2), None, 100),
    "odd": (33, 65, 1, TRANSLATION, shift_warp(0.3, -0.2), None, 100),
    "full": (162, 288, 1, TRANSLATION, shift_warp(1.3, -0.7), None, 100),
    "outside": (48, 64, 1, TRANSLATION, shift_warp(21.3, 0.4), shift_warp(21.0, 0.0), 100),
    "iter1": (48, 64, 1, TRANSLATION, shift_warp(1.3, -0.7), None, 1),
    "iter3": (48, 64, 1, TRANSLATION, shift_warp(1.3, -0.7), None, 3),
}
_solved = {}


def case_frames(name: str):
    h, w, seed, _, A, _, _ = CASES[name]
    return texture(h, w, seed), texture(h, w, seed, A)


def solve_case(name: str):
    """(warp, rho, iterations, code) of a case's second frame by the restatement (computed once)."""
    if name not in _solved:
        _, _, _, mode, _, init, max_iter = CASES[name]
        a, b = case_frames(name)
        ref = EccRef(mode, max_iter=max_iter, scale=None)
        ref.apply(a)
        _solved[name] = ref.apply(b, init)
    return _solved[name]

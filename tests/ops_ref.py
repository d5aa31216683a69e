"""A numpy/scipy restatement of the stateless op-level entry points (include/bxassoc.h,
bxocsort.h, bxboost.h) and the case builders of tests/test_ops_edges_host.py and
tests/test_ops_edges_gpu.py.

Written from the formulas, whole arrays at a time, with numpy's and scipy's own routines where
the reference calls them (np.linalg.norm, scipy cdist, cho_factor / cho_solve, np.linalg.cholesky,
solve_triangular, np.arctan) — no hand-ordered sums, no fdlibm restatements.  The host test pins
it to the reference-captured vectors of tests/golden/ and then holds the C oracle against it on
every case built here; the GPU test holds the HIP ops against both.

How the oracle compares with this file on the CPU, over every case below (`BITWISE`, `TOL`; the
host test asserts it, the GPU test applies the same rule to the HIP ops):

  iou, hmiou, giou, diou, centroid   bitwise
  ciou                               np.arctan vs the restated fdlibm atan; worst 2.3e-16 absolute
                                     (held to atol 4e-16)
  fuse_score                         bitwise
  embedding_distance                 bitwise (every width and content below)
  aw_max_metric                      bitwise, the Inf case included once the oracle's and the
                                     kernel's max(ratio - bottom, 0) kept a NaN as Python's does
  kf initiate, multi_predict         bitwise
  kf update (LAPACK / BLAS order)    mean: worst 6.6e-14 relative, 2.3e-13 absolute (held to
                                     rtol 1e-12, atol 1e-9); covariance: worst 3.1e-14 of the
                                     matrix's largest entry, 2.4e-10 absolute (held to rtol
                                     1e-10, atol 1e-9)
  kf gating_distance                 worst 7.9e-16 relative (held to rtol 1e-10)
  boost mh_dist                      bitwise

A track whose projected covariance is not positive definite makes scipy / numpy raise
LinAlgError in the reference; the oracle and the HIP ops leave such a track's state unchanged on
update and write NaN gating distances (bx_device.h chol4).  kf_update / kf_gating_distance here
follow that convention, so a batch holding one such track is an ordinary case.
"""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np
import scipy.linalg
from scipy.spatial.distance import cdist

GOLDEN = Path(__file__).parent / "golden"
FRAME_W, FRAME_H = 1920, 1080
ASSO_KINDS = ("iou", "hmiou", "giou", "diou", "ciou", "centroid")

# ---------------------------------------------------------------------------- comparison rule
# op -> True (bitwise) or the assert_allclose keywords the project already holds against the
# reference (tests/test_oracle.py, tests/test_gpu_parity.py)
BITWISE = {"iou": True, "hmiou": True, "giou": True, "diou": True, "ciou": False,
           "centroid": True, "fuse": True, "embedding": True, "aw": True, "kf_initiate": True,
           "kf_predict": True, "kf_update_mean": False, "kf_update_cov": False,
           "kf_gating": False, "mh_dist": True}
TOL = {"ciou": dict(rtol=0, atol=4e-16), "kf_update_mean": dict(rtol=1e-12, atol=1e-9),
       "kf_update_cov": dict(rtol=1e-10, atol=1e-9), "kf_gating": dict(rtol=1e-10)}


def assert_matches(op, got, want):
    """got against this file's result for `op`: bitwise or the op's tolerance (NaNs must match)."""
    if BITWISE[op]:
        np.testing.assert_array_equal(got, want)
    else:
        np.testing.assert_allclose(got, want, **TOL[op])


# ------------------------------------------------------------------- association functions
def _pairs(a, b):
    a = np.asarray(a, np.float64).reshape(-1, 4)[:, None, :]
    b = np.asarray(b, np.float64).reshape(-1, 4)[None, :, :]
    return a, b


def _overlap(a, b):
    """Intersection width, height and area; the two box areas."""
    iw = np.maximum(0.0, np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]))
    ih = np.maximum(0.0, np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]))
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return iw, ih, iw * ih, area_a, area_b


def _enclosing(a, b):
    return (np.maximum(a[..., 2], b[..., 2]) - np.minimum(a[..., 0], b[..., 0]),
            np.maximum(a[..., 3], b[..., 3]) - np.minimum(a[..., 1], b[..., 1]))


def _centre_gap_sq(a, b):
    dx = (a[..., 0] + a[..., 2]) / 2.0 - (b[..., 0] + b[..., 2]) / 2.0
    dy = (a[..., 1] + a[..., 3]) / 2.0 - (b[..., 1] + b[..., 3]) / 2.0
    return dx ** 2 + dy ** 2


def iou_batch(a, b):
    a, b = _pairs(a, b)
    _, _, inter, area_a, area_b = _overlap(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area_a + area_b - inter)


def hmiou_batch(a, b):
    """IoU (1e-10 in the denominator) times the ratio of common height to spanned height."""
    a, b = _pairs(a, b)
    _, ih, inter, area_a, area_b = _overlap(a, b)
    _, eh = _enclosing(a, b)
    return inter / (area_a + area_b - inter + 1e-10) * (ih / np.maximum(1e-10, eh))


def giou_batch(a, b):
    a, b = _pairs(a, b)
    _, _, inter, area_a, area_b = _overlap(a, b)
    union = area_a + area_b - inter
    ew, eh = _enclosing(a, b)
    assert (ew > 0).all() and (eh > 0).all(), "giou: enclosing box of zero size (caller's duty)"
    enc = ew * eh
    return (inter / union - (enc - union) / enc + 1.0) / 2.0


def diou_batch(a, b):
    a, b = _pairs(a, b)
    _, _, inter, area_a, area_b = _overlap(a, b)
    ew, eh = _enclosing(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / (area_a + area_b - inter)
        return (iou - _centre_gap_sq(a, b) / (ew ** 2 + eh ** 2) + 1) / 2.0


def ciou_batch(a, b):
    eps = 1e-7
    a, b = _pairs(a, b)
    _, _, inter, area_a, area_b = _overlap(a, b)
    iou = inter / (area_a + area_b - inter + eps)
    ew, eh = _enclosing(a, b)
    gap = _centre_gap_sq(a, b) / (ew ** 2 + eh ** 2 + eps)
    ratio_a = (a[..., 2] - a[..., 0]) / (a[..., 3] - a[..., 1] + eps)
    ratio_b = (b[..., 2] - b[..., 0]) / (b[..., 3] - b[..., 1] + eps)
    v = (4 / np.pi ** 2) * (np.arctan(ratio_b) - np.arctan(ratio_a)) ** 2
    alpha = v / (1 - iou + v + eps)
    return (iou - gap + alpha * v + 1) / 2.0


def centroid_batch(a, b, w=FRAME_W, h=FRAME_H):
    a, b = _pairs(a, b)
    return 1 - np.sqrt(_centre_gap_sq(a, b)) / np.sqrt(w ** 2 + h ** 2)


def asso_batch(kind, a, b, w=FRAME_W, h=FRAME_H):
    if kind == "centroid":
        return centroid_batch(a, b, w, h)
    return {"iou": iou_batch, "hmiou": hmiou_batch, "giou": giou_batch, "diou": diou_batch,
            "ciou": ciou_batch}[kind](a, b)


def fuse_score(cost, confs, threshold=0.5):
    """The fork's enhanced_fuse_score with confidence weighting: similarity times the detection
    confidence (boosted by 1.2 above 0.7, dropped below the threshold), back to a cost, doubled
    below the threshold."""
    cost = np.asarray(cost, np.float64)
    conf = np.broadcast_to(np.asarray(confs, np.float64)[None, :], cost.shape)
    weight = np.where(conf > 0.7, conf * 1.2, conf)
    fused = 1 - (1 - cost) * weight * (conf >= threshold)
    return np.where(conf < threshold, fused * 2.0, fused)


def embedding_distance(trk, det):
    """float32 rows over (float32 norm + 1e-8), scipy's cosine distance, clipped at 0."""
    trk = np.asarray(trk, np.float32)
    det = np.asarray(det, np.float32)
    trk = trk / (np.linalg.norm(trk, axis=1, keepdims=True) + 1e-8)
    det = det / (np.linalg.norm(det, axis=1, keepdims=True) + 1e-8)
    assert trk.dtype == np.float32 and det.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return np.maximum(0.0, cdist(trk, det, "cosine"))


def _aw_line_weight(line, bottom):
    """Weight of one row or column, or None when it has fewer than two positive entries."""
    pos = np.sort(line[line > 0])[::-1]
    if pos.size < 2:
        return None
    if pos[0] == 0:
        return 0
    with np.errstate(invalid="ignore"):  # Inf / Inf
        return 1 - max(pos[1] / pos[0] - bottom, 0) / (1 - bottom)


def aw_max_metric(emb, w_assoc, bottom=0.5):
    emb = np.asarray(emb, np.float64)
    w = np.full_like(emb, w_assoc)
    for i in range(emb.shape[0]):
        lw = _aw_line_weight(emb[i], bottom)
        if lw is not None:
            w[i] *= lw
    for j in range(emb.shape[1]):
        lw = _aw_line_weight(emb[:, j], bottom)
        if lw is not None:
            w[:, j] *= lw
    with np.errstate(invalid="ignore"):  # NaN weight times 0 or Inf
        return w * emb


# ------------------------------------------------------------------- XYAH / XYWH filter
STD_POS, STD_VEL = 1.0 / 20, 1.0 / 160
_F = np.eye(8)
_F[:4, 4:] = np.eye(4)
_H = np.eye(4, 8)


def _scale(kind, m):
    """The length each state component's noise is proportional to ([..., 4]); XYAH's aspect
    ratio (index 2) has constant noise instead."""
    m = np.asarray(m, np.float64)
    if kind == "xyah":
        return np.stack([m[..., 3]] * 4, -1)
    return np.stack([m[..., 2], m[..., 3], m[..., 2], m[..., 3]], -1)


def _noise_std(kind, m, kp, kv, a_pos, a_vel):
    s = _scale(kind, m)
    std = np.concatenate([kp * STD_POS * s, kv * STD_VEL * s], -1)
    if kind == "xyah":
        std[..., 2] = a_pos
        std[..., 6] = a_vel
    return std


def kf_initiate(kind, meas):
    """meas [n,4] -> mean [n,8], covariance [n,8,8]."""
    meas = np.asarray(meas, np.float64).reshape(-1, 4)
    mean = np.concatenate([meas, np.zeros_like(meas)], 1)
    std = _noise_std(kind, meas, 2, 10, 1e-2, 1e-5)
    return mean, np.stack([np.diag(np.square(s)) for s in std])


def kf_multi_predict(kind, mean, cov):
    mean = np.asarray(mean, np.float64)
    cov = np.asarray(cov, np.float64)
    q = np.square(_noise_std(kind, mean, 1, 1, 1e-2, 1e-5))
    Q = np.stack([np.diag(r) for r in q])
    return mean @ _F.T, _F @ cov @ _F.T + Q


def _project(kind, mean, cov, conf):
    std = (1 - conf) * _noise_std(kind, mean, 1, 1, 1e-1, 0.0)[:4]
    return _H @ mean, _H @ cov @ _H.T + np.diag(np.square(std))


def kf_update(kind, mean, cov, z, conf=0.0):
    """One track.  Not positive definite: the state stays (module docstring)."""
    mean = np.asarray(mean, np.float64)
    cov = np.asarray(cov, np.float64)
    pm, S = _project(kind, mean, cov, conf)
    try:
        factor = scipy.linalg.cho_factor(S, lower=True, check_finite=False)
    except np.linalg.LinAlgError:
        return mean.copy(), cov.copy()
    K = scipy.linalg.cho_solve(factor, (cov @ _H.T).T, check_finite=False).T
    return mean + (np.asarray(z, np.float64) - pm) @ K.T, cov - K @ S @ K.T


def kf_gating_distance(kind, mean, cov, zs):
    """One track against zs [nz,4]: squared Mahalanobis distances [nz]."""
    zs = np.asarray(zs, np.float64).reshape(-1, 4)
    pm, S = _project(kind, np.asarray(mean, np.float64), np.asarray(cov, np.float64), 0.0)
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return np.full(zs.shape[0], np.nan)
    y = scipy.linalg.solve_triangular(L, (zs - pm).T, lower=True, check_finite=False)
    return np.sum(y * y, axis=0)


def kf_update_batch(kind, mean, cov, z, conf):
    out = [kf_update(kind, mean[i], cov[i], z[i], conf[i]) for i in range(mean.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def kf_gating_batch(kind, mean, cov, zs):
    return np.stack([kf_gating_distance(kind, mean[i], cov[i], zs) for i in range(mean.shape[0])])


def boost_mh_dist(dets, x, P):
    """BoostTrack's diagonal Mahalanobis distance: detections [nd,4] xyxy as (cx, cy, h, w/h)
    against the first four state components of tracks x [nt,8], P [nt,8,8] -> [nd,nt]."""
    d = np.asarray(dets, np.float64).reshape(-1, 4)
    w, h = d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]
    z = np.stack([d[:, 0] + w / 2.0, d[:, 1] + h / 2.0, h, w / (h + 1e-6)], 1)
    x = np.asarray(x, np.float64)[:, :4]
    inv = np.reciprocal(np.stack([np.diag(p)[:4] for p in np.asarray(P, np.float64)]))
    return ((z[:, None, :] - x[None, :, :]) ** 2 * inv[None, :, :]).sum(axis=2)


# ------------------------------------------------------------------------- case builders
def _rng(*key):
    return np.random.default_rng([20240611, *key])


# output shapes of the element-wise ops: one element, a row / a column one past a block of 256,
# one short of a block, exactly a block, and 1031 x 1021 = 1,052,651 — 4,075 elements into the
# second trip of a 4096 x 256 grid-stride loop, both sides prime
EW_SHAPES = [(1, 1), (1, 257), (257, 1), (3, 85), (16, 16), (1031, 1021)]
STRIDES = [(4, 4), (7, 4), (4, 7), (7, 7)]  # lda, ldb of bx_pairwise_cost
EMB_F_SMALL, EMB_F_BIG = 33, 9  # feature widths at the element-wise shapes (9 at 1031 x 1021)


def rand_boxes(rng, n):
    """n xyxy boxes of 4..400 px in the frame; from 8 boxes on, an eighth of them moved to
    coordinates around 1e7 and an eighth to all-negative coordinates."""
    c = rng.uniform((0, 0), (FRAME_W, FRAME_H), (n, 2))
    s = rng.uniform(4, 400, (n, 2))
    b = np.concatenate([c - s / 2, c + s / 2], 1)
    q = n // 8
    if q:
        b[n - 2 * q:n - q] += 1e7
        b[n - q:] -= 4000.0
    return b


@functools.lru_cache(maxsize=None)
def box_case(shape):
    """(a [na,4], b [nb,4]): random boxes; b's rows are jittered, rescaled copies of a's rows so
    that many pairs overlap."""
    na, nb = shape
    rng = _rng(1, na, nb)
    a = rand_boxes(rng, na)
    src = a[rng.integers(0, na, nb)]
    c = (src[:, :2] + src[:, 2:]) / 2 + rng.normal(0, 6, (nb, 2))
    s = (src[:, 2:] - src[:, :2]) * rng.uniform(0.8, 1.25, (nb, 2))
    b = np.concatenate([c - s / 2, c + s / 2], 1)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def strided(boxes, ld):
    """Rows of stride ld with NaN in the padding, so a read off the box shows."""
    out = np.full((boxes.shape[0], ld), np.nan)
    out[:, :4] = boxes
    return out


# designated degenerate rows: the op runs on every (a row, b row) pair of them
DEGENERATE_A = np.array([[10.0, 20.0, 110.0, 220.0],      # identical to b[0]
                         [200.0, 200.0, 300.0, 300.0],    # touches b[1] along an edge
                         [0.0, 0.0, 50.0, 50.0],          # disjoint from b[2]
                         [400.0, 400.0, 800.0, 800.0],    # contains b[3]
                         [100.0, 100.0, 100.0, 200.0],    # zero width, against itself: 0/0
                         [700.0, 700.0, 700.001, 700.001]])  # 1e-3 px, overlapping b[5]
DEGENERATE_B = np.array([[10.0, 20.0, 110.0, 220.0],
                         [300.0, 200.0, 400.0, 300.0],
                         [1000.0, 800.0, 1100.0, 900.0],
                         [500.0, 500.0, 600.0, 600.0],
                         [100.0, 100.0, 100.0, 200.0],
                         [700.0005, 700.0005, 700.0015, 700.0015]])
ZERO_WIDTH_ROW = 4


def degenerate_boxes(kind):
    """giou's enclosing box must have positive size (the caller's duty, bxassoc.h): its case
    leaves the zero-width row out of a, so no pair has an enclosing box of zero size."""
    a = np.delete(DEGENERATE_A, ZERO_WIDTH_ROW, 0) if kind == "giou" else DEGENERATE_A
    return a, DEGENERATE_B


FUSE_CONFS = (0.0, 0.5, 0.7, 1.0, float(np.nextafter(0.5, 0)), float(np.nextafter(0.7, 1)))


@functools.lru_cache(maxsize=None)
def fuse_case(shape):
    """(cost [nr,nc] in [0,1], confs [nc]): random confidences with the six threshold values
    spread over the columns (one of them when there are fewer than six columns)."""
    nr, nc = shape
    rng = _rng(2, nr, nc)
    cost = rng.uniform(0, 1, (nr, nc))
    conf = rng.uniform(0, 1, nc)
    if nc >= len(FUSE_CONFS):
        conf[np.linspace(0, nc - 1, len(FUSE_CONFS)).astype(int)] = FUSE_CONFS
    else:
        conf[0] = FUSE_CONFS[(nr + nc) % len(FUSE_CONFS)]
    cost.setflags(write=False)
    conf.setflags(write=False)
    return cost, conf


EMB_WIDTHS = [1, 2, 7, 8, 9, 15, 127, 128, 129, 136, 257, 264, 1000]
EMB_COUNTS = [(1, 1), (129, 3), (3, 129)]
EMB_CONTENTS = ["normal", "relu"]


@functools.lru_cache(maxsize=None)
def emb_case(nt, nd, f, content="normal"):
    """(trk [nt,f], det [nd,f]) float32.  "relu": exact zeros where a normal draw is negative,
    the first component kept positive so that no row is all zero.  "zero_row": normal content
    with one all-zero track row and one all-zero detection row (the designated degenerate
    case)."""
    rng = _rng(3, nt, nd, f, EMB_CONTENTS.index(content) if content in EMB_CONTENTS else 9)
    out = []
    for n in (nt, nd):
        x = rng.standard_normal((n, f)).astype(np.float32)
        if content == "relu":
            x = np.maximum(x, np.float32(0))
            x[:, 0] = np.abs(rng.standard_normal(n)).astype(np.float32) + np.float32(0.01)
        if content == "zero_row":
            x[n // 2] = 0
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


AW_SHAPES = [(1, 1), (2, 1), (1, 2), (33, 32), (65, 64), (1025, 3), (3, 1025), (4096, 1),
             (1, 4096)]
AW_BOTTOMS = [0.5, 0.3]
AW_W = 0.75


@functools.lru_cache(maxsize=None)
def aw_case(shape, bottom):
    """Embedding costs with about 30% exact zeros and about 20% negatives; where the matrix has
    five lines of at least three entries (rows, else columns): an all-zero line, an all-negative
    line, a line with one positive entry, a line whose maximum appears twice (ratio 1) and a
    line whose two largest are 1 and `bottom` (ratio exactly `bottom`)."""
    nr, nc = shape
    rng = _rng(4, nr, nc, int(bottom * 10))
    e = rng.uniform(0.01, 1, (nr, nc))
    u = rng.uniform(0, 1, (nr, nc))
    e[u < 0.3] = 0.0
    e[u > 0.8] *= -1
    m = e if nr >= 5 and nc >= 3 else (e.T if nc >= 5 and nr >= 3 else None)
    if m is not None:
        n = m.shape[1]
        m[0] = 0.0
        m[1] = -rng.uniform(0.01, 1, n)
        m[2] = np.where(np.arange(n) == n // 2, 0.6, np.minimum(m[2], 0.0))
        m[3] = np.minimum(m[3], 0.5)
        m[3, [0, n - 1]] = 0.875
        m[4] = np.minimum(m[4], 0.25)
        m[4, [n - 1, 1]] = (1.0, bottom)
    e.setflags(write=False)
    return e


def aw_inf_case():
    """The designated non-finite case (33 x 32): row 0 holds two +Inf (ratio Inf/Inf = NaN, and
    Python's max(NaN, 0) is NaN: the whole row comes out NaN), row 5 one +Inf (ratio 0, weight
    1, Inf stays Inf); their columns see a ratio of 0."""
    e = aw_case((33, 32), 0.5).copy()
    e[0, [3, 17]] = np.inf
    e[5, 5] = np.inf
    return e


KF_KINDS = ("xyah", "xywh")
KF_COUNTS = [1, 63, 64, 65, 129, 200]  # blocks of 64 (predict, update, gating) and 128 (initiate)
KF_GATE_NZ = [1, 9, 65]
KF_BAD_N, KF_BAD_TRACK = 65, 32


@functools.lru_cache(maxsize=None)
def kf_case(kind, n):
    """One chain of n distinct tracks, every stage from this file: measurements (heights 2 to
    3000 px), initiate, non-zero velocities, three predicts, then the update's and the gating's
    inputs.  conf cycles through 0, 0.5, 1 and random values."""
    rng = _rng(5, KF_KINDS.index(kind), n)
    h = np.geomspace(2.0, 3000.0, n) if n > 1 else np.array([57.0])
    h = h * rng.uniform(0.97, 1.03, n)
    third = rng.uniform(0.3, 1.2, n) if kind == "xyah" else h * rng.uniform(0.3, 1.2, n)
    meas = np.stack([rng.uniform(0, FRAME_W, n), rng.uniform(0, FRAME_H, n), third, h], 1)
    mean0, cov0 = kf_initiate(kind, meas)
    moving = mean0.copy()
    scale = np.stack([h, h, third, h], 1) * 0.02
    moving[:, 4:] = rng.normal(0, 1, (n, 4)) * scale
    preds = []
    m, c = moving, cov0
    for _ in range(3):
        m, c = kf_multi_predict(kind, m, c)
        preds.append((m, c))
    z = m[:, :4] * rng.uniform(0.98, 1.02, (n, 4)) + rng.normal(0, 0.5, (n, 4)) * scale
    conf = np.array([(0.0, 0.5, 1.0, rng.uniform(0.05, 0.95))[i % 4] for i in range(n)])
    gate_z = {nz: m[rng.integers(0, n, nz), :4] * rng.uniform(0.9, 1.1, (nz, 4)) for nz in KF_GATE_NZ}
    case = dict(meas=meas, mean0=mean0, cov0=cov0, moving=moving, preds=preds, pred_mean=m,
                pred_cov=c, z=z, conf=conf, gate_z=gate_z)
    for v in (meas, mean0, cov0, moving, m, c, z, conf, *gate_z.values()):
        v.setflags(write=False)
    return case


def kf_bad_cov(case):
    """The predicted covariances with KF_BAD_TRACK's leading diagonal entry made negative."""
    cov = case["pred_cov"].copy()
    cov[KF_BAD_TRACK, 0, 0] = -cov[KF_BAD_TRACK, 0, 0]
    return cov


OCTET_COUNTS = [1, 7, 9, 33, 65]  # eight lanes per track: 8 tracks per wave, 32 per block
MH_SHAPES = [(1, 1), (7, 37), (257, 1)]
XYSR_Q = (0.01, 0.0001)


@functools.lru_cache(maxsize=None)
def kf_ops_pool(filt):
    """The reference-captured steps of kf_ops.npz for "xysr" or "boost" as one pool of
    steps x 48 distinct, independent tracks: in / pred / upd state, z, and the initiate rows."""
    fx = np.load(GOLDEN / "kf_ops.npz")
    steps = range(int(fx[f"{filt}_steps"]))
    pool = {k: np.concatenate([fx[f"{filt}_s{s}_{k}"] for s in steps])
            for k in ("in_x", "in_P", "pred_x", "pred_P", "z", "upd_x", "upd_P")}
    pool["init_arg"] = fx["xysr_init_box" if filt == "xysr" else "boost_init_z"]
    pool["init_x"], pool["init_P"] = fx[f"{filt}_init_x"], fx[f"{filt}_init_P"]
    if filt == "boost":
        pool["mh_dets"] = np.concatenate([fx[f"boost_s{s}_mh_dets"] for s in steps])
    return pool


def octet_pick(filt, n):
    """(rows of the step pool, rows of the initiate pool) for a batch of n tracks: distinct
    draws; the initiate pool has 48 rows, so past 48 it is a second permutation's head."""
    pool = kf_ops_pool(filt)
    rng = _rng(6, n, 0 if filt == "xysr" else 1)
    steps = rng.permutation(pool["in_x"].shape[0])[:n]
    ni = pool["init_x"].shape[0]
    init = np.concatenate([rng.permutation(ni), rng.permutation(ni)])[:n]
    return steps, init


@functools.lru_cache(maxsize=None)
def mh_case(nd, nt):
    """(dets [nd,4], x [nt,8], P [nt,8,8]) drawn from the captured BoostTrack steps."""
    pool = kf_ops_pool("boost")
    rng = _rng(7, nd, nt)
    d = pool["mh_dets"][rng.permutation(pool["mh_dets"].shape[0])[:nd]]
    t = rng.permutation(pool["pred_x"].shape[0])[:nt]
    return d, pool["pred_x"][t], pool["pred_P"][t]

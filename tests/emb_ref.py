"""Cases and references for the appearance-distance ops (bx_nn_cosine_distance, bx_deepoc_embcost,
bx_hybrid_cosdist, bx_hybrid_bank_mean) of tests/test_emb_edges_host.py and
tests/test_emb_edges_gpu.py.  numpy, fractions and math only: no GPU, no torch, no oracle.

Cases come from seeded generators and are cached (read-only arrays).  Entries are standard normal
draws times a per-row scale, with magnitudes clipped into [1e-3, 1e3] (`entries`), so no square
under- or overflows; exact zeros appear only where a case says so.

Three references:

  exact          dot products, cosine distances and nearest-neighbour distances as
                 fractions.Fraction values, rounded once to float64.  Every float64 is an integer
                 over a power of two, so a whole matrix is held as Python integers over one common
                 denominator (`_ints`) and the sums run on integers; the Fraction is formed at the
                 end.  Square roots are math.isqrt at 2^-256 relative precision, far below half an
                 ulp of the result.
  fma chain      acc = float(Fraction(acc) + Fraction(a) * Fraction(b)), ascending k from 0.0
                 (`fma_chain`).  CPython's int / int division is correctly rounded, so this is an
                 exact fma emulation; slow, so only the listed entries of a matrix are chained
                 (`chain_entries`).
  bank mean      a float64 loop, oldest first (`bank_mean_loop`), with math.fsum for the
                 high-precision side (`bank_mean_fsum`).

Error bounds are the ones the project already holds: 2 F 2^-53 (|D| @ |T|.T) for a dot product
(`dot_bound`), `cosdist_bound` (moved here from tests/test_hybridsort_gpu.py, unchanged) and
atol 1e-13 (`NN_ATOL`) for the nearest-neighbour distance.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
NN_ATOL = 1e-13
BANK = 30  # HybridSort's longterm_bank_length: the depth of a track's feature ring
INFTY_COST = 1e5  # a target without samples
TILE_M, TILE_N, TILE_K = 32, 64, 16  # the shared tile: detections x tracks, K chunk
_K = 256  # bits of the fixed-point square roots


def _rng(*key):
    return np.random.default_rng([20250303, *key])


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def entries(rng, n, f):
    """[n, f] standard normal draws times a per-row scale in [0.1, 10], magnitudes clipped into
    [1e-3, 1e3]."""
    return _clip(rng.standard_normal((n, f)) * 10.0 ** rng.uniform(-1, 1, (n, 1)))


def _clip(x, lo=1e-3, hi=1e3):
    return np.copysign(np.clip(np.abs(x), lo, hi), x)


def in_range(x):
    """Every entry is 0 or has a magnitude in [1e-3, 1e3]."""
    a = np.abs(np.asarray(x))
    return bool(((a == 0) | ((a >= 1e-3) & (a <= 1e3))).all())


# --------------------------------------------------------------------------- exact references
def _ints(x):
    """A float64 array as Python integers over one power-of-two denominator: (ints, shift) with
    x == ints / 2^shift exactly."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    mant = (m * 2.0 ** 53).astype(np.int64)  # exact: |m| < 1 has 53 significant bits
    e = e.astype(np.int64) - 53
    emin = int(e.min()) if x.size else 0
    out = np.empty(x.shape, object)
    flat = out.reshape(-1)
    for i, (a, b) in enumerate(zip(mant.reshape(-1).tolist(), (e - emin).reshape(-1).tolist())):
        flat[i] = a << b
    return out, -emin


def _frac(n, shift):
    return Fraction(int(n), 1 << shift) if shift >= 0 else Fraction(int(n) << -shift)


def _int_dot(a, b):
    """a [n, f] @ b [m, f].T on integer object arrays (also for n or m of 0)."""
    if a.shape[0] == 0 or b.shape[0] == 0:
        return np.empty((a.shape[0], b.shape[0]), object)
    return a.dot(b.T)


def _sumsq(ix):
    return [sum(int(v) * int(v) for v in row) for row in ix]


def exact_dot(D, T):
    """D @ T.T, every entry the exact sum rounded once."""
    iD, sD = _ints(D)
    iT, sT = _ints(T)
    p = _int_dot(iD, iT)
    out = np.empty(p.shape)
    for idx in np.ndindex(*p.shape):
        out[idx] = float(_frac(p[idx], sD + sT))
    return out


def dot_bound(D, T):
    """|computed - exact| of a float64 dot product of width F in any summation order, fused or
    not (DeepOCSort's contraction test): 2 F 2^-53 (|D| @ |T|.T)."""
    return 2 * D.shape[1] * U * (np.abs(D) @ np.abs(T).T)


def exact_cosdist(D, T):
    """max(0, 1 - d.t / (|d| |t|)) [nd, nt], exact and rounded once; NaN where a row is zero
    (np.maximum(0, cdist(..., "cosine")) semantics)."""
    iD, _ = _ints(D)
    iT, _ = _ints(T)
    p = _int_dot(iD, iT)
    qd, qt = _sumsq(iD), _sumsq(iT)
    out = np.empty(p.shape)
    for i, j in np.ndindex(*p.shape):
        if qd[i] == 0 or qt[j] == 0:
            out[i, j] = np.nan
            continue
        root = math.isqrt((qd[i] * qt[j]) << (2 * _K))  # |d||t| 2^K in the dot's own scale
        num = root - (int(p[i, j]) << _K)  # (1 - cos) |d||t| 2^K
        out[i, j] = num / root if num > 0 else 0.0  # int / int: correctly rounded
    return out


def cosdist_ref(T, D):
    """np.maximum(0, cdist(T, D, "cosine")).T: scipy's 1 - u.v / (|u| |v|), in float64."""
    nt = np.sqrt((T * T).sum(1))
    nd = np.sqrt((D * D).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.maximum(0.0, 1.0 - (D @ T.T) / (nd[:, None] * nt[None, :]))


def cosdist_bound(T, D):
    """|got - ref| for two float64 evaluations of 1 - d.t / (|d||t|) in any summation order.
    The dot product: the bound DeepOCSort's contraction test uses, F * 2^-53 * (|D| @ |T|.T), once
    for each side, divided by the norms.  Each norm is the square root of such a sum of F
    non-negative terms (relative error F * 2^-53 / 2, plus one rounding), for two norms and two
    sides; the product of the norms, the division and the subtraction round once each, per side."""
    F = T.shape[1]
    nt = np.sqrt((T * T).sum(1))
    nd = np.sqrt((D * D).sum(1))
    nn = nd[:, None] * nt[None, :]
    dot = 2 * F * U * (np.abs(D) @ np.abs(T).T) / nn
    cos = np.abs(D @ T.T) / nn
    return dot + cos * (2 * (F + 2) * U + 4 * U) + 2 * U


def _den_ints(ix, shift, normalized):
    """(|row| + 1e-8) 2^(K + shift) per row as integers; 2^(K + shift) for rows used as given."""
    if normalized:
        return [1 << (_K + shift)] * ix.shape[0]
    eps = Fraction(1e-8) * (1 << (_K + shift))  # the float64 1e-8, as the reference adds it
    assert eps.denominator == 1
    return [math.isqrt(q << (2 * _K)) + int(eps) for q in _sumsq(ix)]


def exact_nn(samples, off, feats, normalized=False):
    """min over a target's samples of 1 - clip(s.d / ((|s| + 1e-8)(|d| + 1e-8)), -1, 1) [T, D],
    exact and rounded once; 1e5 for a target without samples.  normalized: the samples are used
    as given (BX_NN_SAMPLES_NORMALIZED)."""
    off = np.asarray(off)
    T, (D, F) = off.shape[0] - 1, feats.shape
    out = np.full((T, D), INFTY_COST)
    if off[-1] == 0 or D == 0:
        return out
    iS, sS = _ints(np.asarray(samples, np.float64).reshape(-1, F))
    iF, sF = _ints(feats)
    p = _int_dot(iS, iF)
    aS, aF = _den_ints(iS, sS, normalized), _den_ints(iF, sF, False)
    for t in range(T):
        for d in range(D):
            best = None
            for r in range(int(off[t]), int(off[t + 1])):
                den = aS[r] * aF[d]
                num = den - (int(p[r, d]) << (2 * _K))  # (1 - cos) den
                num = min(max(num, 0), 2 * den)
                if best is None or num * best[1] < best[0] * den:
                    best = (num, den)
            if best is not None:
                out[t, d] = best[0] / best[1]  # int / int: correctly rounded
    return out


def nn_numpy(samples, off, feats):
    """The reference's own formula in numpy float64 (np.dot's order): [T, D]."""
    off = np.asarray(off)
    F = feats.shape[1]
    s = np.asarray(samples, np.float64).reshape(-1, F)
    sh = s / (np.linalg.norm(s, axis=1, keepdims=True) + 1e-8)
    fh = feats / (np.linalg.norm(feats, axis=1, keepdims=True) + 1e-8)
    out = np.full((off.shape[0] - 1, feats.shape[0]), INFTY_COST)
    for t in range(off.shape[0] - 1):
        if off[t + 1] > off[t]:
            out[t] = (1.0 - np.clip(sh[off[t]:off[t + 1]] @ fh.T, -1.0, 1.0)).min(0)
    return out


def np_normalise(x):
    """x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-8)."""
    return x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-8)


# ----------------------------------------------------------------------------- the fma chain
def fma_chain(a, b):
    """fma(a[k], b[k], acc) over ascending k from acc = 0.0, every step exact and rounded once."""
    acc = 0.0
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        if x == 0.0 or y == 0.0:
            acc = acc + x * y  # a signed zero product: exact in float64, and keeps the sign rule
        else:
            acc = float(Fraction(acc) + Fraction(x) * Fraction(y))
    return acc


def chain_entries(nd, nt):
    """The entries of an [nd, nt] output the fma chain is applied to: the corners of every
    32 x 64 output tile (cut to the matrix), the last row and the last column, and one whole row
    (the middle one).  Sorted (row, column) pairs."""
    pts = set()
    for d0 in range(0, nd, TILE_M):
        for t0 in range(0, nt, TILE_N):
            for r in (d0, min(d0 + TILE_M, nd) - 1):
                for c in (t0, min(t0 + TILE_N, nt) - 1):
                    pts.add((r, c))
    pts.update((nd - 1, c) for c in range(nt))
    pts.update((r, nt - 1) for r in range(nd))
    pts.update((nd // 2, c) for c in range(nt))
    return sorted(pts)


def chain_dot(D, T, pts):
    return np.array([fma_chain(D[r], T[c]) for r, c in pts])


# ------------------------------------------------------------------------------- bank mean
def bank_rows(bank_t, pushed):
    """The rows present in one track's ring [30, F] after `pushed` pushes, oldest first."""
    n = min(pushed, BANK)
    first = 0 if pushed < BANK else pushed % BANK
    return [bank_t[(first + k) % BANK] for k in range(n)]


def bank_mean_loop(rows):
    """s = v0; s += v_k; s / n in float64, per component."""
    s = np.array(rows[0], np.float64, copy=True)
    for v in rows[1:]:
        s = s + v
    return s / float(len(rows))


def bank_mean_fsum(rows):
    """(mean by math.fsum, sum of magnitudes) per component."""
    m = np.vstack(rows)
    mean = np.array([math.fsum(m[:, q].tolist()) / m.shape[0] for q in range(m.shape[1])])
    return mean, np.abs(m).sum(0)


def bank_mean_bound(mean, absum, n):
    """A sum of n terms in any order, then one division, on each side
    (tests/test_hybridsort_gpu.py::test_bank_mean_op)."""
    return 2 * (n * U * absum / n + U * np.abs(mean))


BANK_WIDTHS = [1, 63, 64, 65, 129]  # one lane, a wave less one, a wave, a wave plus one, three trips
BANK_PUSHED = [0, 1, 2, 29, 30, 31, 59, 60, 61]  # empty; partial; full; wrapped once and twice
BANK_NEGATIVE = [3, -1, 30, -30, 0, 61]


@functools.lru_cache(maxsize=None)
def bank_case(f, negative=False):
    """(bank [nt, 30, F], pushed [nt] int32): every track's ring filled by its own push sequence;
    rows never pushed stay NaN, so reading one shows.  A negative count leaves the ring NaN."""
    pushed = np.array(BANK_NEGATIVE if negative else BANK_PUSHED, np.int32)
    rng = _rng(10, f, int(negative))
    bank = np.full((pushed.shape[0], BANK, f), np.nan)
    for t, n in enumerate(pushed.tolist()):
        for k in range(max(n, 0)):
            bank[t, k % BANK] = entries(rng, 1, f)[0]
    return _frozen(bank, pushed)


# ------------------------------------------------------------------------- shared-tile cases
# F -> nk = ceil(F / 16) chunks through a pipeline of 4 in flight (register slot kc % 4), the A
# side staged in pairs and the B side in quads of k
TILE_WIDTHS = [1, 2, 3, 5,        # the row tail inside one thread's pair / quad
               15, 16, 17,        # one chunk and one more
               47, 48, 49,        # nk = 3 and 4
               63, 64, 65,        # the pipeline exactly full, one more
               81,                # nk = 6
               111, 112, 113,     # nk = 7 and 8
               129]               # nk = 9
TILE_SHAPES = [(1, 1), (31, 63), (32, 64), (33, 65), (1, 65), (33, 1), (65, 129)]
TILE_RUNS = ([((33, 65), f) for f in TILE_WIDTHS]
             + [(s, f) for f in (17, 113) for s in TILE_SHAPES if s != (33, 65)])
HOT_LOW = 7  # the existing test's hot index: min(F - 1, 7)


def tile_id(run):
    (nd, nt), f = run
    return f"{nd}x{nt}-F{f}"


@functools.lru_cache(maxsize=None)
def embcost_case(shape, f):
    """(D [nd, F], T [nt, F], hot): random rows; D's first row is one-hot at F - 1 and, with a
    second row, D's last row one-hot at min(F - 1, 7): hot = [(row, k), ...]."""
    nd, nt = shape
    rng = _rng(11, nd, nt, f)
    D, T = entries(rng, nd, f), entries(rng, nt, f)
    hot = [(0, f - 1)] + ([(nd - 1, min(f - 1, HOT_LOW))] if nd > 1 else [])
    for r, k in hot:
        D[r] = 0.0
        D[r, k] = 1.0
    return _frozen(D, T) + (hot,)


@functools.lru_cache(maxsize=None)
def embcost_expected(shape, f):
    """(exact D @ T.T, its bound, the chained entries, their fma-chain values)."""
    D, T, _ = embcost_case(shape, f)
    pts = chain_entries(*shape)
    return exact_dot(D, T), dot_bound(D, T), pts, chain_dot(D, T, pts)


def _pair_slots(nd, nt):
    """Up to eight (detection, track) slots spread over the matrix, no row or column twice."""
    n = min(nd, nt, 8)
    return [(int(r), int(c)) for r, c in zip(np.linspace(0, nd - 1, n).astype(int),
                                             np.linspace(0, nt - 1, n).astype(int))]


@functools.lru_cache(maxsize=None)
def cosdist_case(shape, f):
    """(D, T, parallel, anti): random rows; at up to eight (d, t) slots D[d] is a multiple of
    T[t] — positive at even slots (`parallel`), negative at odd ones (`anti`).  The multipliers
    are not powers of two, so the rounded cosine of such a pair lands on either side of 1."""
    nd, nt = shape
    rng = _rng(12, nd, nt, f)
    D, T = entries(rng, nd, f), entries(rng, nt, f)
    T = _clip(T, 1e-2, 1e2)  # so a multiple stays inside [1e-3, 1e3]
    par, anti = [], []
    for i, (r, c) in enumerate(_pair_slots(nd, nt)):
        lam = float(rng.uniform(0.3, 3.0))
        D[r] = T[c] * (-lam if i % 2 else lam)
        (anti if i % 2 else par).append((r, c))
    return _frozen(D, T) + (par, anti)


@functools.lru_cache(maxsize=None)
def cosdist_expected(shape, f):
    D, T, _, _ = cosdist_case(shape, f)
    return exact_cosdist(D, T), cosdist_bound(T, D)


def has_zero_rows_case(shape):
    return min(shape) > 8  # rows and columns besides the eight (anti)parallel slots


def cosdist_zero_rows(shape, f):
    """The case with one zero detection row (the last free one) and one zero track row (the
    first free one from the middle on), neither of them an (anti)parallel slot:
    (D, T, zero detection, zero track)."""
    D, T, par, anti = cosdist_case(shape, f)
    nd, nt = shape
    used_r, used_c = {r for r, _ in par + anti}, {c for _, c in par + anti}
    zd = next(r for r in range(nd - 1, -1, -1) if r not in used_r)
    zt = next(c for c in range(nt // 2, nt) if c not in used_c)
    D, T = D.copy(), T.copy()
    D[zd] = 0.0
    T[zt] = 0.0
    return D, T, zd, zt


CLAMP_N = 48


@functools.lru_cache(maxsize=None)
def cosdist_clamp_case():
    """(D [48, 2], T [48, 2]): D[i] is a multiple of T[i], positive for even i and negative for
    odd i (`clamp_case_cosines` gives the rounded cosine of each such pair)."""
    rng = _rng(13)
    T = _clip(entries(rng, CLAMP_N, 2), 1e-2, 1e2)
    lam = rng.uniform(0.3, 3.0, CLAMP_N) * np.where(np.arange(CLAMP_N) % 2, -1.0, 1.0)
    return _frozen(T * lam[:, None], T)


@functools.lru_cache(maxsize=None)
def clamp_case_cosines():
    D, T = cosdist_clamp_case()
    return _frozen(np.array([rounded_cosine_small(d, t) for d, t in zip(D, T)]))


def rounded_cosine_small(d, t):
    """The cosine as any float64 evaluation of d.t / (|d| |t|) rounds it when F <= 2: the fma
    chain over the one or two products, each norm the square root of the one possible sum.  With
    one or two terms there is no summation order to choose, and product, sum, square root and
    division are correctly rounded everywhere, so this is what the kernel must hold before its
    clamp."""
    assert d.shape[0] <= 2
    nd = math.sqrt(float(np.sum(d * d)))
    nt = math.sqrt(float(np.sum(t * t)))
    return fma_chain(d, t) / (nd * nt)


# ------------------------------------------------------------------ nearest-neighbour cases
NN_NORM_WIDTHS = [1, 7, 8, 9, 127, 128, 129, 136, 137, 255, 256, 257, 264, 1000, 4099, 8191, 8192]
NN_NORM_COUNTS = [1, 4, 2, 3, 4]  # T = 5, up to 4 samples per target
NN_NORM_D = 9
NN_F_MAX = 8192
NN_TILE_F = [17, 64]
NN_TILE_G = [63, 64, 65, 129]
NN_TILE_D = [1, 63, 64, 65, 257]


def offsets(counts):
    return _frozen(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))


def pairwise_leaves(n):
    """The leaf lengths of numpy's pairwise sum over n elements, in element order."""
    if n <= 128:
        return [n]
    h = n // 2
    h -= h % 8
    return pairwise_leaves(h) + pairwise_leaves(n - h)


@functools.lru_cache(maxsize=None)
def nn_norm_case(f):
    """(samples [14, F], off [6], feats [9, F])."""
    rng = _rng(20, f)
    s, x = entries(rng, sum(NN_NORM_COUNTS), f), entries(rng, NN_NORM_D, f)
    return _frozen(s), offsets(NN_NORM_COUNTS), _frozen(x)


@functools.lru_cache(maxsize=None)
def nn_onehot_case(f, side):
    """The case that shows a row denominator in the distance.  side "feats": every target holds
    one sample scale * e_j (j spread over the width) against general features, so
    dist[t, d] = 1 - ŝ_j * f̂[d, j] shows f[d, j] / den(f[d]) for several j; side "samples": the
    features are the one-hot rows and every target holds one general sample."""
    rng = _rng(21, f, side == "feats")
    n = min(f, 6)
    hot = np.unique(np.linspace(0, f - 1, n).astype(int))
    one = np.zeros((hot.shape[0], f))
    one[np.arange(hot.shape[0]), hot] = rng.uniform(0.5, 40.0, hot.shape[0])
    gen = entries(rng, NN_NORM_D, f)
    if side == "feats":
        return _frozen(one), offsets(np.ones(hot.shape[0], int)), _frozen(gen), hot
    return _frozen(gen), offsets(np.ones(NN_NORM_D, int)), _frozen(one), hot


def _ragged(rng, total, most):
    """Counts in [1, most] summing to `total`."""
    cnt = []
    while sum(cnt) < total:
        cnt.append(int(min(rng.integers(1, most + 1), total - sum(cnt))))
    return cnt


def _gallery(rng, counts, d, f):
    """Samples near their target's base direction, features near some target's."""
    counts = np.asarray(counts)
    base = rng.standard_normal((counts.shape[0], f))
    g = int(counts.sum())
    s = np.repeat(base, counts, 0) + 0.5 * rng.standard_normal((g, f))
    s *= 10.0 ** rng.uniform(-1, 1, (g, 1))
    x = base[rng.integers(0, counts.shape[0], d)] + 0.5 * rng.standard_normal((d, f))
    x *= 10.0 ** rng.uniform(-1, 1, (d, 1))
    return _clip(s), _clip(x)


@functools.lru_cache(maxsize=None)
def nn_grid_case(g, f):
    """(samples [G, F], off, feats [257, F]): G rows in ragged targets of 1..9 samples; a run at
    D detections takes the first D feature rows."""
    rng = _rng(22, g, f)
    cnt = _ragged(rng, g, 9)
    s, x = _gallery(rng, cnt, max(NN_TILE_D), f)
    return _frozen(s), offsets(cnt), _frozen(x)


NN_KINDS = ["singles", "spanning", "empties", "no_samples", "anticorrelated", "signed_zero",
            "match_and_negation", "zero_rows"]


@functools.lru_cache(maxsize=None)
def nn_kind_case(kind, f):
    """(samples or None, off, feats) of one designated case (NN_KINDS):

    singles             70 targets of one sample each: runs of length 1 inside a lane's rows,
                        over two row blocks
    spanning            targets of 10, 20, 200 and 15 samples: the third starts at row 30 and
                        runs through four 64-row blocks, whose workgroups meet in its keys
    empties             counts 0, 5, 0, 0, 70, 3, 0: empty targets first, in the middle and last
    no_samples          four empty targets, G = 0, no sample array at all
    anticorrelated      every feature is near +v; target 0's samples are near -v (every dot
                        negative), target 1's near +v, target 2 mixes both
    signed_zero         features on the even components, samples on the odd ones.  target 0:
                        positive entries (every product +0); target 1: negative entries (every
                        product -0; the chain from +0.0 still ends at +0, see the host test);
                        target 2: a sample with a negative dot only; target 3: all three kinds
    match_and_negation  target 0 holds feature 0's row times 2, target 1 its negation times 3
    zero_rows           target 1's only sample is zero, target 2 holds a zero row among others;
                        feature 3 is zero
    """
    rng = _rng(23, NN_KINDS.index(kind), f)
    d = 33
    if kind == "singles":
        cnt = [1] * 70
        s, x = _gallery(rng, cnt, d, f)
    elif kind == "spanning":
        cnt = [10, 20, 200, 15]
        s, x = _gallery(rng, cnt, d, f)
    elif kind == "empties":
        cnt = [0, 5, 0, 0, 70, 3, 0]
        s, x = _gallery(rng, cnt, d, f)
    elif kind == "no_samples":
        cnt, s, x = [0, 0, 0, 0], None, entries(rng, 7, f)
    elif kind == "anticorrelated":
        cnt = [40, 30, 8]
        v = entries(rng, 1, f)
        noise = lambda n: 0.05 * np.abs(v) * rng.standard_normal((n, f))  # noqa: E731
        x = (v + noise(d)) * rng.uniform(0.5, 2.0, (d, 1))
        sign = np.concatenate([-np.ones(40), np.ones(30), [-1, 1] * 4])[:, None]
        s = sign * (v + noise(78)) * rng.uniform(0.5, 2.0, (78, 1))
        s, x = _clip(s), _clip(x)
    elif kind == "signed_zero":
        cnt = [3, 3, 2, 4]
        even = (np.arange(f) % 2 == 0)
        x = np.abs(entries(rng, d, f)) * even
        odd = lambda n, sg: sg * np.abs(entries(rng, n, f)) * ~even  # noqa: E731
        neg = lambda n: -np.abs(entries(rng, n, f)) * even  # noqa: E731
        s = np.concatenate([odd(3, 1.0), odd(3, -1.0), neg(2), odd(1, 1.0), odd(1, -1.0), neg(2)])
    elif kind == "match_and_negation":
        cnt = [1, 1, 6]
        s, x = _gallery(rng, cnt, d, f)
        x = _clip(x, 1e-2, 1e2)
        s[0], s[1] = 2.0 * x[0], -3.0 * x[0]
    elif kind == "zero_rows":
        cnt = [4, 1, 5]
        s, x = _gallery(rng, cnt, d, f)
        s[4] = 0.0
        s[7] = 0.0
        x[3] = 0.0
    else:
        raise KeyError(kind)
    return (None if s is None else _frozen(s)), offsets(cnt), _frozen(x)


@functools.lru_cache(maxsize=None)
def nn_clip_case(f):
    """(samples [2, F], off, feats [33, F]) for a run with BX_NN_SAMPLES_NORMALIZED: the samples
    are feature 0's normalised row times 2 and times -2, so their dots with feature 0 are about
    2 and -2 and the clip decides: distances exactly 0 and 2.  (With samples the op normalises
    itself, |ŝ| = |s| / (|s| + 1e-8) < 1 keeps an exact match a few 1e-9 / |s| short of the clip
    at any |s| below 1e8 2^-27: tests/test_emb_edges_host.py shows it.)"""
    _, _, x = nn_kind_case("match_and_negation", f)
    xh = np_normalise(x[:1])
    return _frozen(np.concatenate([2.0 * xh, -2.0 * xh])), offsets([1, 1]), x


BIG_G, BIG_T, BIG_D, BIG_F = 128 * 128, 300, 300, 17
BIG_BM, BIG_BN = 128, 256  # the large tile: sample rows x detections


def big_tile_blocks(g, d):
    """Workgroups of the 128 x 256 tile; the op takes it when this reaches the CU count."""
    return -(-g // BIG_BM) * -(-d // BIG_BN)


@functools.lru_cache(maxsize=None)
def nn_big_case(cut):
    """(samples [G, 17], off [301], feats [D, 17]) with G = 16384 - cut rows in 300 ragged
    targets (some of them empty) and D = 300 - cut."""
    rng = _rng(24)
    g, d = BIG_G - cut, BIG_D - cut
    w = rng.dirichlet(np.full(BIG_T, 0.7))
    cnt = rng.multinomial(g, w)
    cnt[[0, 150]] = 0
    cnt[299] += g - cnt.sum()
    s, x = _gallery(rng, cnt, d, BIG_F)
    return _frozen(s), offsets(cnt), _frozen(x)

"""The reference side of the appearance-distance edge cases, on the CPU.

tests/emb_ref.py holds the cases tests/test_emb_edges_gpu.py runs on the device and three
references for them.  Here the references are checked against each other, against numpy and
against the C oracle, so that the GPU test compares the kernels with something that was itself
checked: the Fraction fma chain equals the oracle's contraction bit for bit, the float64
bank-mean loop equals numpy's mean(0) bit for bit, the oracle's row denominators equal numpy's
bit for bit at every norm width, and the exact references agree with numpy within the bounds the
GPU test uses.  Every designated case is shown to reach what it was built for.
"""
import struct

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import emb_ref as E


def bits(v):
    return struct.pack("<d", float(v))


# ------------------------------------------------------------------------------ the fma chain
@pytest.mark.parametrize("f", [17, 64, 129])
def test_fma_chain_equals_oracle_contraction(f):
    """Unit rows in: the oracle divides them by |x| + 1e-8 once more (numpy's own division, whose
    denominators test_oracle_denominators_equal_numpy pins) and contracts; the Fraction chain over
    the same rows, through 1 - clip and the minimum over a target's samples, gives the same bits."""
    s, off, x = E.nn_norm_case(f)
    s, x = E.np_normalise(s), E.np_normalise(x)
    a, b = E.np_normalise(s), E.np_normalise(x)
    want = np.empty((off.shape[0] - 1, x.shape[0]))
    for t in range(want.shape[0]):
        for d in range(want.shape[1]):
            dots = [E.fma_chain(a[r], b[d]) for r in range(off[t], off[t + 1])]
            want[t, d] = min(1.0 - min(max(c, -1.0), 1.0) for c in dots)
    got = po.nn_cosine_distance(s, off, x)
    assert np.isfinite(want).all() and (want > 0).all()
    np.testing.assert_array_equal(got, want)


def test_fma_chain_is_a_fused_chain():
    """One rounding per step: 1 + 2^-30 squared minus 1 keeps the 2^-60 term an unfused product
    would drop, and a chain of -0 products started at +0.0 ends at +0."""
    x = 1.0 + 2.0 ** -30
    assert E.fma_chain([1.0, x], [-1.0, x]) == 2.0 ** -29 + 2.0 ** -60
    assert (x * x) - 1.0 == 2.0 ** -29
    z = E.fma_chain([-3.0, 0.0, -0.5], [0.0, 7.0, 0.0])
    assert bits(z) == bits(0.0) and bits(z) != bits(-0.0)


def test_chain_entries_cover_what_is_listed():
    pts = E.chain_entries(65, 129)
    assert len(set(pts)) == len(pts)
    for p in [(0, 0), (31, 63), (32, 64), (63, 127), (64, 128), (64, 0), (0, 128), (31, 128)]:
        assert p in pts  # corners of the nine tiles, the last one cut to 1 x 1
    assert all((64, c) in pts and (32, c) in pts for c in range(129))
    assert all((r, 128) in pts for r in range(65))
    assert E.chain_entries(1, 1) == [(0, 0)]


# ----------------------------------------------------------------------------- exact references
@pytest.mark.parametrize("run", E.TILE_RUNS, ids=E.tile_id)
def test_tile_cases(run):
    """The embcost and cosdist cases of one run: in range, finite where asserted finite; numpy's
    own float64 results lie within the bounds of the exact references; the chain lies within the
    dot bound of the exact dot and equals the column for a one-hot row; the zero-row case has NaN
    in exactly one row and one column."""
    shape, f = run
    D, T, hot = E.embcost_case(shape, f)
    exact, bound, pts, chain = E.embcost_expected(shape, f)
    assert D.shape == (shape[0], f) and T.shape == (shape[1], f) and E.in_range(D) and E.in_range(T)
    assert np.isfinite(exact).all() and (np.abs(D @ T.T - exact) <= bound).all()
    rows, cols = np.array(pts).T
    assert (np.abs(chain - exact[rows, cols]) <= bound[rows, cols]).all()
    for r, k in hot:
        np.testing.assert_array_equal(exact[r], T[:, k])
        assert all(chain[i] == T[c, k] for i, (rr, c) in enumerate(pts) if rr == r)
    assert hot[0] == (0, f - 1)

    D, T, par, anti = E.cosdist_case(shape, f)
    exact, bound = E.cosdist_expected(shape, f)
    assert E.in_range(D) and E.in_range(T)
    assert np.isfinite(exact).all() and (exact >= 0).all() and (exact <= 2).all()
    assert (np.abs(E.cosdist_ref(T, D) - exact) <= bound).all()
    # (a rounded multiple is parallel to 2^-53: an exact distance of some 1e-32, not of 0)
    assert par and all(exact[p] < 1e-30 for p in par)
    assert all(exact[p] == 2.0 for p in anti) and (len(anti) > 0 or min(shape) == 1)
    if E.has_zero_rows_case(shape):
        Dz, Tz, zd, zt = E.cosdist_zero_rows(shape, f)
        nan = np.zeros(shape, bool)
        nan[zd, :] = True
        nan[:, zt] = True
        np.testing.assert_array_equal(np.isnan(E.exact_cosdist(Dz, Tz)), nan)
        np.testing.assert_array_equal(np.isnan(E.cosdist_ref(Tz, Dz)), nan)
        keep = ~nan
        np.testing.assert_array_equal(E.exact_cosdist(Dz, Tz)[keep], exact[keep])


def test_rounded_cosine_passes_one_at_width_two():
    """At F = 2 a float64 evaluation of the cosine has no summation order to choose.  Among the
    48 (anti)parallel pairs of the clamp case the rounded cosine lands above 1 for some and below
    -1 for others: the pairs the clamp is for, whose distances must be exactly 0 and 2.  The
    excess is one ulp of 1, and 1 - (-1 - 2^-52) rounds to 2 by itself, as max(0, .) catches the
    other side: the outputs pin the clamped result, they cannot tell which step produced it.
    (At F = 1 sqrt(x * x) is |x| and the rounded cosine is exactly 1 or -1 for every pair.)"""
    D, T = E.cosdist_clamp_case()
    assert E.in_range(D) and E.in_range(T)
    c = E.clamp_case_cosines()
    assert (c > 1.0).sum() >= 3 and (c < -1.0).sum() >= 3 and (np.abs(c) <= 1.0).sum() >= 3
    assert (np.abs(c) <= 1.0 + 2.0 ** -52).all()
    D1, T1, _, _ = E.cosdist_case((33, 65), 1)
    assert all(abs(E.rounded_cosine_small(d, t)) == 1.0 for d in D1[:8] for t in T1[:8])


# ------------------------------------------------------------------------------- bank mean
@pytest.mark.parametrize("f", E.BANK_WIDTHS)
def test_bank_mean_loop_is_numpys_mean(f):
    bank, pushed = E.bank_case(f)
    assert pushed.tolist() == E.BANK_PUSHED
    for t, n in enumerate(pushed.tolist()):
        present = np.isfinite(bank[t]).all(1)
        assert present.sum() == min(n, E.BANK) and np.isnan(bank[t][~present]).all()
        if n <= 0:
            continue
        rows = E.bank_rows(bank[t], n)
        assert len(rows) == min(n, E.BANK) and E.in_range(np.vstack(rows))
        loop = E.bank_mean_loop(rows)
        if f > 1:
            np.testing.assert_array_equal(loop, np.vstack(rows).mean(0))
        else:
            # a finding about numpy, not papered over: mean(0) of an [n, 1] array reduces one
            # contiguous run, which numpy sums pairwise (eight accumulators from 8 elements on),
            # so at F = 1 it leaves the oldest-first order the reference's wider banks get.  The
            # same column inside an [n, 2] array is summed row by row: that order is the loop's.
            two = np.repeat(np.vstack(rows), 2, axis=1)
            np.testing.assert_array_equal(loop, two.mean(0)[:1])
            if len(rows) < 8:
                np.testing.assert_array_equal(loop, np.vstack(rows).mean(0))
        mean, absum = E.bank_mean_fsum(rows)
        assert (np.abs(loop - mean) <= E.bank_mean_bound(mean, absum, len(rows))).all()
    neg, cnt = E.bank_case(f, negative=True)
    assert (cnt < 0).sum() == 2 and np.isnan(neg[cnt <= 0]).all()


def test_bank_rows_follow_a_deque():
    """Oldest first, through the wrap: the ring after 61 pushes holds pushes 31..60."""
    from collections import deque

    ring = np.full((E.BANK, 1), np.nan)
    dq = deque(maxlen=E.BANK)
    for k in range(61):
        ring[k % E.BANK] = float(k)
        dq.append(float(k))
        got = [float(r[0]) for r in E.bank_rows(ring, k + 1)]
        assert got == list(dq)


# ------------------------------------------------------------------------------ row norms
def test_norm_widths_reach_the_pairwise_branches():
    """What the widths were chosen for, from numpy's own halving rule."""
    leaves = {f: E.pairwise_leaves(f) for f in E.NN_NORM_WIDTHS}
    assert all(sum(v) == f and max(v) <= 128 for f, v in leaves.items())
    assert leaves[1] == [1] and leaves[7] == [7]  # the loop below 8 elements
    assert leaves[9] == [9] and leaves[127] == [127]  # 8-lane leaves with a tail of 1 and of 7
    assert leaves[128] == [128] and leaves[129] == [64, 65] and leaves[136] == [64, 72]
    assert leaves[137] == [64, 73] and leaves[255] == [120, 64, 71]
    assert leaves[257] == [128, 64, 65] and leaves[264] == [128, 64, 72]
    assert set(leaves[1000]) == {120, 128}  # uneven splits
    for f in (4099, 8191):  # uneven splits and a leaf with a tail
        assert len(set(leaves[f])) > 1 and any(m % 8 for m in leaves[f])
    assert leaves[8192] == [128] * 64 and E.NN_F_MAX == 8192


@pytest.mark.parametrize("f", E.NN_NORM_WIDTHS)
def test_oracle_norm_widths_against_numpy(f):
    s, off, x = E.nn_norm_case(f)
    assert E.in_range(s) and E.in_range(x) and off[-1] == s.shape[0] == 14 and x.shape[0] == 9
    got = po.nn_cosine_distance(s, off, x)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, E.nn_numpy(s, off, x), rtol=0, atol=E.NN_ATOL)
    if f <= 1000:  # (the exact side of the widest rows takes seconds and adds nothing here)
        np.testing.assert_allclose(got, E.exact_nn(s, off, x), rtol=0, atol=E.NN_ATOL)


@pytest.mark.parametrize("side", ["feats", "samples"])
@pytest.mark.parametrize("f", E.NN_NORM_WIDTHS)
def test_oracle_denominators_equal_numpy(f, side):
    """One side one-hot rows scale * e_j: dist = 1 - clip(ŝ[j] * f̂[j]) is a single product, so
    with numpy's own x / (np.linalg.norm(x) + 1e-8) on both sides the distance is known to the
    bit, and equal bits at several j of every general row mean equal denominators."""
    s, off, x, hot = E.nn_onehot_case(f, side)
    sh, xh = E.np_normalise(s), E.np_normalise(x)
    if side == "feats":
        want = 1.0 - np.clip(sh[np.arange(hot.shape[0]), hot][:, None] * xh[:, hot].T, -1.0, 1.0)
    else:
        want = 1.0 - np.clip(sh[:, hot] * xh[np.arange(hot.shape[0]), hot][None, :], -1.0, 1.0)
    got = po.nn_cosine_distance(s, off, x)
    assert got.shape == want.shape and (want != 1.0).all()
    np.testing.assert_array_equal(got, want)


# --------------------------------------------------------------------- tiles and the key order
def check_nn(s, off, x):
    """The oracle within 1e-13 of the exact reference and of numpy; returns (oracle, exact)."""
    got = po.nn_cosine_distance(np.zeros((0, x.shape[1])) if s is None else s, off, x)
    exact = E.exact_nn(s, off, x)
    np.testing.assert_allclose(got, exact, rtol=0, atol=E.NN_ATOL)
    np.testing.assert_allclose(got, E.nn_numpy(np.zeros((0, x.shape[1])) if s is None else s,
                                               off, x), rtol=0, atol=E.NN_ATOL)
    return got, exact


@pytest.mark.parametrize("f", E.NN_TILE_F)
@pytest.mark.parametrize("g", E.NN_TILE_G)
def test_nn_grid_cases(g, f):
    s, off, x = E.nn_grid_case(g, f)
    assert s.shape == (g, f) and off[-1] == g and x.shape == (257, f)
    assert E.in_range(s) and E.in_range(x) and (np.diff(off) >= 1).all()
    got, _ = check_nn(s, off, x)
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 2).all()


@pytest.mark.parametrize("f", E.NN_TILE_F)
@pytest.mark.parametrize("kind", E.NN_KINDS)
def test_nn_designated_cases(kind, f):
    s, off, x = E.nn_kind_case(kind, f)
    cnt = np.diff(off)
    assert E.in_range(x) and (s is None or (E.in_range(s) and s.shape == (off[-1], f)))
    got, exact = check_nn(s, off, x)
    assert (got[cnt == 0] == E.INFTY_COST).all() and (exact[cnt == 0] == E.INFTY_COST).all()
    assert (got[cnt > 0] >= 0).all() and (got[cnt > 0] <= 2).all()
    if kind == "singles":
        assert (cnt == 1).all() and cnt.shape[0] == 70
    if kind == "spanning":
        assert off[2] == 30 and cnt[2] == 200
    if kind == "empties":
        assert cnt[0] == 0 and cnt[-1] == 0 and (cnt[2:4] == 0).all() and cnt[4] > 64
    if kind == "no_samples":
        assert s is None and off[-1] == 0 and (got == E.INFTY_COST).all()
    if kind == "anticorrelated":  # the best dot of target 0 is negative for every detection
        assert (exact[0] > 1.5).all() and (exact[1] < 0.5).all() and (exact[2] < 0.5).all()
    if kind == "signed_zero":
        for t in (0, 1, 3):
            assert (got[t] == 1.0).all() and (exact[t] == 1.0).all()
        assert (exact[2] > 1.0).all()
        # every product of target 1 is -0; the chain from +0.0 gives +0
        prods = E.np_normalise(s)[3] * E.np_normalise(x)[0]
        assert all(bits(p) == bits(-0.0) for p in prods)
        assert bits(E.fma_chain(E.np_normalise(s)[3], E.np_normalise(x)[0])) == bits(0.0)
    if kind == "match_and_negation":
        # |ŝ| < 1: an exact match stays short of the clip (emb_ref.nn_clip_case reaches it)
        assert 0.0 < exact[0, 0] < 1e-7 and 2.0 - 1e-7 < exact[1, 0] < 2.0
        assert 0.0 < got[0, 0] < 1e-7 and 2.0 - 1e-7 < got[1, 0] < 2.0
    if kind == "zero_rows":
        assert (got[1] == 1.0).all() and (exact[1] == 1.0).all()
        assert (got[:, 3] == 1.0).all() and (exact[:, 3] == 1.0).all()
        assert (exact[2] <= 1.0).all()  # the zero row among others offers a dot of 0


@pytest.mark.parametrize("f", E.NN_TILE_F)
def test_nn_clip_case(f):
    s, off, x = E.nn_clip_case(f)
    exact = E.exact_nn(s, off, x, normalized=True)
    assert exact[0, 0] == 0.0 and exact[1, 0] == 2.0
    assert ((exact > 0) & (exact < 2)).sum() > 0  # other detections stay inside the clip
    # the float64 evaluation agrees: the dot with feature 0 passes 1 in magnitude
    dots = s @ E.np_normalise(x).T
    assert dots[0, 0] > 1.5 and dots[1, 0] < -1.5


@pytest.mark.parametrize("cut", [0, 1])
def test_nn_big_case(cut):
    """The 128 x 256 tile's case qualifies on a device of up to 256 CUs, cut by one as well, and
    the oracle is within 1e-13 of numpy's own formula on it."""
    s, off, x = E.nn_big_case(cut)
    g, d = E.BIG_G - cut, E.BIG_D - cut
    assert s.shape == (g, E.BIG_F) and x.shape == (d, E.BIG_F) and off.shape == (E.BIG_T + 1,)
    assert off[-1] == g and (np.diff(off) >= 0).all() and (np.diff(off) == 0).sum() >= 2
    assert E.in_range(s) and E.in_range(x) and s.nbytes < 3 << 20
    assert E.big_tile_blocks(g, d) == 256
    assert (g % E.BIG_BM != 0) == bool(cut) and d % E.BIG_BN != 0
    got = po.nn_cosine_distance(s, off, x)
    np.testing.assert_allclose(got, E.nn_numpy(s, off, x), rtol=0, atol=E.NN_ATOL)

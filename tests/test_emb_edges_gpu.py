"""The appearance-distance HIP ops at pipeline, tile and norm edges: bx_deepoc_embcost and
bx_hybrid_cosdist (the shared MFMA tile of bx_embtile.h), bx_hybrid_bank_mean and
bx_nn_cosine_distance, and BoostTrack's use of the tile inside its engine.

Every case and reference comes from tests/emb_ref.py, whose reference side
tests/test_emb_edges_host.py checks on the CPU.  Every output lives between 64 leading and 64
trailing sentinel elements that must survive the call (tests/test_ops_edges_gpu.py's Guarded).
No tolerance here is new: the dot bound 2 F 2^-53 (|D| @ |T|.T), emb_ref.cosdist_bound, the bank
mean's bound of tests/test_hybridsort_gpu.py and atol 1e-13 for the nearest-neighbour distance;
everything else is bit for bit.
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import emb_ref as E
from tests.test_ops_edges_gpu import BX_ERR_INVALID, BX_OK, SENTINEL, Guarded, dev, ok

pytestmark = pytest.mark.gpu

BX_NN_SAMPLES_NORMALIZED = 1


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()  # must be the in-tree HIP library, never a fallback
    return torch


@pytest.fixture(scope="module")
def lib(torch_cuda):
    from boxmot_amd import _native

    return _native.load()


def nan_output(torch, shape):
    return Guarded(torch, shape, init=np.full(shape, np.nan))


# ------------------------------------------------------------- 1. the shared tile, as ops
def run_tile_op(torch, fn, D, T):
    out = nan_output(torch, (D.shape[0], T.shape[0]))
    dd, td = dev(torch, D), dev(torch, T)
    ok(fn(D.shape[0], T.shape[0], D.shape[1], dd.data_ptr(), td.data_ptr(), out.ptr, None))
    return out.get()


@pytest.mark.parametrize("run", E.TILE_RUNS, ids=E.tile_id)
def test_embcost_tile_edges(torch_cuda, lib, run):
    """Within the dot bound of the exact product everywhere (an unwritten entry would still be
    NaN); bit for bit the ascending-k fma chain on the corners of every output tile, the last
    row, the last column and one whole row; a one-hot row (hot at F - 1, and at min(F - 1, 7))
    returns the column exactly."""
    shape, f = run
    D, T, hot = E.embcost_case(shape, f)
    exact, bound, pts, chain = E.embcost_expected(shape, f)
    got = run_tile_op(torch_cuda, lib.bx_deepoc_embcost, D, T)
    err = np.abs(got - exact)
    print(f"embcost {E.tile_id(run)}: max err {np.nanmax(err):.3e}, "
          f"min slack {np.nanmin(bound - err):.3e}")
    assert np.isfinite(got).all() and (err <= bound).all()
    rows, cols = np.array(pts).T
    np.testing.assert_array_equal(got[rows, cols], chain)
    for r, k in hot:
        np.testing.assert_array_equal(got[r], T[:, k])


@pytest.mark.parametrize("run", E.TILE_RUNS, ids=E.tile_id)
def test_cosdist_tile_edges(torch_cuda, lib, run):
    """Within cosdist_bound of the exact distance, never negative; a parallel pair within its
    bound of 0, an antiparallel pair within its bound of 2 and never above 2; a zero detection
    row and a zero track row give NaN in exactly that row and column, and every other entry
    keeps its bits."""
    shape, f = run
    D, T, par, anti = E.cosdist_case(shape, f)
    exact, bound = E.cosdist_expected(shape, f)
    got = run_tile_op(torch_cuda, lib.bx_hybrid_cosdist, D, T)
    err = np.abs(got - exact)
    print(f"cosdist {E.tile_id(run)}: max err {np.nanmax(err):.3e}, "
          f"min slack {np.nanmin(bound - err):.3e}")
    assert np.isfinite(got).all() and (err <= bound).all()
    assert (got >= 0.0).all() and (got <= 2.0).all()
    for p in par:
        assert got[p] <= bound[p]
    for p in anti:
        assert 2.0 - got[p] <= bound[p]
    if E.has_zero_rows_case(shape):
        Dz, Tz, zd, zt = E.cosdist_zero_rows(shape, f)
        gz = run_tile_op(torch_cuda, lib.bx_hybrid_cosdist, Dz, Tz)
        nan = np.zeros(shape, bool)
        nan[zd, :] = True
        nan[:, zt] = True
        np.testing.assert_array_equal(np.isnan(gz), nan)
        np.testing.assert_array_equal(gz[~nan], got[~nan])


def test_cosdist_clamps_a_rounded_cosine_past_one(torch_cuda, lib):
    """48 (anti)parallel pairs at F = 2, where the float64 cosine has one possible evaluation
    (emb_ref.rounded_cosine_small): where it rounds above 1 the distance is exactly 0, where it
    rounds below -1 exactly 2, elsewhere exactly max(0, 1 - c)."""
    D, T = E.cosdist_clamp_case()
    c = E.clamp_case_cosines()
    got = run_tile_op(torch_cuda, lib.bx_hybrid_cosdist, D, T)
    assert (got >= 0.0).all() and (got <= 2.0).all()
    diag = np.diagonal(got)
    assert (c > 1.0).any() and (c < -1.0).any()
    np.testing.assert_array_equal(diag[c > 1.0], 0.0)
    np.testing.assert_array_equal(diag[c < -1.0], 2.0)
    inside = np.abs(c) <= 1.0
    np.testing.assert_array_equal(diag[inside], np.maximum(0.0, 1.0 - c[inside]))


# ------------------------------------------------------------------------ 2. the bank mean
@pytest.mark.parametrize("negative", [False, True], ids=["counts", "negative"])
@pytest.mark.parametrize("f", E.BANK_WIDTHS)
def test_bank_mean_edges(torch_cuda, lib, f, negative):
    """One call over tracks pushed 0, 1, 2, 29, 30, 31, 59, 60 and 61 times (and one with
    negative counts): bit for bit the oldest-first float64 loop, within the existing bound of the
    fsum mean; never-pushed ring rows are NaN and must not be read; rows with pushed <= 0 keep
    their sentinel."""
    torch = torch_cuda
    bank, pushed = E.bank_case(f, negative)
    nt = pushed.shape[0]
    out = Guarded(torch, (nt, f))
    bd, pd = dev(torch, bank), dev(torch, pushed)
    ok(lib.bx_hybrid_bank_mean(nt, f, bd.data_ptr(), pd.data_ptr(), out.ptr, None))
    got = out.get()
    assert (pushed <= 0).sum() >= 1
    for t, n in enumerate(pushed.tolist()):
        if n <= 0:
            assert (got[t] == SENTINEL).all(), f"track {t} pushed {n}: written"
            continue
        rows = E.bank_rows(bank[t], n)
        np.testing.assert_array_equal(got[t], E.bank_mean_loop(rows), err_msg=f"pushed {n}")
        mean, absum = E.bank_mean_fsum(rows)
        assert (np.abs(got[t] - mean) <= E.bank_mean_bound(mean, absum, len(rows))).all()


# --------------------------------------------------- 3. nearest neighbour: the row norms
def run_nn(torch, lib, s, off, x, flags=0):
    T, (D, F) = off.shape[0] - 1, x.shape
    out = Guarded(torch, (T, D))
    sd = None if s is None else dev(torch, s)
    od, xd = dev(torch, off), dev(torch, x)
    ok(lib.bx_nn_cosine_distance(None if sd is None else sd.data_ptr(), int(off[-1]),
                                 od.data_ptr(), T, xd.data_ptr(), D, F, flags, out.ptr, None))
    return out.get()


@pytest.mark.parametrize("f", E.NN_NORM_WIDTHS)
def test_nn_norm_widths(torch_cuda, lib, f):
    """Bit for bit the oracle (whose denominators the host test holds to numpy's bit for bit)
    and within 1e-13 of numpy; the run on samples normalised beforehand equals the plain run bit
    for bit, which holds the device norm and scale kernels alone to numpy's
    x / (norm + 1e-8)."""
    s, off, x = E.nn_norm_case(f)
    got = run_nn(torch_cuda, lib, s, off, x)
    np.testing.assert_array_equal(got, po.nn_cosine_distance(s, off, x))
    np.testing.assert_allclose(got, E.nn_numpy(s, off, x), rtol=0, atol=E.NN_ATOL)
    pre = run_nn(torch_cuda, lib, E.np_normalise(s), off, x, BX_NN_SAMPLES_NORMALIZED)
    np.testing.assert_array_equal(pre, got)


@pytest.mark.parametrize("side", ["feats", "samples"])
@pytest.mark.parametrize("f", [1, 9, 129, 137, 264, 4099])
def test_nn_denominators_through_one_hot_rows(torch_cuda, lib, f, side):
    """The host test's observation of the row denominators, on the device."""
    s, off, x, _ = E.nn_onehot_case(f, side)
    np.testing.assert_array_equal(run_nn(torch_cuda, lib, s, off, x),
                                  po.nn_cosine_distance(s, off, x))


# ---------------------------------------- 4. nearest neighbour: tiles and the key order
@functools.lru_cache(maxsize=None)
def nn_expected(kind, f):
    """(oracle, exact) of a grid case (kind = G) or a designated one, computed once."""
    s, off, x = E.nn_grid_case(kind, f) if isinstance(kind, int) else E.nn_kind_case(kind, f)
    orc = po.nn_cosine_distance(np.zeros((0, f)) if s is None else s, off, x)
    return orc, E.exact_nn(s, off, x)


@pytest.mark.parametrize("f", E.NN_TILE_F)
@pytest.mark.parametrize("g", E.NN_TILE_G)
def test_nn_small_tile_edges(torch_cuda, lib, g, f):
    """G in {63, 64, 65, 129} sample rows in ragged targets against D in {1, 63, 64, 65, 257}
    detections: one row or column short of the 64 x 64 tile, exactly it, one past it, and a
    third row block / fifth column block of one row / column."""
    s, off, x = E.nn_grid_case(g, f)
    orc, exact = nn_expected(g, f)
    for d in E.NN_TILE_D:
        got = run_nn(torch_cuda, lib, s, off, x[:d])
        np.testing.assert_array_equal(got, orc[:, :d], err_msg=f"D = {d}")
        np.testing.assert_allclose(got, exact[:, :d], rtol=0, atol=E.NN_ATOL)


@pytest.mark.parametrize("f", E.NN_TILE_F)
@pytest.mark.parametrize("kind", E.NN_KINDS)
def test_nn_designated_cases(torch_cuda, lib, kind, f):
    """emb_ref.nn_kind_case: runs of one-sample targets, a target across four row blocks, empty
    targets, no samples at all, a maximum among negative dots, dots of exactly zero against a
    negative one, a match and its negation, zero rows.  Bit for bit the oracle, within 1e-13 of
    the exact reference, and the designated entries exact."""
    s, off, x = E.nn_kind_case(kind, f)
    orc, exact = nn_expected(kind, f)
    got = run_nn(torch_cuda, lib, s, off, x)
    np.testing.assert_array_equal(got, orc)
    np.testing.assert_allclose(got, exact, rtol=0, atol=E.NN_ATOL)
    empty = np.diff(off) == 0
    assert (got[empty] == E.INFTY_COST).all() and (got[~empty] <= 2.0).all()
    if kind == "no_samples":
        assert empty.all() and (got == E.INFTY_COST).all()
    if kind == "anticorrelated":
        assert (got[0] > 1.5).all() and (got[1:] < 0.5).all()
    if kind == "signed_zero":
        assert (got[[0, 1, 3]] == 1.0).all() and (got[2] > 1.0).all()
    if kind == "zero_rows":
        assert (got[1] == 1.0).all() and (got[:, 3] == 1.0).all()


@pytest.mark.parametrize("f", E.NN_TILE_F)
def test_nn_clip_decides_exactly(torch_cuda, lib, f):
    """Samples used as given (BX_NN_SAMPLES_NORMALIZED) that are twice a normalised feature and
    its negation: dots of about 2 and -2, distances exactly 0 and 2 after the clip."""
    s, off, x = E.nn_clip_case(f)
    got = run_nn(torch_cuda, lib, s, off, x, BX_NN_SAMPLES_NORMALIZED)
    assert got[0, 0] == 0.0 and got[1, 0] == 2.0
    assert (got >= 0.0).all() and (got <= 2.0).all()
    np.testing.assert_allclose(got, E.exact_nn(s, off, x, normalized=True), rtol=0,
                               atol=E.NN_ATOL)


# ------------------------------------------------------------------ 5. the 128 x 256 tile
@pytest.mark.parametrize("cut", [0, 1], ids=["full", "cut_by_one"])
def test_nn_big_tile(torch_cuda, lib, cut):
    """G = 128 * 128 sample rows in 300 ragged targets against 300 detections at F = 17, and the
    same generator with G and D cut by one (a partial last row block and column block).  The op
    takes the 128 x 256 tile when ceil(G / 128) * ceil(D / 256) reaches the device's CU count;
    the rule is restated here and the case must qualify on this device, so it cannot fall back
    to the 64 x 64 tile unnoticed.  Which kernel ran cannot be observed from outside the op:
    this test holds the result, and the rule, not the launch.  Bit for bit the oracle, within
    1e-13 of numpy."""
    s, off, x = E.nn_big_case(cut)
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    assert E.big_tile_blocks(s.shape[0], x.shape[0]) >= cus, (s.shape, x.shape, cus)
    got = run_nn(torch_cuda, lib, s, off, x)
    np.testing.assert_array_equal(got, po.nn_cosine_distance(s, off, x))
    np.testing.assert_allclose(got, E.nn_numpy(s, off, x), rtol=0, atol=E.NN_ATOL)


# --------------------------------------------------------- 6. BoostTrack inside the engine
@pytest.mark.parametrize("emb_dim", [1, 17, 49, 113])
def test_boosttrack_odd_embedding_widths(torch_cuda, emb_dim):
    """The tile inside an engine at widths that are no multiple of 4 (a row tail inside a
    thread's staged pair / quad, rows that start off 16- and 32-byte phase): two sequences of
    about 12 objects over 12 frames, outputs and state bit for bit against the C oracle."""
    from boxmot_amd.synth import SyntheticScene
    from tests.test_gpu_parity import BOOST_ARGS, run_boost_batched

    scenes = [SyntheticScene(n_obj=12 + s, seed=1700 + 10 * emb_dim + s, emb_dim=emb_dim,
                             emb_dtype=np.float64, layout="crowded" if s else "grid", p_det=0.5,
                             conf_lo=0.3) for s in range(2)]
    run_boost_batched(torch_cuda, scenes, 12, dict(BOOST_ARGS), emb_dim, track_cap=64, det_cap=32)


# ------------------------------------------------------------------ 7. argument handling
# op -> (call(lib, src, out, **sizes), valid sizes, overrides that are zero-size (BX_OK),
# overrides that are invalid (BX_ERR_INVALID)); src is a readable device pointer, out a
# sentinel-filled buffer.  No call here may launch anything or write anywhere.
def _nn(L, s, o, G, T, D, F, off=True):
    return L.bx_nn_cosine_distance(s, G, s if off else None, T, s, D, F, 0, o, None)


ARG_OPS = {
    "deepoc_embcost": (lambda L, s, o, nd, nt, f: L.bx_deepoc_embcost(nd, nt, f, s, s, o, None),
                       dict(nd=2, nt=3, f=4), [dict(nd=0), dict(nt=0), dict(nd=0, nt=0)],
                       [dict(nd=-1), dict(nt=-1), dict(f=0), dict(f=-1)]),
    "hybrid_cosdist": (lambda L, s, o, nd, nt, f: L.bx_hybrid_cosdist(nd, nt, f, s, s, o, None),
                       dict(nd=2, nt=3, f=4), [dict(nd=0), dict(nt=0), dict(nd=0, nt=0)],
                       [dict(nd=-1), dict(nt=-1), dict(f=0), dict(f=-1)]),
    "hybrid_bank_mean": (lambda L, s, o, nt, f: L.bx_hybrid_bank_mean(nt, f, s, s, o, None),
                         dict(nt=2, f=4), [dict(nt=0)], [dict(nt=-1), dict(f=0), dict(f=-1)]),
    "nn_cosine_distance": (_nn, dict(G=3, T=2, D=3, F=4),
                           [dict(T=0), dict(D=0), dict(T=0, D=0, G=0)],
                           [dict(G=-1), dict(T=-1), dict(D=-1), dict(F=0), dict(F=-1),
                            dict(F=E.NN_F_MAX + 1), dict(off=False)]),
}


@pytest.mark.parametrize("op", sorted(ARG_OPS))
def test_argument_handling(torch_cuda, lib, op):
    """Zero sizes are BX_OK; negative sizes, F <= 0, F = 8193 for the nearest-neighbour op and a
    null offset array with T > 0 are BX_ERR_INVALID; neither writes a byte."""
    call, valid, zero, invalid = ARG_OPS[op]
    src = torch_cuda.zeros(4096, dtype=torch_cuda.float64, device="cuda")
    out = Guarded(torch_cuda, (4096,))
    for want, overrides in ((BX_OK, zero), (BX_ERR_INVALID, invalid)):
        for o in overrides:
            rc = call(lib, src.data_ptr(), out.ptr, **{**valid, **o})
            assert rc == want, (op, o, rc)
    assert out.untouched()

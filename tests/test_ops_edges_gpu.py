"""The stateless op-level HIP entry points at wave, block and grid-stride edges.

Every case comes from tests/ops_ref.py, whose reference side tests/test_ops_edges_host.py checks
on the CPU.  Here each HIP op must equal the C oracle bit for bit and tests/ops_ref.py by the
rule the host test established (ops_ref.assert_matches: bitwise, or the tolerance the project
already holds against the reference).  Every output lives between 64 leading and 64 trailing
sentinel elements that must survive the call.
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import ops_ref as R
from tests.test_ops_edges_host import oracle_kf_gating, oracle_kf_initiate, oracle_kf_update

pytestmark = pytest.mark.gpu

BX_OK, BX_ERR_INVALID = 0, 1
PAD, SENTINEL = 64, -72057.25
shape_id = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


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


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cases are read-only)


class Guarded:
    """A float64 device array between PAD leading and PAD trailing sentinel elements."""

    def __init__(self, torch, shape, init=None):
        self.torch, self.shape, self.n = torch, tuple(shape), int(np.prod(shape))
        self.buf = torch.full((PAD + self.n + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
        if init is not None:
            self.buf[PAD:PAD + self.n] = dev(torch, np.asarray(init, np.float64).reshape(-1))
        self.ptr = self.buf.data_ptr() + PAD * 8

    def _host(self):
        self.torch.cuda.synchronize()
        return self.buf.cpu().numpy()

    def get(self):
        """The array, after checking both guards."""
        h = self._host()
        assert (h[:PAD] == SENTINEL).all(), "write before the output"
        assert (h[PAD + self.n:] == SENTINEL).all(), "write past the output"
        return h[PAD:PAD + self.n].reshape(self.shape).copy()

    def untouched(self):
        return bool((self._host() == SENTINEL).all())


def ok(rc):
    assert rc == BX_OK, rc


# ------------------------------------------------------------------ association functions
@functools.lru_cache(maxsize=None)
def expected_asso(kind, shape):
    a, b = R.degenerate_boxes(kind) if shape == "degenerate" else R.box_case(shape)
    with np.errstate(all="ignore"):
        return a, b, po.asso_batch(kind, a, b, R.FRAME_W, R.FRAME_H), R.asso_batch(kind, a, b)


def run_pairwise(torch, lib, kind, a, b, lda, ldb):
    out = Guarded(torch, (a.shape[0], b.shape[0]))
    ad, bd = dev(torch, R.strided(a, lda)), dev(torch, R.strided(b, ldb))
    ok(lib.bx_pairwise_cost(po.ASSO_KIND[kind], ad.data_ptr(), a.shape[0], lda, bd.data_ptr(),
                            b.shape[0], ldb, float(R.FRAME_W), float(R.FRAME_H), out.ptr, None))
    return out.get()


def run_iou(torch, lib, a, b):
    out = Guarded(torch, (a.shape[0], b.shape[0]))
    ad, bd = dev(torch, a), dev(torch, b)
    ok(lib.bx_iou_batch(ad.data_ptr(), a.shape[0], bd.data_ptr(), b.shape[0], out.ptr, None))
    return out.get()


@pytest.mark.parametrize("shape", R.EW_SHAPES, ids=shape_id)
@pytest.mark.parametrize("kind", R.ASSO_KINDS)
def test_pairwise_cost_edges(torch_cuda, lib, kind, shape):
    a, b, orc, ref = expected_asso(kind, shape)
    assert np.isfinite(ref).all()
    for lda, ldb in R.STRIDES:
        got = run_pairwise(torch_cuda, lib, kind, a, b, lda, ldb)
        np.testing.assert_array_equal(got, orc)
        R.assert_matches(kind, got, ref)
    if kind == "iou":
        got = run_iou(torch_cuda, lib, a, b)
        np.testing.assert_array_equal(got, orc)
        R.assert_matches("iou", got, ref)


@pytest.mark.parametrize("kind", R.ASSO_KINDS)
def test_pairwise_cost_degenerate_rows(torch_cuda, lib, kind):
    a, b, orc, ref = expected_asso(kind, "degenerate")
    for lda, ldb in R.STRIDES:
        got = run_pairwise(torch_cuda, lib, kind, a, b, lda, ldb)
        np.testing.assert_array_equal(got, orc)
        R.assert_matches(kind, got, ref)
    if kind == "iou":
        got = run_iou(torch_cuda, lib, a, b)
        np.testing.assert_array_equal(got, orc)
        assert np.isnan(got[R.ZERO_WIDTH_ROW, R.ZERO_WIDTH_ROW]) and np.isnan(got).sum() == 1


@pytest.mark.parametrize("shape", R.EW_SHAPES, ids=shape_id)
def test_fuse_score_edges(torch_cuda, lib, shape):
    cost, conf = R.fuse_case(shape)
    c = Guarded(torch_cuda, shape, init=cost)
    cd = dev(torch_cuda, conf)
    ok(lib.bx_fuse_score(c.ptr, shape[0], shape[1], cd.data_ptr(), None))
    got = c.get()
    np.testing.assert_array_equal(got, po.fuse_score(cost, conf))
    ref = R.fuse_score(cost, conf)
    assert np.isfinite(ref).all()
    R.assert_matches("fuse", got, ref)


# ------------------------------------------------------------------ embedding distance
def run_embedding(torch, lib, t, d):
    out = Guarded(torch, (t.shape[0], d.shape[0]))
    td, dd = dev(torch, t), dev(torch, d)
    ok(lib.bx_embedding_distance(td.data_ptr(), t.shape[0], dd.data_ptr(), d.shape[0], t.shape[1],
                                 out.ptr, None))
    return out.get()


@pytest.mark.parametrize("shape", R.EW_SHAPES, ids=shape_id)
def test_embedding_distance_edges(torch_cuda, lib, shape):
    f = R.EMB_F_BIG if shape[0] * shape[1] > 1 << 20 else R.EMB_F_SMALL
    t, d = R.emb_case(*shape, f)
    got = run_embedding(torch_cuda, lib, t, d)
    np.testing.assert_array_equal(got, po.embedding_distance(t, d))
    ref = R.embedding_distance(t, d)
    assert np.isfinite(ref).all()
    R.assert_matches("embedding", got, ref)


@pytest.mark.parametrize("f", R.EMB_WIDTHS)
def test_embedding_distance_widths(torch_cuda, lib, f):
    for counts in R.EMB_COUNTS:
        for content in R.EMB_CONTENTS:
            t, d = R.emb_case(*counts, f, content)
            got = run_embedding(torch_cuda, lib, t, d)
            np.testing.assert_array_equal(got, po.embedding_distance(t, d))
            ref = R.embedding_distance(t, d)
            assert np.isfinite(ref).all()
            R.assert_matches("embedding", got, ref)


def test_embedding_distance_zero_row(torch_cuda, lib):
    t, d = R.emb_case(3, 129, 9, "zero_row")
    got = run_embedding(torch_cuda, lib, t, d)
    np.testing.assert_array_equal(got, po.embedding_distance(t, d))
    R.assert_matches("embedding", got, R.embedding_distance(t, d))
    assert np.isnan(got[1]).all() and np.isnan(got[:, 64]).all() and np.isnan(got).sum() == 129 + 2


# ---------------------------------------------------------------------- aw_max_metric
def run_aw(torch, lib, e, bottom):
    out = Guarded(torch, e.shape)
    ed = dev(torch, e)
    ok(lib.bx_aw_max_metric(ed.data_ptr(), e.shape[0], e.shape[1], R.AW_W, bottom, out.ptr, None))
    return out.get()


@pytest.mark.parametrize("bottom", R.AW_BOTTOMS)
@pytest.mark.parametrize("shape", R.AW_SHAPES, ids=shape_id)
def test_aw_max_metric_edges(torch_cuda, lib, shape, bottom):
    e = R.aw_case(shape, bottom)
    got = run_aw(torch_cuda, lib, e, bottom)
    np.testing.assert_array_equal(got, po.aw_max_metric(e, R.AW_W, bottom))
    ref = R.aw_max_metric(e, R.AW_W, bottom)
    assert np.isfinite(ref).all()
    R.assert_matches("aw", got, ref)


def test_aw_max_metric_infinite_entries(torch_cuda, lib):
    e = R.aw_inf_case()
    got = run_aw(torch_cuda, lib, e, 0.5)
    np.testing.assert_array_equal(got, po.aw_max_metric(e, R.AW_W, 0.5))
    R.assert_matches("aw", got, R.aw_max_metric(e, R.AW_W, 0.5))
    assert np.isnan(got[0]).all() and np.isnan(got[1:]).sum() == 0 and got[5, 5] == np.inf


# ----------------------------------------------------------------- XYAH / XYWH filter
def run_kf_update(torch, lib, kind, mean, cov, z, conf):
    n = mean.shape[0]
    m, P = Guarded(torch, (n, 8), init=mean), Guarded(torch, (n, 8, 8), init=cov)
    zd = dev(torch, z)
    cd = None if conf is None else dev(torch, conf)
    ok(lib.bx_kf_update(po.KF_KIND[kind], n, m.ptr, P.ptr, zd.data_ptr(),
                        None if cd is None else cd.data_ptr(), None))
    return m.get(), P.get()


def run_kf_gating(torch, lib, kind, mean, cov, zs):
    n, nz = mean.shape[0], zs.shape[0]
    out = Guarded(torch, (n, nz))
    md, Pd, zd = dev(torch, mean), dev(torch, cov), dev(torch, zs)
    ok(lib.bx_kf_gating_distance(po.KF_KIND[kind], n, md.data_ptr(), Pd.data_ptr(), zd.data_ptr(),
                                 nz, out.ptr, None))
    return out.get()


@pytest.mark.parametrize("n", R.KF_COUNTS)
@pytest.mark.parametrize("kind", R.KF_KINDS)
def test_kf_edges(torch_cuda, lib, kind, n):
    """initiate; three predicts of moving tracks; update with conf from {0, 0.5, 1, random};
    gating against 1, 9 and 65 measurements — a lone track, a wave less one, a full wave, a wave
    plus one, two blocks plus one and 200 tracks."""
    torch, c, k = torch_cuda, R.kf_case(kind, n), po.KF_KIND[kind]
    m, P = Guarded(torch, (n, 8)), Guarded(torch, (n, 8, 8))
    ok(lib.bx_kf_initiate(k, n, dev(torch, c["meas"]).data_ptr(), m.ptr, P.ptr, None))
    om, oP = oracle_kf_initiate(kind, c["meas"])
    gm, gP = m.get(), P.get()
    np.testing.assert_array_equal(gm, om)
    np.testing.assert_array_equal(gP, oP)
    R.assert_matches("kf_initiate", gm, c["mean0"])
    R.assert_matches("kf_initiate", gP, c["cov0"])

    m, P = Guarded(torch, (n, 8), init=c["moving"]), Guarded(torch, (n, 8, 8), init=c["cov0"])
    om, oP = c["moving"], c["cov0"]
    for rm, rP in c["preds"]:
        ok(lib.bx_kf_multi_predict(k, n, m.ptr, P.ptr, None))
        om, oP = po.kf_multi_predict(kind, om, oP)
        gm, gP = m.get(), P.get()
        np.testing.assert_array_equal(gm, om)
        np.testing.assert_array_equal(gP, oP)
        R.assert_matches("kf_predict", gm, rm)
        R.assert_matches("kf_predict", gP, rP)

    gm, gP = run_kf_update(torch, lib, kind, c["pred_mean"], c["pred_cov"], c["z"], c["conf"])
    om, oP = oracle_kf_update(kind, c["pred_mean"], c["pred_cov"], c["z"], c["conf"])
    np.testing.assert_array_equal(gm, om)
    np.testing.assert_array_equal(gP, oP)
    rm, rP = R.kf_update_batch(kind, c["pred_mean"], c["pred_cov"], c["z"], c["conf"])
    assert np.isfinite(rm).all() and np.isfinite(rP).all()
    R.assert_matches("kf_update_mean", gm, rm)
    R.assert_matches("kf_update_cov", gP, rP)

    for nz, zs in c["gate_z"].items():
        g = run_kf_gating(torch, lib, kind, c["pred_mean"], c["pred_cov"], zs)
        np.testing.assert_array_equal(g, oracle_kf_gating(kind, c["pred_mean"], c["pred_cov"], zs))
        rg = R.kf_gating_batch(kind, c["pred_mean"], c["pred_cov"], zs)
        assert np.isfinite(rg).all()
        R.assert_matches("kf_gating", g, rg)


@pytest.mark.parametrize("kind", R.KF_KINDS)
def test_kf_update_null_conf_is_zero_conf(torch_cuda, lib, kind):
    c = R.kf_case(kind, 65)
    zero = np.zeros(65)
    gm, gP = run_kf_update(torch_cuda, lib, kind, c["pred_mean"], c["pred_cov"], c["z"], None)
    zm, zP = run_kf_update(torch_cuda, lib, kind, c["pred_mean"], c["pred_cov"], c["z"], zero)
    np.testing.assert_array_equal(gm, zm)
    np.testing.assert_array_equal(gP, zP)
    om, oP = oracle_kf_update(kind, c["pred_mean"], c["pred_cov"], c["z"], zero)
    np.testing.assert_array_equal(gm, om)
    np.testing.assert_array_equal(gP, oP)
    rm, rP = R.kf_update_batch(kind, c["pred_mean"], c["pred_cov"], c["z"], zero)
    R.assert_matches("kf_update_mean", gm, rm)
    R.assert_matches("kf_update_cov", gP, rP)


@pytest.mark.parametrize("kind", R.KF_KINDS)
def test_kf_bad_covariance_is_an_ordinary_track(torch_cuda, lib, kind):
    """One track in the middle of 65 with a negative leading diagonal: the Cholesky factorisation
    fails, the update leaves that track's state, its gating row is NaN, and every other track
    comes out exactly as in the clean batch."""
    torch, c, t = torch_cuda, R.kf_case(kind, R.KF_BAD_N), R.KF_BAD_TRACK
    bad = R.kf_bad_cov(c)
    others = np.arange(R.KF_BAD_N) != t
    cm, cP = run_kf_update(torch, lib, kind, c["pred_mean"], c["pred_cov"], c["z"], c["conf"])
    gm, gP = run_kf_update(torch, lib, kind, c["pred_mean"], bad, c["z"], c["conf"])
    om, oP = oracle_kf_update(kind, c["pred_mean"], bad, c["z"], c["conf"])
    np.testing.assert_array_equal(gm, om)
    np.testing.assert_array_equal(gP, oP)
    np.testing.assert_array_equal(gm[t], c["pred_mean"][t])
    np.testing.assert_array_equal(gP[t], bad[t])
    np.testing.assert_array_equal(gm[others], cm[others])
    np.testing.assert_array_equal(gP[others], cP[others])
    rm, rP = R.kf_update_batch(kind, c["pred_mean"], bad, c["z"], c["conf"])
    R.assert_matches("kf_update_mean", gm, rm)
    R.assert_matches("kf_update_cov", gP, rP)
    zs = c["gate_z"][9]
    cg = run_kf_gating(torch, lib, kind, c["pred_mean"], c["pred_cov"], zs)
    g = run_kf_gating(torch, lib, kind, c["pred_mean"], bad, zs)
    np.testing.assert_array_equal(g, oracle_kf_gating(kind, c["pred_mean"], bad, zs))
    assert np.isnan(g[t]).all() and np.isfinite(g[others]).all()
    np.testing.assert_array_equal(g[others], cg[others])
    R.assert_matches("kf_gating", g, R.kf_gating_batch(kind, c["pred_mean"], bad, zs))


# ------------------------------------------------------- XYSR and Boost octet filters
@pytest.mark.parametrize("n", R.OCTET_COUNTS)
@pytest.mark.parametrize("filt", ["xysr", "boost"])
def test_octet_filter_partial_waves(torch_cuda, lib, filt, n):
    """Eight lanes per track: 1, 7, 9 and 33 tracks leave a wave whose upper octets have exited
    before the in-octet exchanges, 33 and 65 also cross a 32-track block.  Batches are distinct
    rows of the reference-captured steps, so the captured outputs' same rows are expected."""
    torch = torch_cuda
    pool = R.kf_ops_pool(filt)
    rows, init = R.octet_pick(filt, n)
    d = 7 if filt == "xysr" else 8
    x, P = Guarded(torch, (n, d)), Guarded(torch, (n, d, d))
    arg = dev(torch, pool["init_arg"][init])
    initiate = lib.bx_kf_xysr_initiate if filt == "xysr" else lib.bx_kf_boost_initiate
    ok(initiate(n, arg.data_ptr(), x.ptr, P.ptr, None))
    np.testing.assert_array_equal(x.get(), pool["init_x"][init])
    np.testing.assert_array_equal(P.get(), pool["init_P"][init])

    x = Guarded(torch, (n, d), init=pool["in_x"][rows])
    P = Guarded(torch, (n, d, d), init=pool["in_P"][rows])
    if filt == "xysr":
        ok(lib.bx_kf_xysr_predict(n, x.ptr, P.ptr, *R.XYSR_Q, None))
    else:
        ok(lib.bx_kf_boost_predict(n, x.ptr, P.ptr, None))
    np.testing.assert_array_equal(x.get(), pool["pred_x"][rows])
    np.testing.assert_array_equal(P.get(), pool["pred_P"][rows])

    z = dev(torch, pool["z"][rows])
    update = lib.bx_kf_xysr_update if filt == "xysr" else lib.bx_kf_boost_update
    ok(update(n, x.ptr, P.ptr, z.data_ptr(), None))
    kf = po.kf_xysr if filt == "xysr" else po.kf_boost
    ox, oP = kf("update", pool["pred_x"][rows], pool["pred_P"][rows], pool["z"][rows])
    gx, gP = x.get(), P.get()
    np.testing.assert_array_equal(gx, ox)
    np.testing.assert_array_equal(gP, oP)
    np.testing.assert_allclose(gx, pool["upd_x"][rows], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(gP, pool["upd_P"][rows], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("shape", R.MH_SHAPES, ids=shape_id)
def test_boost_mh_dist_edges(torch_cuda, lib, shape):
    torch = torch_cuda
    d, x, P = R.mh_case(*shape)
    out = Guarded(torch, shape)
    dd, xd, Pd = dev(torch, d), dev(torch, x), dev(torch, P)
    ok(lib.bx_kf_boost_mh_dist(shape[0], dd.data_ptr(), shape[1], xd.data_ptr(), Pd.data_ptr(),
                               out.ptr, None))
    got = out.get()
    np.testing.assert_array_equal(got, po.kf_boost("mh_dist", x, P, d))
    ref = R.boost_mh_dist(d, x, P)
    assert np.isfinite(ref).all()
    R.assert_matches("mh_dist", got, ref)


# ------------------------------------------------------------------ argument handling
# op -> (call(lib, src, out0, out1, **sizes), valid sizes, overrides that are zero-size (BX_OK),
# overrides that are invalid (BX_ERR_INVALID)); src is a readable device pointer, out0 / out1
# sentinel-filled buffers.  No call here may launch anything or write anywhere.
W, H = float(R.FRAME_W), float(R.FRAME_H)
ARG_OPS = {
    "iou_batch": (lambda L, s, o, p, na, nb: L.bx_iou_batch(s, na, s, nb, o, None),
                  dict(na=2, nb=3), [dict(na=0), dict(nb=0)], [dict(na=-1), dict(nb=-1)]),
    "pairwise_cost": (lambda L, s, o, p, kind, na, lda, nb, ldb:
                      L.bx_pairwise_cost(kind, s, na, lda, s, nb, ldb, W, H, o, None),
                      dict(kind=0, na=2, lda=4, nb=3, ldb=4), [dict(na=0), dict(nb=0)],
                      [dict(na=-1), dict(nb=-1), dict(lda=3), dict(ldb=3), dict(lda=0),
                       dict(kind=-1), dict(kind=6)]),
    "fuse_score": (lambda L, s, o, p, nr, nc: L.bx_fuse_score(o, nr, nc, s, None),
                   dict(nr=2, nc=3), [dict(nr=0), dict(nc=0)], [dict(nr=-1), dict(nc=-1)]),
    "embedding_distance": (lambda L, s, o, p, nt, nd, f:
                           L.bx_embedding_distance(s, nt, s, nd, f, o, None),
                           dict(nt=2, nd=3, f=4), [dict(nt=0), dict(nd=0)],
                           [dict(nt=-1), dict(nd=-1), dict(f=0), dict(f=-1)]),
    "aw_max_metric": (lambda L, s, o, p, nr, nc: L.bx_aw_max_metric(s, nr, nc, 0.75, 0.5, o, None),
                      dict(nr=2, nc=3), [dict(nr=0), dict(nc=0)],
                      [dict(nr=-1), dict(nc=-1), dict(nr=4097), dict(nc=4097)]),
    "kf_initiate": (lambda L, s, o, p, kind, n: L.bx_kf_initiate(kind, n, s, o, p, None),
                    dict(kind=0, n=2), [dict(n=0)], [dict(n=-1), dict(kind=2), dict(kind=-1)]),
    "kf_multi_predict": (lambda L, s, o, p, kind, n: L.bx_kf_multi_predict(kind, n, o, p, None),
                         dict(kind=1, n=2), [dict(n=0)], [dict(n=-1), dict(kind=2), dict(kind=-1)]),
    "kf_update": (lambda L, s, o, p, kind, n: L.bx_kf_update(kind, n, o, p, s, s, None),
                  dict(kind=0, n=2), [dict(n=0)], [dict(n=-1), dict(kind=2), dict(kind=-1)]),
    "kf_gating_distance": (lambda L, s, o, p, kind, n, nz:
                           L.bx_kf_gating_distance(kind, n, s, s, s, nz, o, None),
                           dict(kind=1, n=2, nz=3), [dict(n=0), dict(nz=0)],
                           [dict(n=-1), dict(nz=-1), dict(kind=2), dict(kind=-1)]),
    "kf_xysr_initiate": (lambda L, s, o, p, n: L.bx_kf_xysr_initiate(n, s, o, p, None),
                         dict(n=2), [dict(n=0)], [dict(n=-1)]),
    "kf_xysr_predict": (lambda L, s, o, p, n: L.bx_kf_xysr_predict(n, o, p, 0.01, 0.0001, None),
                        dict(n=2), [dict(n=0)], [dict(n=-1)]),
    "kf_xysr_update": (lambda L, s, o, p, n: L.bx_kf_xysr_update(n, o, p, s, None),
                       dict(n=2), [dict(n=0)], [dict(n=-1)]),
    "kf_boost_initiate": (lambda L, s, o, p, n: L.bx_kf_boost_initiate(n, s, o, p, None),
                          dict(n=2), [dict(n=0)], [dict(n=-1)]),
    "kf_boost_predict": (lambda L, s, o, p, n: L.bx_kf_boost_predict(n, o, p, None),
                         dict(n=2), [dict(n=0)], [dict(n=-1)]),
    "kf_boost_update": (lambda L, s, o, p, n: L.bx_kf_boost_update(n, o, p, s, None),
                        dict(n=2), [dict(n=0)], [dict(n=-1)]),
    "kf_boost_mh_dist": (lambda L, s, o, p, nd, nt: L.bx_kf_boost_mh_dist(nd, s, nt, s, s, o, None),
                         dict(nd=2, nt=3), [dict(nd=0), dict(nt=0)], [dict(nd=-1), dict(nt=-1)]),
}


@pytest.mark.parametrize("op", sorted(ARG_OPS))
def test_argument_handling(torch_cuda, lib, op):
    """Zero sizes are BX_OK, bad arguments BX_ERR_INVALID (negative sizes, a row stride below 4,
    an unknown kind, f <= 0, aw_max_metric past 4096); neither writes a byte."""
    call, valid, zero, invalid = ARG_OPS[op]
    src = torch_cuda.ones(4096, dtype=torch_cuda.float64, device="cuda")
    out0, out1 = Guarded(torch_cuda, (4096,)), Guarded(torch_cuda, (4096,))
    for want, overrides in ((BX_OK, zero), (BX_ERR_INVALID, invalid)):
        for o in overrides:
            rc = call(lib, src.data_ptr(), out0.ptr, out1.ptr, **{**valid, **o})
            assert rc == want, (op, o, rc)
    assert out0.untouched() and out1.untouched()

"""The reference side of the op-level edge cases, on the CPU.

tests/ops_ref.py (numpy/scipy, from the formulas) is first pinned to the reference-captured
vectors of tests/golden/ with the comparisons tests/test_oracle.py uses, so it is no unchecked
second opinion.  Then the C oracle is held against it on every case tests/test_ops_edges_gpu.py
runs on the device: bitwise where ops_ref.BITWISE says so, else within ops_ref.TOL.  Every random
case must be finite on both sides, so the GPU test cannot pass by comparing NaN with NaN.
"""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import ops_ref as R


@pytest.fixture(scope="module")
def K(golden_dir):
    return np.load(golden_dir / "kernels.npz")


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(golden_dir / "asso_funcs.npz")


# ------------------------------------------------------- the oracle on whole batches
def oracle_kf_initiate(kind, meas):
    out = [po.kf_initiate(kind, z) for z in meas]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def oracle_kf_update(kind, mean, cov, z, conf):
    out = [po.kf_update(kind, mean[i], cov[i], z[i], conf[i]) for i in range(mean.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def oracle_kf_gating(kind, mean, cov, zs):
    return np.stack([po.kf_gating_distance(kind, mean[i], cov[i], zs)
                     for i in range(mean.shape[0])])


def finite(*arrays):
    return all(np.isfinite(a).all() for a in arrays)


# ------------------------------------------------ ops_ref against the reference's vectors
def test_ref_iou_fuse_embedding_pinned(K):
    np.testing.assert_array_equal(R.iou_batch(K["iou_a"], K["iou_b"]), K["iou_out"])
    np.testing.assert_array_equal(R.fuse_score(K["fuse_cost_in"], K["fuse_conf"]), K["fuse_out"])
    np.testing.assert_array_equal(R.embedding_distance(K["emb_trk"], K["emb_det"]), K["emb_out"])


@pytest.mark.parametrize("kind", R.ASSO_KINDS)
@pytest.mark.parametrize("which", ["rand", "edge"])
def test_ref_asso_pinned(G, kind, which):
    with np.errstate(all="ignore"):
        got = R.asso_batch(kind, G[f"{which}_a"], G[f"{which}_b"], int(G["w"]), int(G["h"]))
    if kind == "ciou":  # np.arctan is the platform's libm: <= 1 ulp, as tests/test_oracle.py
        np.testing.assert_allclose(got, G[f"{kind}_{which}"], rtol=0, atol=4e-16)
    else:
        np.testing.assert_array_equal(got, G[f"{kind}_{which}"])


def test_ref_aw_max_metric_pinned(G):
    for k in range(int(G["aw_count"])):
        got = R.aw_max_metric(G[f"aw{k}_in"], float(G[f"aw{k}_w"]), 0.5)
        np.testing.assert_array_equal(got, G[f"aw{k}_out"])


@pytest.mark.parametrize("kind", R.KF_KINDS)
def test_ref_kalman_pinned(K, kind):
    m, c = R.kf_initiate(kind, K[f"kf_{kind}_meas"])
    np.testing.assert_array_equal(m, K[f"kf_{kind}_init_mean"])
    np.testing.assert_array_equal(c, K[f"kf_{kind}_init_cov"])
    pm, pc = R.kf_multi_predict(kind, K[f"kf_{kind}_pred_in_mean"], K[f"kf_{kind}_init_cov"])
    np.testing.assert_array_equal(pm, K[f"kf_{kind}_pred_mean"])
    np.testing.assert_array_equal(pc, K[f"kf_{kind}_pred_cov"])
    um, uc = R.kf_update_batch(kind, pm, pc, K[f"kf_{kind}_upd_z"], K[f"kf_{kind}_upd_conf"])
    np.testing.assert_allclose(um, K[f"kf_{kind}_upd_mean"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(uc, K[f"kf_{kind}_upd_cov"], rtol=1e-10, atol=1e-9)
    g = R.kf_gating_batch(kind, pm, pc, K[f"kf_{kind}_gate_z"])
    np.testing.assert_allclose(g, K[f"kf_{kind}_gate_out"], rtol=1e-10)


def test_ref_mh_dist_pinned(golden_dir):
    fx = np.load(golden_dir / "kf_ops.npz")
    for s in range(int(fx["boost_steps"])):
        got = R.boost_mh_dist(fx[f"boost_s{s}_mh_dets"], fx[f"boost_s{s}_pred_x"],
                              fx[f"boost_s{s}_pred_P"])
        np.testing.assert_array_equal(got, fx[f"boost_s{s}_mh"])


# ------------------------------------------------------------ the oracle against ops_ref
@pytest.mark.parametrize("shape", R.EW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", R.ASSO_KINDS)
def test_asso_edges(kind, shape):
    a, b = R.box_case(shape)
    ref = R.asso_batch(kind, a, b)
    got = po.asso_batch(kind, a, b, R.FRAME_W, R.FRAME_H)
    assert ref.shape == shape and finite(ref, got)
    R.assert_matches(kind, got, ref)
    if kind == "iou":
        np.testing.assert_array_equal(po.iou_batch(a, b), ref)


@pytest.mark.parametrize("kind", R.ASSO_KINDS)
def test_asso_degenerate_rows(kind):
    a, b = R.degenerate_boxes(kind)
    ref = R.asso_batch(kind, a, b)
    got = po.asso_batch(kind, a, b, R.FRAME_W, R.FRAME_H)
    R.assert_matches(kind, got, ref)
    # the only 0/0: iou and diou (no epsilon) of the zero-width box against itself
    nan = np.zeros(ref.shape, bool)
    if kind in ("iou", "diou"):
        nan[R.ZERO_WIDTH_ROW, R.ZERO_WIDTH_ROW] = True
    np.testing.assert_array_equal(np.isnan(ref), nan)
    assert np.isfinite(ref[~nan]).all()
    if kind == "iou":
        np.testing.assert_array_equal(po.iou_batch(a, b), ref)
        assert ref[0, 0] == 1.0 and ref[1, 1] == 0.0 and ref[2, 2] == 0.0
        assert ref[3, 3] == (100.0 * 100.0) / (400.0 * 400.0) and 0 < ref[5, 5] < 1


@pytest.mark.parametrize("shape", R.EW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fuse_edges(shape):
    cost, conf = R.fuse_case(shape)
    ref = R.fuse_score(cost, conf)
    got = po.fuse_score(cost, conf)
    assert finite(ref, got)
    R.assert_matches("fuse", got, ref)


def test_fuse_threshold_values():
    """The six designated confidences fall on the sides of 0.5 and 0.7 the formula gives them."""
    conf = np.array(R.FUSE_CONFS)
    ref = R.fuse_score(np.full((1, 6), 0.25), conf)[0]
    np.testing.assert_array_equal(po.fuse_score(np.full((1, 6), 0.25), conf)[0], ref)
    # 0 and just below 0.5: masked and doubled; 0.5 and 0.7: plain; above 0.7: boosted by 1.2
    np.testing.assert_array_equal(ref[[0, 4]], [2.0, 2.0])
    np.testing.assert_array_equal(ref[[1, 2]], [1 - 0.75 * 0.5, 1 - 0.75 * 0.7])
    np.testing.assert_array_equal(ref[[3, 5]], [1 - 0.75 * 1.2, 1 - 0.75 * (conf[5] * 1.2)])


@pytest.mark.parametrize("shape", R.EW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_embedding_edges(shape):
    f = R.EMB_F_BIG if shape[0] * shape[1] > 1 << 20 else R.EMB_F_SMALL
    t, d = R.emb_case(*shape, f)
    ref = R.embedding_distance(t, d)
    got = po.embedding_distance(t, d)
    assert ref.shape == shape and finite(ref, got)
    R.assert_matches("embedding", got, ref)


@pytest.mark.parametrize("content", R.EMB_CONTENTS)
@pytest.mark.parametrize("counts", R.EMB_COUNTS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("f", R.EMB_WIDTHS)
def test_embedding_widths(f, counts, content):
    t, d = R.emb_case(*counts, f, content)
    if content == "relu" and f > 2:
        assert (t == 0).any() or (d == 0).any()
    ref = R.embedding_distance(t, d)
    got = po.embedding_distance(t, d)
    assert finite(ref, got)
    R.assert_matches("embedding", got, ref)


def test_embedding_zero_row():
    """An all-zero row has norm 0 + 1e-8, a zero normalised row and a 0/0 cosine: NaN in its
    whole row / column on both sides, finite elsewhere."""
    t, d = R.emb_case(3, 129, 9, "zero_row")
    ref = R.embedding_distance(t, d)
    got = po.embedding_distance(t, d)
    nan = np.zeros(ref.shape, bool)
    nan[3 // 2, :] = True
    nan[:, 129 // 2] = True
    np.testing.assert_array_equal(np.isnan(ref), nan)
    R.assert_matches("embedding", got, ref)


@pytest.mark.parametrize("bottom", R.AW_BOTTOMS)
@pytest.mark.parametrize("shape", R.AW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_aw_max_metric_edges(shape, bottom):
    e = R.aw_case(shape, bottom)
    ref = R.aw_max_metric(e, R.AW_W, bottom)
    got = po.aw_max_metric(e, R.AW_W, bottom)
    assert finite(ref, got)
    R.assert_matches("aw", got, ref)
    if min(shape) >= 3:  # the designated lines got the weights they were built for
        m, w = (e, ref) if shape[0] >= 5 else (e.T, ref.T)
        assert (m[0] == 0).all() and (m[1] < 0).all() and (m[2] > 0).sum() == 1
        assert np.sort(m[3])[-1] == np.sort(m[3])[-2] and np.sort(m[4])[-2] == bottom


def test_aw_max_metric_infinite_entries():
    """Two +Inf in a row: ratio Inf / Inf = NaN, and Python's max(NaN, 0) keeps it, so the
    reference returns a NaN row.  The oracle (and the kernel's shared aw_weight) once clamped
    that NaN to 0 and returned weight 1."""
    e = R.aw_inf_case()
    ref = R.aw_max_metric(e, R.AW_W, 0.5)
    assert np.isnan(ref[0]).all() and not np.isnan(ref[1:]).any() and ref[5, 5] == np.inf
    assert np.isfinite(np.delete(ref[1:], 4 * 32 + 5)).all()
    R.assert_matches("aw", po.aw_max_metric(e, R.AW_W, 0.5), ref)


@pytest.mark.parametrize("n", R.KF_COUNTS)
@pytest.mark.parametrize("kind", R.KF_KINDS)
def test_kf_edges(kind, n):
    c = R.kf_case(kind, n)
    assert len({tuple(r) for r in c["meas"]}) == n  # every track distinct
    assert (c["moving"][:, 4:] != 0).all()
    m, P = oracle_kf_initiate(kind, c["meas"])
    R.assert_matches("kf_initiate", m, c["mean0"])
    R.assert_matches("kf_initiate", P, c["cov0"])
    m, P = c["moving"], c["cov0"]
    for rm, rP in c["preds"]:
        m, P = po.kf_multi_predict(kind, m, P)
        R.assert_matches("kf_predict", m, rm)
        R.assert_matches("kf_predict", P, rP)
    rm, rP = R.kf_update_batch(kind, c["pred_mean"], c["pred_cov"], c["z"], c["conf"])
    m, P = oracle_kf_update(kind, c["pred_mean"], c["pred_cov"], c["z"], c["conf"])
    assert finite(rm, rP, m, P)
    R.assert_matches("kf_update_mean", m, rm)
    R.assert_matches("kf_update_cov", P, rP)
    for nz, zs in c["gate_z"].items():
        rg = R.kf_gating_batch(kind, c["pred_mean"], c["pred_cov"], zs)
        g = oracle_kf_gating(kind, c["pred_mean"], c["pred_cov"], zs)
        assert rg.shape == (n, nz) and finite(rg, g)
        R.assert_matches("kf_gating", g, rg)


@pytest.mark.parametrize("kind", R.KF_KINDS)
def test_kf_bad_covariance(kind):
    """A negative leading diagonal: the update leaves that track's state, its gating row is NaN,
    and both sides agree on every other track."""
    c = R.kf_case(kind, R.KF_BAD_N)
    bad, t = R.kf_bad_cov(c), R.KF_BAD_TRACK
    rm, rP = R.kf_update_batch(kind, c["pred_mean"], bad, c["z"], c["conf"])
    m, P = oracle_kf_update(kind, c["pred_mean"], bad, c["z"], c["conf"])
    for mm, PP in ((rm, rP), (m, P)):
        np.testing.assert_array_equal(mm[t], c["pred_mean"][t])
        np.testing.assert_array_equal(PP[t], bad[t])
    R.assert_matches("kf_update_mean", m, rm)
    R.assert_matches("kf_update_cov", P, rP)
    zs = c["gate_z"][9]
    rg = R.kf_gating_batch(kind, c["pred_mean"], bad, zs)
    g = oracle_kf_gating(kind, c["pred_mean"], bad, zs)
    nan = np.zeros(rg.shape, bool)
    nan[t] = True
    np.testing.assert_array_equal(np.isnan(rg), nan)
    np.testing.assert_array_equal(np.isnan(g), nan)
    R.assert_matches("kf_gating", g, rg)


@pytest.mark.parametrize("shape", R.MH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mh_dist_edges(shape):
    d, x, P = R.mh_case(*shape)
    ref = R.boost_mh_dist(d, x, P)
    got = po.kf_boost("mh_dist", x, P, d)
    assert ref.shape == shape and finite(ref, got)
    R.assert_matches("mh_dist", got, ref)


@pytest.mark.parametrize("n", R.OCTET_COUNTS)
@pytest.mark.parametrize("filt", ["xysr", "boost"])
def test_octet_filter_batches(filt, n):
    """Tracks are independent, so the oracle on a batch of rows drawn from the captured steps
    gives the same rows of the captured outputs (as tests/test_oracle.py compares them)."""
    pool = R.kf_ops_pool(filt)
    rows, init = R.octet_pick(filt, n)
    assert len(set(rows.tolist())) == n
    assert len({r.tobytes() for r in pool["in_x"][rows]}) == n  # distinct tracks
    kf = po.kf_xysr if filt == "xysr" else po.kf_boost
    x, P = kf("initiate", None, None, pool["init_arg"][init])
    np.testing.assert_array_equal(x, pool["init_x"][init])
    np.testing.assert_array_equal(P, pool["init_P"][init])
    x, P = kf("predict", pool["in_x"][rows], pool["in_P"][rows])
    np.testing.assert_array_equal(x, pool["pred_x"][rows])
    np.testing.assert_array_equal(P, pool["pred_P"][rows])
    x, P = kf("update", x, P, pool["z"][rows])
    np.testing.assert_allclose(x, pool["upd_x"][rows], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(P, pool["upd_P"][rows], rtol=1e-12, atol=1e-9)

"""CPU checks of the sparse-optical-flow camera-motion compensation: the numpy restatement
(tests/sof_ref.py) against cases with known answers, its arithmetic worked by hand, and the public
surface of boxmot_amd.cmc.  OpenCV is not a dependency: nothing here (or anywhere in the project)
is compared with goodFeaturesToTrack, calcOpticalFlowPyrLK or estimateAffinePartial2D.

Recovery bounds are four times the restatement's measured error (DESIGN.md 2.17 records both)."""
import inspect

import numpy as np
import pytest

import boxmot_amd
from boxmot_amd import cmc
from tests import sof_ref as R

H, W = 96, 128
_runs = {}


def run_pair(name, second, **kw):
    """The restatement over (texture, second frame), computed once per name."""
    if name not in _runs:
        r = R.SofRef(scale=None, max_corners=200, **kw)
        first = r.apply(R.texture(H, W, 1))
        _runs[name] = (first, r.apply(second), r)
    return _runs[name]


def corner_error(M, A):
    """Largest displacement error of a warp over the image corners, in pixels."""
    c = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], float).T
    return np.abs(M @ c - A @ c).max()


# ------------------------------------------------------------------- the restatement's answers
def test_subpixel_shift_recovered():
    A = np.array([[1, 0, 1.3], [0, 1, -0.7]])
    first, (M, code, nk, nt, ni), r = run_pair("sub", R.texture(H, W, 1, A))
    assert first[1] == R.FIRST_FRAME and np.array_equal(first[0], np.eye(2, 3)) and first[2] == 200
    err_t, err_l = np.abs(M[:, 2] - A[:, 2]).max(), np.abs(M[:, :2] - A[:, :2]).max()
    print("sub-pixel shift: tracked", nt, "inliers", ni, "translation error", err_t, "linear", err_l)
    assert code == R.OK and nt >= 4 and ni >= 4 and len(r.levels) == 3
    assert err_t < 0.027   # measured 0.0066
    assert err_l < 1e-4    # measured 2.3e-5


def test_large_shift_needs_the_pyramid():
    # (6, -4) px left ECC's basin of convergence (tests/ecc_ref.py, case large_b)
    A = np.array([[1, 0, 6.0], [0, 1, -4.0]])
    _, (M, code, nk, nt, ni), r = run_pair("big", R.texture(H, W, 1, A))
    err = np.abs(M - A).max()
    print("large shift: tracked", nt, "inliers", ni, "error", err)
    assert code == R.OK and nt >= 4 and ni >= 4
    assert err < 7e-5  # measured 1.7e-5
    assert len(r.levels) == 3 and r.levels[2].shape == (24, 32)


def test_rotation_and_zoom_recovered():
    A = R.sim_warp(0.4, 1.01, 0.5, -0.3, 64, 48)
    _, (M, code, nk, nt, ni), _ = run_pair("rot", R.texture(H, W, 1, A))
    err_l, err_t = np.abs(M[:, :2] - A[:, :2]).max(), np.abs(M[:, 2] - A[:, 2]).max()
    print("rotation + zoom: tracked", nt, "inliers", ni, "linear", err_l, "translation", err_t)
    assert code == R.OK and nt >= 4 and ni >= 4
    assert M[0, 0] == M[1, 1] and M[0, 1] == -M[1, 0]  # a similarity
    assert err_l < 1.7e-4   # measured 4.2e-5
    assert err_t < 0.0042   # measured 0.00103


def test_consensus_ignores_a_moving_foreground():
    # a 64 x 48 patch (a quarter of the frame) moves by (-7, 6) while the background moves by
    # (1.3, -0.7); win 9 keeps the band of windows that see both motions narrow
    A = np.array([[1, 0, 1.3], [0, 1, -0.7]])
    B = np.array([[1, 0, -7.0], [0, 1, 6.0]])
    box = (40, 30, 104, 78)
    assert (box[2] - box[0]) * (box[3] - box[1]) * 4 == H * W
    _, (M, code, nk, nt, ni), r = run_pair("two", R.two_motion_frame(H, W, 1, A, B, box),
                                           win_size=9)
    rec = r.record
    P, Q = rec["prev"][rec["tracked"]], rec["next"][rec["tracked"]]
    plain = R.lstsq_similarity(P, Q)
    e_fit, e_plain = corner_error(M, A), corner_error(plain, A)
    print("two motions: tracked", nt, "inliers", ni, "consensus", e_fit, "plain", e_plain)
    assert code == R.OK and nt >= 4 and 4 <= ni < nt
    assert e_fit < 0.25     # measured 0.062
    assert e_plain > 0.25   # measured 1.97: the plain fit over every tracked point is pulled away
    assert rec["inlier"].sum() == ni and not rec["inlier"][~rec["tracked"]].any()


def test_translation_upscaled_by_inverse_scale():
    a = R.texture(192, 256, 1)
    b = R.texture(192, 256, 1, np.array([[1, 0, 2.6], [0, 1, -1.4]]))
    r = R.SofRef(scale=0.5, max_corners=200)
    r.apply(a)
    M, code, _, nt, _ = r.apply(b)
    assert code == R.OK and nt >= 4 and r.levels[0].shape == (96, 128)
    assert np.abs(M[:, 2] - [2.6, -1.4]).max() < 0.1  # full-resolution pixels
    r1 = R.SofRef(scale=None, max_corners=200)
    r1.apply(R.prep(a, 0.5).astype(np.uint8))
    M1 = r1.apply(R.prep(b, 0.5).astype(np.uint8))[0]
    assert np.array_equal(M[:, 2], M1[:, 2] / 0.5) and np.array_equal(M[:, :2], M1[:, :2])


def test_codes_without_corners_and_with_few_points():
    flat = np.full((H, W), 77, np.uint8)
    r = R.SofRef(scale=None, win_size=9)
    assert r.apply(flat)[1] == R.NO_KEYPOINTS and r.levels is None
    out = r.apply(R.texture(H, W, 1))  # still a first frame
    assert out[1] == R.FIRST_FRAME and out[2] > 0
    # one blob on a flat frame, then a flat frame: no corner to detect, the tracked points are kept
    r = R.SofRef(scale=None, win_size=9)
    img = flat.copy()
    img[40:44, 60:64] = 200  # one blob: a handful of corners, all close together
    r.apply(img)
    n0 = len(r.kp)
    assert 0 < n0
    M, code, nk, nt, ni = r.apply(flat)
    assert nk == nt and (code in (R.OK, R.TOO_FEW, R.NO_MODEL))
    if code != R.OK:
        assert np.array_equal(M, np.eye(2, 3))


# -------------------------------------------------------------------------- arithmetic by hand
def test_pyramid_by_hand():
    g = np.arange(37 * 53).reshape(37, 53) % 251
    lv = R.pyramid(g, 9, 3)
    assert [a.shape for a in lv] == [(37, 53), (19, 27), (10, 14)]  # 5 x 7 is not above 9
    assert [a.shape for a in R.pyramid(g[:22, :30], 21, 3)] == [(22, 30)]  # 11 x 15: level 0 only
    assert [a.shape for a in R.pyramid(g, 9, 1)] == [(37, 53), (19, 27)]
    # pixel (x 3, y 2) of level 1: rows 2..6, columns 4..8 of level 0 under [1 4 6 4 1]^2
    k = np.array([1, 4, 6, 4, 1])
    want = (int((np.outer(k, k) * g[2:7, 4:9]).sum()) + 128) >> 8
    assert lv[1][2, 3] == want
    # pixel (0, 0): reflect-101 (index -1 reads 1, -2 reads 2)
    rows = [2, 1, 0, 1, 2]
    want = (int((np.outer(k, k) * g[np.ix_(rows, rows)]).sum()) + 128) >> 8
    assert lv[1][0, 0] == want
    # a constant image stays constant
    assert np.all(R.pyr_down(np.full((9, 12), 200)) == 200)


def test_lambda_by_hand():
    # a vertical step edge: Dy = 0 everywhere, so b = c = 0 and lambda = 0.5 a - sqrt(0.25 a^2) = 0
    g = np.zeros((8, 8), np.int64)
    g[:, 4:] = 10
    lam = R.lam_plane(g)
    assert np.all(lam == 0)
    # a corner, against explicit loops over the 3x3 block with reflected indices
    rng = np.random.default_rng(11)
    g = rng.integers(0, 256, (7, 9)).astype(np.int64)
    g[3:, 4:] += 300
    lam = R.lam_plane(g)

    def refl(i, n):
        return -i if i < 0 else 2 * n - 2 - i if i >= n else i

    def sobel(x, y):
        v = lambda dx, dy: int(g[refl(y + dy, 7), refl(x + dx, 9)])  # noqa: E731
        dx = (v(1, -1) - v(-1, -1)) + 2 * (v(1, 0) - v(-1, 0)) + (v(1, 1) - v(-1, 1))
        dy = (v(-1, 1) - v(-1, -1)) + 2 * (v(0, 1) - v(0, -1)) + (v(1, 1) - v(1, -1))
        return dx, dy

    for x, y in [(4, 3), (0, 0), (8, 6), (1, 5), (8, 0)]:
        a = b = c = 0
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                dx, dy = sobel(refl(x + j, 9), refl(y + i, 7))
                a, b, c = a + dx * dx, b + dx * dy, c + dy * dy
        assert lam[y, x] == 0.5 * (a + c) - np.sqrt(0.25 * float(a - c) ** 2 + float(b) * b)
    kp = R.keypoints(g, 10, 0.01)
    assert 1 <= len(kp) <= 10 and np.all((kp[:, 0] >= 1) & (kp[:, 0] <= 7))
    assert np.all((kp[:, 1] >= 1) & (kp[:, 1] <= 5))


def test_selection_order_and_ties():
    # a periodic integer texture gives exactly equal lambdas: the pixel index breaks the ties
    ys, xs = np.mgrid[0:24, 0:32]
    g = ((xs % 8 < 4) ^ (ys % 8 < 4)).astype(np.int64) * 100
    lam = R.lam_plane(g)
    cand = np.flatnonzero(R.candidates(lam, 0.01).ravel())
    vals = lam.ravel()[cand]
    assert len(cand) > 20 and len(np.unique(vals)) < len(cand)  # ties exist
    kp = R.keypoints(g, 20, 0.01)
    idx = (kp[:, 1] * 32 + kp[:, 0]).astype(int)
    lv = lam.ravel()[idx]
    assert len(kp) == 20 and np.all(np.diff(lv) <= 0)
    for i in range(19):
        if lv[i] == lv[i + 1]:
            assert idx[i] < idx[i + 1]
    # cutting at 20 inside a tie keeps the lowest indices of the tied value
    tied = cand[vals == lv[-1]]
    kept = idx[lv == lv[-1]]
    assert np.array_equal(kept, tied[: len(kept)])


def test_generator_and_fit_by_hand():
    # the counter-based generator (an integer hash, no state): fixed values
    assert [R.mix(x) for x in (0, 1, 2, 3)] == [0, 1753845952, 3507691905, 1408362973]
    # an exact similarity through every pair: every hypothesis has every point, k = 0 wins
    rng = np.random.default_rng(5)
    P = rng.uniform(0, 100, (40, 2))
    A = R.sim_warp(3.0, 1.05, 2.0, -1.0)
    Q = P @ A[:, :2].T + A[:, 2]
    M, code, winner, inl = R.fit(P, Q)
    i, j = R.mix(0) % 40, R.mix(1) % 40
    assert (code, winner) == (R.OK, 0 if i != j else winner) and inl.all()
    assert np.abs(M - A).max() < 1e-12
    # outliers: 15 of 40 points moved far away are not in the winner's set
    Q2 = Q.copy()
    Q2[:15] += 50.0
    M, code, winner, inl = R.fit(P, Q2)
    assert code == R.OK and not inl[:15].any() and inl[15:].all()
    assert np.abs(M - A).max() < 1e-12
    # three points: too few; coincident points only: no model
    assert R.fit(P[:3], Q[:3])[1] == R.TOO_FEW
    same = np.tile(P[:1], (5, 1))
    assert R.fit(same, same + 1.0)[1] == R.NO_MODEL


# ----------------------------------------------------------------------------- public surface
def test_exports_and_codes():
    for name in ("SOF", "SofBatch", "ECC", "EccBatch", "get_cmc_method"):
        assert name in boxmot_amd.__all__ and hasattr(boxmot_amd, name)
    assert (cmc.SOF_OK, cmc.SOF_FIRST_FRAME, cmc.SOF_TOO_FEW, cmc.SOF_NO_MODEL,
            cmc.SOF_NO_KEYPOINTS) == (R.OK, R.FIRST_FRAME, R.TOO_FEW, R.NO_MODEL, R.NO_KEYPOINTS)
    assert cmc.SOF_HYPOTHESES == R.HYPOTHESES


def test_sof_signature_is_the_references():
    # motion/cmc/sof.py:14 and :64
    sig = inspect.signature(boxmot_amd.SOF.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("scale", 0.15)]
    ap = inspect.signature(boxmot_amd.SOF.apply)
    assert [(p.name, p.default) for p in list(ap.parameters.values())[1:]] == [
        ("img", inspect.Parameter.empty), ("detections", None)]
    s = boxmot_amd.SOF()
    assert (s.scale, s.grayscale, s.max_corners, s.quality_level, s.min_distance, s.block_size,
            s.win_size, s.max_level, s.criteria, s.ransac_threshold) == (
                0.15, True, 1000, 0.01, 1, 3, 21, 3, (30, 0.01), 3.0)
    assert s.last is None
    b = boxmot_amd.SofBatch(4)
    assert (b.n_streams, b.scale, b.win_size, b.max_corners) == (4, 0.15, 21, 1000)


def test_get_cmc_method_unchanged():
    assert boxmot_amd.get_cmc_method("ecc") is boxmot_amd.ECC
    for name in ("orb", "sift", "sof"):
        with pytest.raises(NotImplementedError, match=name):
            boxmot_amd.get_cmc_method(name)
    with pytest.raises(NotImplementedError, match="boxmot_amd.SOF"):
        boxmot_amd.get_cmc_method("sof")
    assert boxmot_amd.get_cmc_method("nope") is None


def test_refusals_need_no_device():
    img = np.zeros((40, 40, 3), np.uint8)
    s = boxmot_amd.SOF()
    s.min_distance = 2
    with pytest.raises(NotImplementedError, match="min_distance"):
        s.apply(img)
    s = boxmot_amd.SOF()
    s.block_size = 5
    with pytest.raises(NotImplementedError, match="block_size"):
        s.apply(img)
    for bad in (20, 3, 33):
        s = boxmot_amd.SOF()
        s.win_size = bad
        with pytest.raises(ValueError, match="win_size"):
            s.apply(img)
    s = boxmot_amd.SOF()
    s.max_corners = 5000
    with pytest.raises(ValueError, match="max_corners"):
        s.apply(img)
    with pytest.raises(NotImplementedError):
        boxmot_amd.SOF(scale=[4, 4]).apply(img)
    b = boxmot_amd.SofBatch(2)
    b.min_distance = 3
    with pytest.raises(NotImplementedError, match="min_distance"):
        b.apply(img[None])
    with pytest.raises(ValueError):
        boxmot_amd.SofBatch(0)

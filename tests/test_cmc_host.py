"""CPU checks of the ECC camera-motion compensation: the numpy restatement (tests/ecc_ref.py)
against cases with known answers, the preprocessing arithmetic worked by hand, and the public
surface of boxmot_amd.cmc.  OpenCV is not a dependency: nothing here (or anywhere in the
project) is compared with cv2.findTransformECC itself."""
import inspect

import numpy as np
import pytest

import boxmot_amd
from boxmot_amd import cmc
from tests import ecc_ref as R


# ------------------------------------------------------------------- the restatement's answers
@pytest.mark.parametrize("name", ["shift_a", "shift_b", "shift_c"])
def test_translation_recovered(name):
    A = R.CASES[name][4]
    assert np.hypot(A[0, 2], A[1, 2]) < 2.0
    M, rho, it, code = R.solve_case(name)
    err = np.abs(M[:, 2] - A[:, 2]).max()
    print(name, "recovered", M[:, 2], "error", err, "rho", rho, "iterations", it)
    assert code == R.OK and it < 20
    assert np.array_equal(M[:, :2], np.eye(2))
    assert err < 0.02
    assert rho > 0.95


@pytest.mark.parametrize("name", ["euclidean", "affine"])
def test_linear_part_recovered(name):
    A = R.CASES[name][4]
    M, rho, it, code = R.solve_case(name)
    err = np.abs(M[:, :2] - A[:, :2]).max()
    print(name, "linear error", err, "translation error", np.abs(M[:, 2] - A[:, 2]).max(), it)
    assert code == R.OK and it < 20
    assert err < 2e-3
    if name == "euclidean":  # a rotation: the angle is the parameter
        assert M[0, 0] == M[1, 1] and M[0, 1] == -M[1, 0]
        assert abs(M[0, 0] ** 2 + M[1, 0] ** 2 - 1) < 1e-15


@pytest.mark.parametrize("name", ["large_a", "large_b"])
def test_large_shift_not_converged(name):
    M, rho, it, code = R.solve_case(name)
    assert code == R.NOT_CONVERGED
    assert np.array_equal(M, np.eye(2, 3))


def test_masked_case_leaves_pixels_out():
    # the "outside" case starts 21 px to the right: a third of the 64 columns map past the image
    h, w, _, _, A, init, _ = R.CASES["outside"]
    assert R.mask_count(np.eye(2, 3), h, w) == h * w
    assert R.mask_count(init, h, w) == h * (w - 21) and 3 * 21 * h >= 0.98 * h * w
    M, rho, it, code = R.solve_case("outside")
    assert code == R.OK and np.abs(M[:, 2] - A[:, 2]).max() < 0.02
    assert R.mask_count(M, h, w) == h * (w - 21)  # 21.3 rounds to 21 columns, 0.4 to no row
    # a vertical start drops rows: nearest pixel of y + 0.5 is y + 1 (half rounds up)
    assert R.mask_count(R.shift_warp(0.0, 0.5), h, w) == (h - 1) * w
    assert R.mask_count(R.shift_warp(-0.5, 0.0), h, w) == h * w  # floor(x - 0.5 + 0.5) = x


def test_first_frame_is_identity():
    ref = R.EccRef(scale=None)
    M, rho, it, code = ref.apply(R.texture(48, 64, 1))
    assert code == R.FIRST_FRAME and it == 0 and np.array_equal(M, np.eye(2, 3))
    assert ref.prev is not None


def test_constant_image_not_converged():
    ref = R.EccRef(scale=None)
    ref.apply(R.texture(48, 64, 1))
    M, rho, it, code = ref.apply(np.full((48, 64), 77, np.uint8))
    assert code == R.NOT_CONVERGED and np.isnan(rho) and it == 1
    assert np.array_equal(M, np.eye(2, 3))
    # the constant image became the previous one all the same
    assert np.array_equal(ref.prev, np.full((48, 64), 77, np.uint8))


def test_count_exits():
    assert R.solve_case("iter1")[2] == 1 and R.solve_case("iter3")[2] == 3
    assert R.solve_case("iter1")[3] == R.OK
    ref = R.EccRef(scale=None, max_iter=0)
    a, b = R.case_frames("shift_a")
    ref.apply(a)
    M, rho, it, code = ref.apply(b)
    assert (rho, it, code) == (-1.0, 0, R.OK) and np.array_equal(M, np.eye(2, 3))


def test_translation_upscaled_by_inverse_scale():
    a = R.texture(96, 128, 1)
    b = R.texture(96, 128, 1, R.shift_warp(2.6, -1.4))
    ref = R.EccRef(scale=0.5)
    ref.apply(a)
    M, rho, it, code = ref.apply(b)
    assert code == R.OK
    ga, gb = R.prep(a, 0.5), R.prep(b, 0.5)
    assert ga[0].shape == (48, 64)
    Mw, rw, iw, cw = R.ecc_solve(ga[0], gb[0].astype(np.float64), gb[1], gb[2], R.TRANSLATION,
                                 1e-5, 100)
    assert np.array_equal(M[:, 2], Mw[:, 2] / 0.5) and np.array_equal(M[:, :2], Mw[:, :2])
    assert np.abs(M[:, 2] - [2.6, -1.4]).max() < 0.1  # full-resolution pixels
    # no division without a resize
    ref = R.EccRef(scale=None)
    ref.apply(ga[0])
    assert np.array_equal(ref.apply(gb[0])[0], Mw)


# ------------------------------------------------------------------------------ preprocessing
def test_grey_by_hand():
    # (B, G, R) -> (1868 B + 9617 G + 4899 R + 8192) >> 14, each worked by hand
    worked = [((255, 0, 0), 29),      # 484532 / 16384 = 29.57
              ((0, 255, 0), 150),     # 2460527 / 16384 = 150.18
              ((0, 0, 255), 76),      # 1257437 / 16384 = 76.75
              ((255, 255, 255), 255),
              ((10, 20, 30), 22),     # 366182 / 16384 = 22.35
              ((100, 150, 200), 159),  # 2617342 / 16384 = 159.75
              ((1, 1, 1), 1),         # 24576 / 16384 = 1.5
              ((0, 0, 0), 0),
              ((200, 100, 50), 96),   # 1588442 / 16384 = 96.95
              ((3, 200, 7), 120)]     # 1971489 / 16384 = 120.33
    px = [worked[k % len(worked)] for k in range(16)]
    img = np.array([p[0] for p in px], np.uint8).reshape(4, 4, 3)
    want = np.array([p[1] for p in px], np.uint8).reshape(4, 4)
    g, gx, gy = R.prep(img, None)
    assert g.dtype == np.uint8 and np.array_equal(g, want)
    # gradients: reflect-101 makes the border differences zero
    assert np.all(gx[:, 0] == 0) and np.all(gx[:, -1] == 0) and np.all(gy[0] == 0)
    assert gx[0, 1] == 0.5 * (int(want[0, 2]) - int(want[0, 0]))
    assert gy[2, 3] == 0.5 * (int(want[3, 3]) - int(want[1, 3]))
    assert gx.dtype == np.float32 and gy.dtype == np.float32


def test_resize_by_hand():
    ys, xs = np.mgrid[0:20, 0:40]
    g = (2 * xs + 3 * ys).astype(np.uint8)  # grey input, at most 135
    out, _, _ = R.prep(g, 0.15)
    assert out.shape == (3, 6)
    # output (0, 0): f = 0.5 / 0.15 - 0.5 = 2.8333 on both axes: s0 = 2, q = rint(0.8333 * 2048) =
    # 1707; taps g[2][2] = 10, g[2][3] = 12, g[3][2] = 13, g[3][3] = 15 with 341 = 2048 - 1707:
    # (10 * 341 * 341 + 12 * 1707 * 341 + 13 * 341 * 1707 + 15 * 1707 * 1707 + 2^21) >> 22
    #   = (1162810 + 6985044 + 7567131 + 43707735 + 2097152) >> 22 = 61519872 >> 22 = 14
    assert out[0, 0] == 14
    # output (y 2, x 5): fx = 5.5 / 0.15 - 0.5 = 36.1667: s0 = 36, qx = 341; fy = 16.1667: s0 = 16,
    # qy = 341; taps 120, 122, 123, 125:
    # (120 * 2913849 + 122 * 582087 + 123 * 582087 + 125 * 116281 + 2^21) >> 22
    #   = 508905472 >> 22 = 121
    assert out[2, 5] == 121
    x0, x1, q = R.axis_taps(6, 0.15, 40)
    assert (x0[0], x1[0], q[0]) == (2, 3, 1707) and (x0[5], x1[5], q[5]) == (36, 37, 341)
    # clamped edges: a scale whose first sample lies left of pixel 0, and the last pixel
    x0, x1, q = R.axis_taps(3, 0.75, 4)
    assert (x0[0], q[0]) == (0, rint_q(1 / 6)) and (x0[2], x1[2], q[2]) == (2, 3, rint_q(5 / 6))
    x0, x1, q = R.axis_taps(2, 0.999, 2)
    assert (x0[1], x1[1], q[1]) == (1, 1, 0)


def rint_q(a):
    return int(np.rint(a * 2048))


def test_working_sizes_round_half_even():
    assert R.work_size(1080, 1920, 0.15) == (162, 288)
    assert R.work_size(10, 30, 0.25) == (2, 8)  # 2.5 -> 2, 7.5 -> 8
    assert R.work_size(37, 53, 0.15) == (6, 8)  # 5.55, 7.95
    assert R.work_size(37, 53, None) == (37, 53) and R.work_size(37, 53, 1.0) == (37, 53)
    for H, W, s in [(1080, 1920, 0.15), (10, 30, 0.25), (37, 53, 0.5), (37, 53, None), (9, 9, 2.0)]:
        assert cmc.work_size(H, W, s) == R.work_size(H, W, s)


# ----------------------------------------------------------------------------- public surface
def test_exports_and_constants():
    for name in ("ECC", "EccBatch", "get_cmc_method", "MOTION_TRANSLATION", "MOTION_EUCLIDEAN",
                 "MOTION_AFFINE", "MOTION_HOMOGRAPHY"):
        assert name in boxmot_amd.__all__ and hasattr(boxmot_amd, name)
    assert (boxmot_amd.MOTION_TRANSLATION, boxmot_amd.MOTION_EUCLIDEAN, boxmot_amd.MOTION_AFFINE,
            boxmot_amd.MOTION_HOMOGRAPHY) == (0, 1, 2, 3)
    assert (cmc.OK, cmc.FIRST_FRAME, cmc.NOT_CONVERGED) == (R.OK, R.FIRST_FRAME, R.NOT_CONVERGED)


def test_ecc_signature_is_the_references():
    # motion/cmc/ecc.py:14-22 (cv2.MOTION_TRANSLATION is 0)
    sig = inspect.signature(boxmot_amd.ECC.__init__)
    got = [(p.name, p.default) for p in list(sig.parameters.values())[1:]]
    assert got == [("warp_mode", 0), ("eps", 1e-5), ("max_iter", 100), ("scale", 0.15),
                   ("align", False), ("grayscale", True)]
    e = boxmot_amd.ECC()
    assert e.prev_img is None and e.scale == 0.15 and e.termination_criteria == (3, 100, 1e-5)
    names = list(inspect.signature(boxmot_amd.ECC.apply).parameters)
    assert names[:3] == ["self", "img", "dets"]


def test_get_cmc_method():
    assert boxmot_amd.get_cmc_method("ecc") is boxmot_amd.ECC
    for name in ("orb", "sift", "sof"):
        with pytest.raises(NotImplementedError, match=name):
            boxmot_amd.get_cmc_method(name)
    assert boxmot_amd.get_cmc_method("nope") is None  # as motion/cmc/__init__.py


def test_refusals_need_no_device():
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="HOMOGRAPHY"):
        boxmot_amd.ECC(warp_mode=boxmot_amd.MOTION_HOMOGRAPHY).apply(img)
    with pytest.raises(NotImplementedError):
        boxmot_amd.ECC(scale=[4, 4]).apply(img)
    with pytest.raises(NotImplementedError):
        boxmot_amd.ECC(align=True).apply(img)
    with pytest.raises(NotImplementedError, match="HOMOGRAPHY"):
        boxmot_amd.EccBatch(2, warp_mode=boxmot_amd.MOTION_HOMOGRAPHY).apply(img[None])


def test_drop_ins_keep_the_identity_default():
    from boxmot_amd.trackers.botsort import IdentityCMC

    t = boxmot_amd.BotSort(with_reid=True)
    assert isinstance(t.cmc, IdentityCMC)

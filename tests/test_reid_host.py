"""The ReID front end without a GPU: the numpy restatement (tests/reid_ref.py) against values
worked out by hand and against the framework's own arithmetic on the CPU, the header against the
binding table, the argument checks of the C entry points (they run before any device call), and
the loud failure without a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from boxmot_amd import _native as N
from tests import reid_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "bxreid.h"


# ------------------------------------------------------------------------------- restatement
def test_resize_2x2_to_4x4_by_hand():
    # per axis L = 2, O = 4: f = d / 2 - 0.25 = -0.25, 0.25, 0.75, 1.25, so the weights of the
    # second pixel are 0 (clamped), 1/4, 3/4, 1 (clamped); every product is exact in 22 bits and
    # the blend rounds the exact bilinear value half up
    crop = np.array([[0, 100], [200, 40]], np.uint8)[..., None]
    want = np.array([[0, 25, 75, 100],        # 0.75 * 0 + 0.25 * 100 = 25, ...
                     [50, 59, 76, 85],        # 58.75 -> 59, 76.25 -> 76
                     [150, 126, 79, 55],      # 126.25 -> 126, 78.75 -> 79
                     [200, 160, 80, 40]], np.uint8)
    assert np.array_equal(R.resize(crop, 4, 4)[..., 0], want)
    s0, s1, q = R.axis_taps(2, 4)
    assert s0.tolist() == [0, 0, 0, 1] and s1.tolist() == [1, 1, 1, 1]
    assert q.tolist() == [0, 512, 1536, 0]


def test_resize_one_pixel_wide_crop():
    # L = 1 in x: every tap is pixel 0 with weight 0; in y 3 -> 6 is the 2x2 case's ratio
    crop = np.array([[10], [50], [250]], np.uint8)[..., None]
    got = R.resize(crop, 6, 5)[..., 0]
    col = np.array([10, 20, 40, 100, 200, 250], np.uint8)  # f = -0.25, 0.25, ..., 2.25
    assert np.array_equal(got, np.repeat(col[:, None], 5, 1))


def test_resize_to_its_own_size_reproduces_the_pixels():
    crop = np.random.default_rng(3).integers(0, 256, (9, 7, 3), dtype=np.uint8)
    assert np.array_equal(R.resize(crop, 9, 7), crop)


def test_corners_round_half_to_even_and_clamp():
    assert R.corners([2.5, 3.5, 6.5, 7.5], 48, 64) == (2, 4, 6, 8)
    assert R.corners([0.5, 1.5, 4.5, 5.5], 48, 64) == (0, 2, 4, 6)
    assert R.corners([-3.0, -2.0, 1e9, 1e9], 48, 64) == (0, 0, 64, 48)
    assert R.corners([62.4, 46.6, 63.5, 47.5], 48, 64) == (62, 47, 64, 48)
    for box in ([30, 10, 20, 40], [10, 10, 10.4, 40], [70, 10, 90, 40], [-9, 10, -1, 40],
                [np.nan, 1, 5, 5], [1, 1, np.inf, 5], [-np.inf, 1, 5, 5], [1e9, 1, 2e9, 5]):
        assert R.corners(box, 48, 64) is None, box


def test_crops_layout_swap_and_codes():
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    boxes = np.array([[5, 6, 12, 15], [30, 30, 20, 40], [5, 6, 12, 15]], np.float32)
    out, codes = R.crops(frames, boxes, [1, 1, 5], size=(9, 7))
    assert codes.tolist() == [R.OK, R.EMPTY, R.EMPTY] and out.shape == (3, 3, 9, 7)
    assert not out[1:].any()
    # a 9x7 box into a 9x7 output: the frame's own pixels, channels reversed, normalised
    px = frames[1, 6:15, 5:12, ::-1]
    assert np.array_equal(out[0], R.normalise(px, R.IMAGENET_MEAN, R.IMAGENET_STD, False)
                          .transpose(2, 0, 1))
    nh, _ = R.crops(frames, boxes, [1, 1, 5], size=(9, 7), nhwc=True, swap_rb=False)
    assert np.array_equal(nh[0], R.normalise(frames[1, 6:15, 5:12], R.IMAGENET_MEAN,
                                             R.IMAGENET_STD, False))


@pytest.mark.parametrize("half", [False, True], ids=["float32", "half"])
def test_normalisation_matches_the_framework_on_the_cpu(half):
    """The reference's three expressions (base_backend.py:62-71) on the same resized uint8 crop,
    run by torch on the CPU: to(dtype), crops / 255.0, (crops - mean) / std with float32 mean and
    std tensors; with half the float32 result is cast back (inference_preprocess)."""
    import torch

    px = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)  # every value, every channel
    dtype = torch.half if half else torch.float
    crops = torch.empty((1, 3, 16, 16), dtype=dtype)
    crops[0] = torch.permute(torch.from_numpy(px).to(dtype=dtype), (2, 0, 1))
    crops = crops / 255.0
    mean_array = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std_array = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    crops = (crops - mean_array) / std_array
    assert crops.dtype == torch.float32
    if half:
        crops = crops.half()
    want = crops[0].permute(1, 2, 0).numpy()
    got = R.normalise(px, R.IMAGENET_MEAN, R.IMAGENET_STD, half)
    assert got.dtype == want.dtype
    assert np.array_equal(got.view(np.uint16 if half else np.uint32),
                          want.view(np.uint16 if half else np.uint32))


# ------------------------------------------------------------------------ header and bindings
def prototypes():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in
            re.finditer(r"\bint\s+(bx_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_matches_bindings():
    protos = prototypes()
    assert sorted(protos) == ["bx_reid_crops", "bx_reid_normalize"]
    for name, args in protos.items():
        assert name in N.EXPORTS
        argtypes, res = N._SIGS[name]
        assert res is C.c_int
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p, (name, p)
            elif p.startswith("float"):
                assert t is C.c_float, (name, p)
            elif p.startswith("int64_t"):
                assert t is C.c_int64, (name, p)
            else:
                assert p.startswith("int ") and t is C.c_int, (name, p)


def test_header_constants_match_python():
    from boxmot_amd import reid

    text = HEADER.read_text()
    val = lambda k: int(re.search(rf"\b{k}\s*=\s*(\d+)", text).group(1))  # noqa: E731
    assert (val("BX_CROP_OK"), val("BX_CROP_EMPTY")) == (reid.CROP_OK, reid.CROP_EMPTY)
    assert (val("BX_CROP_HALF"), val("BX_CROP_NHWC"), val("BX_CROP_SWAP_RB")) == (
        reid._HALF, reid._NHWC, reid._SWAP_RB)
    assert (R.OK, R.EMPTY) == (reid.CROP_OK, reid.CROP_EMPTY)
    assert R.IMAGENET_MEAN == reid.IMAGENET_MEAN and R.IMAGENET_STD == reid.IMAGENET_STD
    assert "unmeasured" in text and "not reproduced" in text


def test_argument_checks_run_before_any_launch():
    """BX_ERR_INVALID and the n == 0 no-op are decided on the host, so they answer here too.  (The
    pointers are never dereferenced: the calls that get past the checks have n == 0.)"""
    L = N.load()
    m, s = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    buf = (C.c_char * 64)()
    p = C.addressof(buf)

    def crops(F=1, H=4, W=4, n=0, oh=2, ow=2, mean=m, std=s, flags=4, frames=p, boxes=p, out=p):
        return L.bx_reid_crops(frames, F, H, W, boxes, None, n, oh, ow, *mean, *std, flags, out,
                               None, None)

    assert crops() == 0 and crops(frames=None, boxes=None, out=None) == 0  # n == 0: a no-op
    for bad in (dict(F=0), dict(H=0), dict(W=0), dict(oh=0), dict(ow=0), dict(n=-1),
                dict(std=(0.229, 0.0, 0.225)), dict(std=(0.229, float("nan"), 0.225)),
                dict(mean=(float("inf"), 0.0, 0.0)), dict(flags=8),
                dict(n=1, frames=None), dict(n=1, boxes=None), dict(n=1, out=None)):
        assert crops(**bad) == 1, bad
        assert L.bx_last_error()

    def norm(n=0, F=4, stride=4, src=p, dst=p):
        return L.bx_reid_normalize(src, 0, stride, n, F, dst, 0, None)

    assert norm() == 0 and norm(src=None, dst=None) == 0
    for bad in (dict(F=0), dict(n=-1), dict(stride=3), dict(n=1, src=None), dict(n=1, dst=None)):
        assert norm(**bad) == 1, bad


# ------------------------------------------------------------------------------------ Python
class _FakeModel:
    def __init__(self):
        self.calls = []

    def get_features(self, xyxys, img):
        self.calls.append((xyxys.copy(), img))
        return np.ones((len(xyxys), 4), np.float32)


def test_model_embs_helper():
    from boxmot_amd.trackers.basetracker import model_embs

    class T:
        model = None

    t, img = T(), np.zeros((4, 4, 3), np.uint8)
    dets = np.arange(12, dtype=np.float64).reshape(2, 6)
    given = np.zeros((2, 3))
    assert model_embs(t, dets, img, None) is None and model_embs(t, dets, img, given) is given
    t.model = _FakeModel()
    assert model_embs(t, dets, img, given) is given and not t.model.calls
    assert model_embs(t, dets[:0], img, None) is None and not t.model.calls
    assert model_embs(t, dets, img, None, wanted=False) is None and not t.model.calls
    e = model_embs(t, dets, img, None)
    assert e.shape == (2, 4) and np.array_equal(t.model.calls[0][0], dets[:, :4])
    assert t.model.calls[0][1] is img


def test_trackers_carry_a_model_slot():
    import boxmot_amd as B

    for cls in (B.BotSort, B.BoostTrack, B.StrongSort, B.DeepOcSort, B.HybridSort,
                B.DeepOcSortPerClass, B.HybridSortPerClass):
        assert cls.model is None


def test_front_end_without_a_device_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from boxmot_amd import ReidFrontEnd, crop_batch, normalize_features

    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(N.NativeUnavailable):
        crop_batch(img, np.array([[0, 0, 4, 4]], np.float32))
    with pytest.raises(N.NativeUnavailable):
        normalize_features(torch.zeros(2, 4))
    with pytest.raises(N.NativeUnavailable):
        ReidFrontEnd(lambda x: x)

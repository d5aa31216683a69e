"""The detector front end without a GPU: the numpy restatement (tests/det_ref.py) against the
definition of greedy NMS stated by brute force and against values worked out by hand, the header
against the binding table, the argument checks of det.py and of the C entry points (they run
before any device call), and the loud failure without a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from boxmot_amd import _native as N
from tests import det_ref as D

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "bxdet.h"


# ------------------------------------------------------------------------------- restatement
def kept_by_definition(boxes, cls, thr, agnostic):
    """Kept iff no earlier kept box of a comparable class has IoU > thr: the definition, with
    every earlier box looked at again for every box."""
    kept = []
    for i in range(len(boxes)):
        kept.append(not any(kept[j] and (agnostic or cls[j] == cls[i])
                            and D.iou(boxes[j], boxes[i]) > np.float32(thr) for j in range(i)))
    return [i for i, k in enumerate(kept) if k]


def grid_boxes(rng, n, span=12, side=6):
    """Boxes with small integer corners: many exact ties and many equal IoUs."""
    x1, y1 = rng.integers(0, span, n), rng.integers(0, span, n)
    w, h = rng.integers(0, side, n), rng.integers(0, side, n)  # (zero sizes among them)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)


@pytest.mark.parametrize("agnostic", [False, True], ids=["per-class", "agnostic"])
@pytest.mark.parametrize("thr", [0.0, 0.25, 0.5, 0.7])
def test_greedy_nms_is_the_definition(thr, agnostic):
    rng = np.random.default_rng([int(thr * 100), agnostic])
    for n in (1, 2, 17, 90):
        boxes = grid_boxes(rng, n)
        cls = rng.integers(0, 3, n)
        assert D.greedy_nms(boxes, cls, thr, agnostic) == kept_by_definition(boxes, cls, thr,
                                                                             agnostic)
    same = np.tile(np.array([[2, 2, 8, 8]], np.float32), (9, 1))  # identical boxes: one survives
    assert D.greedy_nms(same, np.zeros(9, int), thr, agnostic) == [0]
    smooth = rng.uniform(0, 40, (60, 2)).astype(np.float32)
    boxes = np.concatenate([smooth, smooth + rng.uniform(1, 25, (60, 2)).astype(np.float32)], 1)
    cls = rng.integers(0, 2, 60)
    assert D.greedy_nms(boxes, cls, thr, agnostic) == kept_by_definition(boxes, cls, thr, agnostic)


def test_chain_keeps_the_third_box():
    # a suppresses b (IoU 2/3), b alone would suppress c (2/3), a and c overlap by 1/3 only
    boxes = np.array([[0, 0, 10, 10], [2, 0, 12, 10], [4, 0, 14, 10]], np.float32)
    assert np.isclose(D.iou(boxes[0], boxes[1]), 8 / 12) and np.isclose(D.iou(boxes[0], boxes[2]),
                                                                        6 / 14)
    assert D.greedy_nms(boxes, [0, 0, 0], 0.5, False) == [0, 2]
    assert D.greedy_nms(boxes, [0, 1, 0], 0.5, False) == [0, 1, 2]
    assert D.greedy_nms(boxes, [0, 1, 0], 0.5, True) == [0, 2]


def test_iou_edges():
    a = np.array([0, 0, 4, 4], np.float32)
    assert D.iou(a, np.array([2, 0, 6, 4], np.float32)) == np.float32(8) / np.float32(24)
    assert D.iou(a, np.array([4, 0, 8, 4], np.float32)) == 0  # touching
    z = np.array([1, 1, 1, 1], np.float32)
    assert np.isnan(D.iou(z, z))  # 0 / 0: suppresses nothing
    assert D.greedy_nms(np.stack([z, z]), [0, 0], 0.0, True) == [0, 1]
    nan = np.array([np.nan, 0, 4, 4], np.float32)
    assert not D.iou(a, nan) > 0 and not D.iou(nan, a) > 0  # a NaN never wins a comparison


def test_order_ties_and_threshold():
    s = np.array([0.5, 0.9, 0.5, np.nan, 0.25, 0.9, -0.0, 0.24999], np.float32)
    assert D.candidates(s, 0.25) == [1, 5, 0, 2, 4]
    assert D.candidates(s, 0.0) == [1, 5, 0, 2, 4, 7, 6]
    pred = np.zeros((1, 3, 8), np.float32)
    pred[0, :, 4] = 1.0
    pred[0, 0, 5:] = [0.2, 0.7, 0.7]  # the first maximum
    pred[0, 1, 5:] = [0.1, np.nan, 0.9]  # a NaN counts as a maximum
    pred[0, 2, 5:] = [0.3, 0.1, 0.2]
    sc, cls = D.scores(pred[0])
    assert cls.tolist() == [1, 1, 0] and np.isnan(sc[1]) and sc[0] == np.float32(0.7)


def test_postprocess_caps_classes_and_offsets():
    # image 0: five far-apart boxes of classes 0, 1, 0, 1, 0 with falling scores; image 1: none;
    # image 2: two boxes on top of each other, classes 0 and 1
    pred = np.zeros((3, 5, 7), np.float32)
    for k in range(5):
        pred[0, k] = [20 * k + 5, 5, 4, 4, 1.0, 0.9 - 0.1 * k if k % 2 == 0 else 0,
                      0.9 - 0.1 * k if k % 2 else 0]
    pred[2, 0] = [5, 5, 4, 4, 1.0, 0.8, 0.1]
    pred[2, 1] = [5, 5, 4, 4, 1.0, 0.1, 0.6]
    d, off, anc, code = D.postprocess(pred, conf=0.05)
    assert off.tolist() == [0, 5, 5, 7] and anc.tolist() == [0, 1, 2, 3, 4, 0, 1] and not code.any()
    assert d[0].tolist() == [3, 3, 7, 7, np.float32(0.9), 0] and d[6, 5] == 1
    d, off, anc, code = D.postprocess(pred, conf=0.05, class_agnostic=True, classes=[1], ratio=2.0)
    assert off.tolist() == [0, 2, 2, 2] and anc.tolist() == [1, 3]  # (2, 1) was suppressed first
    assert d[0, :4].tolist() == [11.5, 1.5, 13.5, 3.5]
    d, off, anc, code = D.postprocess(pred, conf=0.05, cand_cap=3, max_det=2)
    assert off.tolist() == [0, 2, 2, 4] and anc.tolist() == [0, 1, 0, 1]
    assert code.tolist() == [D.CAND_OVERFLOW | D.MAX_DET, 0, 0]
    assert D.postprocess(pred[:, :0])[0].shape == (0, 6)


def test_letterbox_2x2_into_4x6_by_hand():
    # r = min(4 / 2, 6 / 2) = 2: the frame becomes 4 x 4 in the top left, columns 4 and 5 are
    # padding.  Per axis 2 -> 4 reads f = -0.25, 0.25, 0.75, 1.25: weights of the second pixel
    # 0, 1/4, 3/4, 1, and the blend rounds the exact bilinear value half up.
    frame = np.empty((2, 2, 3), np.uint8)
    frame[..., 0] = [[0, 100], [200, 40]]
    frame[..., 1] = 10
    frame[..., 2] = 250
    resized = np.array([[0, 25, 75, 100], [50, 59, 76, 85], [150, 126, 79, 55],
                        [200, 160, 80, 40]], np.float64)
    assert D.geometry(2, 2, (4, 6)) == (2.0, 4, 4)
    out, r = D.letterbox(frame, (4, 6), mean=None, std=None)
    assert r == 2.0 and out.shape == (1, 3, 4, 6) and out.dtype == np.float32
    pad = np.float32(114.0 / 255.0)
    assert np.array_equal(out[0, 2, :, :4], (resized / 255.0).astype(np.float32))  # BGR -> RGB
    assert np.all(out[0, 0, :, :4] == np.float32(250 / 255.0))
    assert np.all(out[0, 1, :, :4] == np.float32(10 / 255.0))
    assert np.all(out[0, :, :, 4:] == pad)
    # mean and std by output channel, in float64, one cast
    out, _ = D.letterbox(frame, (4, 6), swap_rb=False)
    assert np.array_equal(out[0, 0, :, :4],
                          ((resized / 255.0 - 0.485) / 0.229).astype(np.float32))
    assert np.all(out[0, 2, :, 4:] == np.float32((114.0 / 255.0 - 0.406) / 0.225))
    half, _ = D.letterbox(frame, (4, 6), half=True)
    assert half.dtype == np.float16
    assert np.array_equal(half, D.letterbox(frame, (4, 6))[0].astype(np.float16))
    # the limiting axis changes: 2 x 2 into 6 x 4 pads rows
    tall, r = D.letterbox(frame, (6, 4), mean=None, std=None)
    assert r == 2.0 and np.all(tall[0, :, 4:, :] == pad)
    assert np.array_equal(tall[0, :, :4, :], D.letterbox(frame, (4, 6), mean=None, std=None)[0][0, :, :, :4])


# ------------------------------------------------------------------------ header and bindings
def prototypes():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in
            re.finditer(r"\bint\s+(bx_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_matches_bindings():
    protos = prototypes()
    assert sorted(protos) == ["bx_det_letterbox", "bx_det_postprocess", "bx_det_scratch_bytes"]
    assert N.HEADER_DET == HEADER and "bx_det.hip" in N.SOURCES
    for name, args in protos.items():
        assert name in N.EXPORTS
        argtypes, res = N._SIGS[name]
        assert res is C.c_int
        params = [" ".join(a.split()) for a in args.split(",")]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            if p.startswith("size_t *"):
                assert t is C.POINTER(C.c_size_t), (name, p)
            elif "*" in p:
                assert t is C.c_void_p, (name, p)
            elif p.startswith("double"):
                assert t is C.c_double, (name, p)
            elif p.startswith("float"):
                assert t is C.c_float, (name, p)
            elif p.startswith("int64_t"):
                assert t is C.c_int64, (name, p)
            else:
                assert p.startswith("int ") and t is C.c_int, (name, p)


def test_header_constants_match_python():
    from boxmot_amd import det

    text = HEADER.read_text()
    val = lambda k: int(re.search(rf"\b{k}\s*=\s*(\d+)", text).group(1))  # noqa: E731
    assert (val("BX_LB_HALF"), val("BX_LB_SWAP_RB"), val("BX_LB_NO_MEAN"), val("BX_LB_NO_STD")) \
        == (det._LB_HALF, det._LB_SWAP_RB, det._LB_NO_MEAN, det._LB_NO_STD)
    assert (val("BX_DET_PRED_HALF"), val("BX_DET_AGNOSTIC")) == (det._PRED_HALF, det._AGNOSTIC)
    assert (val("BX_DET_CAND_OVERFLOW"), val("BX_DET_MAX_DET")) == (det.CAND_OVERFLOW, det.MAX_DET)
    assert (D.CAND_OVERFLOW, D.MAX_DET) == (det.CAND_OVERFLOW, det.MAX_DET)
    assert val("BX_DET_CAND_MAX") == det.CAND_MAX
    assert D.YOLOX_MEAN == det.YOLOX_MEAN and D.YOLOX_STD == det.YOLOX_STD
    assert text.count("unmeasured") >= 2  # cv2.resize, torchvision's offset form


def test_c_argument_checks_run_before_any_launch():
    """BX_ERR_INVALID and the F == 0 / B == 0 no-ops are decided on the host, so they answer here
    too.  (The pointers are never dereferenced: the calls that get past the checks launch
    nothing.)"""
    L = N.load()
    m, s = D.YOLOX_MEAN, D.YOLOX_STD
    buf = (C.c_char * 1024)()
    p = (C.addressof(buf) + 255) & ~255

    def lb(F=0, H=4, W=4, ih=8, iw=8, rh=8, rw=8, mean=m, std=s, flags=2, frames=p, out=p):
        return L.bx_det_letterbox(frames, F, H, W, ih, iw, rh, rw, *mean, *std, flags, out, None)

    assert lb() == 0 and lb(frames=None, out=None) == 0  # F == 0: a no-op
    assert lb(std=(0.2, 0.0, 0.2), flags=2 | 8) == 0     # std switched off: not looked at
    for bad in (dict(F=-1), dict(H=0), dict(W=0), dict(ih=0), dict(iw=0), dict(rh=0), dict(rh=9),
                dict(rw=0), dict(rw=9), dict(std=(0.2, 0.0, 0.2)),
                dict(std=(0.2, float("nan"), 0.2)), dict(mean=(float("inf"), 0.0, 0.0)),
                dict(flags=16), dict(F=1, frames=None), dict(F=1, out=None)):
        assert lb(**bad) == 1, bad
        assert L.bx_last_error()

    def pp(B=0, A=10, C_=1, rs=6, ims=60, conf=0.01, thr=0.7, cap=64, md=64, flags=0, pred=p,
           scratch=p, dets=p, off=p):
        return L.bx_det_postprocess(pred, B, A, C_, rs, ims, conf, thr, None, None, cap, md,
                                    flags, scratch, dets, off, None, None, None, None)

    assert pp() == 0 and pp(pred=None, scratch=None, dets=None, off=None) == 0  # B == 0
    for bad in (dict(B=-1), dict(A=-1), dict(C_=0), dict(rs=5), dict(ims=59), dict(conf=-0.1),
                dict(conf=1.5), dict(conf=float("nan")), dict(thr=-0.1), dict(thr=1.01),
                dict(cap=0), dict(cap=16385), dict(md=0), dict(flags=4), dict(B=1, pred=None),
                dict(B=1, scratch=None), dict(B=1, dets=None), dict(B=1, off=None),
                dict(B=1, scratch=p + 8)):
        assert pp(**bad) == 1, bad

    def need(B, A, cap):
        n = C.c_size_t(0)
        assert L.bx_det_scratch_bytes(B, A, cap, C.byref(n)) == 0
        return n.value

    assert need(0, 0, 1) % 256 == 0
    assert need(2, 1000, 256) > need(1, 1000, 256) > need(1, 1000, 64)
    assert need(1, 1025, 64) > need(1, 1024, 64) == need(1, 513, 64)  # keys: A to a power of two
    # the suppression matrix: one bit per pair of candidates, rows in whole blocks
    assert need(1, 1, 4096) - need(1, 1, 64) >= (4096 * 4096 - 64 * 64) // 8
    assert L.bx_det_scratch_bytes(1, 1, 0, C.byref(C.c_size_t(0))) == 1
    assert L.bx_det_scratch_bytes(1, 1, 64, None) == 1


# ------------------------------------------------------------------------------------ Python
def test_letterbox_arguments_are_checked_without_a_device():
    from boxmot_amd import det

    good = np.zeros((2, 8, 8, 3), np.uint8)
    for frames, size, kw in (
            (good.astype(np.float32), (16, 16), {}), (good[..., :2], (16, 16), {}),
            (good[0, 0], (16, 16), {}), (good, (0, 16), {}), (good, (16,), {}),
            (good, (16, 16), dict(std=(0.2, 0.0, 0.2))), (good, (16, 16), dict(mean=(0.1, 0.2))),
            (good, (16, 16), dict(mean=(0.1, np.inf, 0.2))), ([[1, 2, 3]], (16, 16), {})):
        with pytest.raises(ValueError):
            det.letterbox(frames, size, **kw)
    assert det.letterbox_geometry(1080, 1920, (800, 1440)) == (0.7407407407407407, 800, 1422)
    assert det.letterbox_geometry(48, 64, (7, 9))[1:] == (6, 9)


def test_postprocess_arguments_are_checked_without_a_device():
    from boxmot_amd import det

    good = np.zeros((2, 10, 6), np.float32)
    for pred, kw in ((good[0], {}), (good[..., :5], {}), (good, dict(cand_cap=0)),
                     (good, dict(cand_cap=det.CAND_MAX + 1)), (good, dict(max_det=0)),
                     (good, dict(conf=-0.01)), (good, dict(conf=1.01)), (good, dict(iou=-0.5)),
                     (good, dict(iou=2.0)), (good, dict(iou=float("nan"))), (None, {})):
        with pytest.raises(ValueError):
            det.postprocess(pred, **kw)
    assert det._class_flags([0, 2, 7], 3).tolist() == [1, 0, 1]
    assert det._class_flags(None, 3) is None
    with pytest.raises(ValueError):
        det._class_flags([0.5], 3)
    for kw in (dict(batch=0), dict(cand_cap=0), dict(max_det=0), dict(conf=2.0), dict(iou=-1.0),
               dict(input_size=(0, 8))):
        with pytest.raises(ValueError):
            det.DetFrontEnd(lambda x: x, **kw)


def test_exports():
    import boxmot_amd
    from boxmot_amd import det

    for name in ("DetFrontEnd", "letterbox", "postprocess"):
        assert name in boxmot_amd.__all__ and getattr(boxmot_amd, name) is getattr(det, name)


def test_front_end_without_a_device_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from boxmot_amd import DetFrontEnd, letterbox, postprocess

    with pytest.raises(N.NativeUnavailable):
        letterbox(np.zeros((8, 8, 3), np.uint8), (16, 16))
    with pytest.raises(N.NativeUnavailable):
        postprocess(torch.zeros(1, 4, 6))
    with pytest.raises(N.NativeUnavailable):
        DetFrontEnd(lambda x: x)

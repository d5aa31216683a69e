"""A numpy restatement of the ReID front end's contract (include/bxreid.h): the
oracle of tests/test_reid_host.py and tests/test_reid_gpu.py.

Written per box and per axis, the way the contract reads, with gathers instead of the kernel's
runs and tiles.  The bilinear rule is the one tests/ecc_ref.py restates for the ECC preprocessing
(index pair, 11-bit weight, one integer blend), with a ratio per axis.  OpenCV is not involved
anywhere.
"""
from __future__ import annotations

import numpy as np

OK, EMPTY = 0, 1
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def corners(box, H: int, W: int):
    """(x1, y1, x2, y2) ints of a float32 xyxy box in an H x W frame, or None for an empty crop."""
    b = np.asarray(box, np.float32)
    if not np.all(np.isfinite(b)):
        return None
    r = np.rint(b)  # half to even, in float32
    x1, x2 = (int(min(max(v, np.float32(0)), np.float32(W))) for v in (r[0], r[2]))
    y1, y2 = (int(min(max(v, np.float32(0)), np.float32(H))) for v in (r[1], r[3]))
    if x2 <= x1 or y2 <= y1:
        return None
    return x1, y1, x2, y2


def axis_taps(L: int, O: int):
    """(s0, s1, q) of every output index of an axis of crop length L and output length O."""
    f = (np.arange(O, dtype=np.float64) + 0.5) * float(L) / float(O) - 0.5
    fl = np.floor(f)
    a = f - fl
    lo, hi = fl < 0, fl >= L - 1
    s0 = np.where(lo, 0, np.where(hi, L - 1, fl)).astype(np.int64)
    a = np.where(lo | hi, 0.0, a)
    s1 = np.minimum(s0 + 1, L - 1)
    return s0, s1, np.rint(a * 2048.0).astype(np.int64)


def resize(crop: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """uint8 [h, w, C] -> uint8 [oh, ow, C]."""
    g = crop.astype(np.int64)
    x0, x1, qx = axis_taps(crop.shape[1], ow)
    y0, y1, qy = axis_taps(crop.shape[0], oh)
    qx, qy = qx[None, :, None], qy[:, None, None]
    g00, g01 = g[y0][:, x0], g[y0][:, x1]
    g10, g11 = g[y1][:, x0], g[y1][:, x1]
    v = (g00 * (2048 - qx) * (2048 - qy) + g01 * qx * (2048 - qy) + g10 * (2048 - qx) * qy
         + g11 * qx * qy + (1 << 21)) >> 22
    return v.astype(np.uint8)


def normalise(px: np.ndarray, mean, std, half: bool) -> np.ndarray:
    """uint8 [..., 3] -> float32 / float16 [..., 3]: every operation rounded once."""
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    u = px.astype(np.float32) / np.float32(255.0)
    if half:
        u = u.astype(np.float16).astype(np.float32)
    v = (u - m) / s
    return v.astype(np.float16) if half else v


def crops(frames, boxes, frame_of=None, size=(256, 128), half=False, nhwc=False,
          mean=IMAGENET_MEAN, std=IMAGENET_STD, swap_rb=True):
    """(out [n, 3, oh, ow] or [n, oh, ow, 3], codes int32 [n]) of uint8 frames [F, H, W, 3]."""
    frames = np.asarray(frames)
    F, H, W = frames.shape[:3]
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    n = boxes.shape[0]
    oh, ow = size
    out = np.zeros((n, oh, ow, 3), np.float16 if half else np.float32)
    codes = np.zeros(n, np.int32)
    for i in range(n):
        fr = 0 if frame_of is None else int(frame_of[i])
        c = corners(boxes[i], H, W) if 0 <= fr < F else None
        if c is None:
            codes[i] = EMPTY
            continue
        x1, y1, x2, y2 = c
        px = resize(frames[fr, y1:y2, x1:x2], oh, ow)
        if swap_rb:
            px = px[..., ::-1]
        out[i] = normalise(px, mean, std, half)
    return (out if nhwc else np.ascontiguousarray(out.transpose(0, 3, 1, 2))), codes


def unit_rows(x: np.ndarray) -> np.ndarray:
    """get_features' division; fp16 rows are widened first (the contract's documented choice)."""
    x = np.asarray(x)
    if x.dtype == np.float16:
        x = x.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.linalg.norm(x, axis=-1, keepdims=True)

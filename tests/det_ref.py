"""A numpy restatement of the detector front end's contract (include/bxdet.h): the
oracle of tests/test_det_host.py and tests/test_det_gpu.py.

Written per frame and per image, the way the contract reads.  The letterbox takes its resize from
tests/reid_ref.py (the rule of DESIGN.md 2.14 with a ratio per axis) and normalises with the
reference's own numpy lines on a float64 array; the post-process is a plain float32 loop over the
candidates in order.  Neither OpenCV nor torchvision is involved anywhere.
"""
from __future__ import annotations

import numpy as np

from tests import reid_ref as R

CAND_OVERFLOW, MAX_DET = 1, 2
YOLOX_MEAN = (0.485, 0.456, 0.406)
YOLOX_STD = (0.229, 0.224, 0.225)
PAD = 114.0

f32 = np.float32


def geometry(H: int, W: int, input_size):
    """(r, rh, rw): yolox_preprocess's ratio and resized size."""
    r = min(input_size[0] / H, input_size[1] / W)
    return r, int(H * r), int(W * r)


def letterbox(frames, input_size, half=False, mean=YOLOX_MEAN, std=YOLOX_STD, swap_rb=True):
    """(out [F, 3, in_h, in_w] float32 / float16, r) of uint8 frames [F, H, W, 3] (or one
    frame), line by line as the reference's yolox_preprocess with the resize restated."""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = frames[None]
    r, rh, rw = geometry(frames.shape[1], frames.shape[2], input_size)
    out = []
    for img in frames:
        padded_img = np.ones((input_size[0], input_size[1], 3)) * PAD
        resized_img = R.resize(img, rh, rw).astype(np.float32)
        padded_img[:rh, :rw] = resized_img
        if swap_rb:
            padded_img = padded_img[:, :, ::-1]
        padded_img /= 255.0
        if mean is not None:
            padded_img -= mean
        if std is not None:
            padded_img /= std
        padded_img = padded_img.transpose((2, 0, 1))
        padded_img = np.ascontiguousarray(padded_img, dtype=np.float32)
        out.append(padded_img.astype(np.float16) if half else padded_img)
    return np.stack(out), r


def scores(pred):
    """(score float32 [A], cls int [A]) of one image's rows (float16 widened first)."""
    p = np.asarray(pred).astype(np.float32)
    cls = np.argmax(p[:, 5:], axis=1)  # the first maximum; a NaN counts as one
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = p[:, 4] * p[np.arange(len(p)), 5 + cls]
    return s, cls


def corners(pred):
    """float32 [A, 4] xyxy."""
    p = np.asarray(pred).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        hw, hh = p[:, 2] / f32(2), p[:, 3] / f32(2)
        return np.stack([p[:, 0] - hw, p[:, 1] - hh, p[:, 0] + hw, p[:, 1] + hh], 1)


def candidates(score, conf):
    """Rows with score >= conf in the contract's order: descending score, ties by row."""
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero(score >= f32(conf))
    return sorted(idx.tolist(), key=lambda i: (-float(score[i]), i))


def iou(a, b):
    """float32 IoU of the earlier box a and the later box b, every operation rounded once."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        area_a = (a[2] - a[0]) * (a[3] - a[1])
        area_b = (b[2] - b[0]) * (b[3] - b[1])
        xx2 = b[2] if b[2] < a[2] else a[2]
        xx1 = b[0] if b[0] > a[0] else a[0]
        yy2 = b[3] if b[3] < a[3] else a[3]
        yy1 = b[1] if b[1] > a[1] else a[1]
        dw, dh = xx2 - xx1, yy2 - yy1
        iw = dw if dw > 0 else f32(0)
        ih = dh if dh > 0 else f32(0)
        inter = iw * ih
        return inter / ((area_a + area_b) - inter)


def iou_row(a, bs):
    """iou(a, b) for every later box b of bs [n, 4] at once: the same operations on arrays."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        area_a = (a[2] - a[0]) * (a[3] - a[1])
        area_b = (bs[:, 2] - bs[:, 0]) * (bs[:, 3] - bs[:, 1])
        xx2 = np.where(bs[:, 2] < a[2], bs[:, 2], a[2])
        xx1 = np.where(bs[:, 0] > a[0], bs[:, 0], a[0])
        yy2 = np.where(bs[:, 3] < a[3], bs[:, 3], a[3])
        yy1 = np.where(bs[:, 1] > a[1], bs[:, 1], a[1])
        dw, dh = xx2 - xx1, yy2 - yy1
        inter = np.where(dw > 0, dw, f32(0)) * np.where(dh > 0, dh, f32(0))
        return inter / ((area_a + area_b) - inter)


def greedy_nms(boxes, cls, thr, agnostic):
    """Indices kept of boxes already in order: one pass, each kept box marks what it removes."""
    boxes, cls = np.asarray(boxes, f32).reshape(-1, 4), np.asarray(cls)
    n = len(boxes)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        with np.errstate(invalid="ignore"):
            hit = iou_row(boxes[i], boxes[i + 1:]) > f32(thr)
        if not agnostic:
            hit &= cls[i + 1:] == cls[i]
        removed[i + 1:] |= hit
    return keep


def postprocess(pred, conf=0.01, iou_thr=0.7, class_agnostic=False, classes=None, ratio=None,
                cand_cap=4096, max_det=None):
    """(dets [sum N, 6] float32, det_off int32 [B + 1], anchor_of int32 [sum N], code int32 [B])
    of pred [B, A, 5 + C]; ratio a float or one per image."""
    pred = np.asarray(pred)
    B = pred.shape[0]
    max_det = cand_cap if max_det is None else max_det
    ratio = np.ones(B, f32) if ratio is None else np.broadcast_to(
        np.asarray(ratio, np.float64).astype(f32), (B,))
    rows, anchors, off, code = [], [], [0], np.zeros(B, np.int32)
    for b in range(B):
        s, cls = scores(pred[b])
        box = corners(pred[b])
        cand = candidates(s, conf)
        if len(cand) > cand_cap:
            code[b] |= CAND_OVERFLOW
            cand = cand[:cand_cap]
        keep = [cand[k] for k in greedy_nms(box[cand], cls[cand], iou_thr, class_agnostic)]
        if classes is not None:
            keep = [i for i in keep if int(cls[i]) in set(classes)]
        if len(keep) > max_det:
            code[b] |= MAX_DET
            keep = keep[:max_det]
        for i in keep:
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                rows.append(np.concatenate([box[i] / ratio[b],
                                            [s[i] + f32(0), f32(cls[i])]]).astype(f32))
            anchors.append(i)
        off.append(len(rows))
    dets = np.stack(rows) if rows else np.empty((0, 6), f32)
    return dets, np.asarray(off, np.int32), np.asarray(anchors, np.int32), code

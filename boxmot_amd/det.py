"""The detector front end on the GPU: everything between the camera frames and the ``dets`` /
``det_off`` pair the engines take except the detector network itself.

Reference stages replaced (``boxmot/engine/detectors/yolox.py``): ``yolox_preprocess`` (:197-226,
one ``cv2.resize`` per frame into a padded float64 image, then the normalisation) and the
post-process (:249-276): YOLOX's published ``postprocess`` (score filter and torchvision's batched
NMS, which this platform's torch build does not ship) and the rescale to image coordinates.  Both
run in libbxassoc.so (``include/bxdet.h``; DESIGN.md 2.27 is the contract): one launch letterboxes
every camera's frame into the network's input tensor, a memset and five launches turn the
network's output into the rows of every camera, ``det_off`` included.  The network is the
caller's own torch module; backbones, weights and the Ultralytics glue are out of scope
(DESIGN.md 7).

``DetFrontEnd`` ties the two around a model: ``front(img)`` returns the ``dets`` of
``tracker.update(dets, img)``; ``detect(frames)`` is the many-camera path, which stays on the
device without a host synchronisation.  There is no CPU fallback: without the library or a HIP
device the calls raise ``NativeUnavailable``.

Agreement of the bilinear rule with OpenCV's ``INTER_LINEAR`` and agreement with torchvision's
coordinate-offset form of batched NMS on borderline pairs are unmeasured.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

YOLOX_MEAN = (0.485, 0.456, 0.406)
YOLOX_STD = (0.229, 0.224, 0.225)

# bits of an image's code (include/bxdet.h)
CAND_OVERFLOW, MAX_DET = 1, 2
CAND_MAX = 16384
_LB_HALF, _LB_SWAP_RB, _LB_NO_MEAN, _LB_NO_STD = 1, 2, 4, 8
_PRED_HALF, _AGNOSTIC = 1, 2


def _device():
    """(library, torch) or NativeUnavailable."""
    import torch  # (first, as everywhere in the package: one HIP runtime per process)

    L = N.load()
    if N.device_count() == 0 or not torch.cuda.is_available():
        raise N.NativeUnavailable("the detector front end needs a HIP device")
    return L, torch


def _three(v, what):
    v = np.asarray(v, np.float64).reshape(-1)
    if v.size != 3:
        raise ValueError(f"{what} must have 3 entries")
    return [float(x) for x in v]


def letterbox_geometry(H: int, W: int, input_size):
    """``(r, rh, rw)`` of an H x W frame in ``input_size = (in_h, in_w)``: the reference's
    ``r = min(in_h / H, in_w / W)`` and the resized size ``int(H * r), int(W * r)``."""
    in_h, in_w = int(input_size[0]), int(input_size[1])
    if H < 1 or W < 1 or in_h < 1 or in_w < 1:
        raise ValueError("frame and input sizes must be at least 1")
    r = min(in_h / H, in_w / W)
    rh, rw = int(H * r), int(W * r)
    if not (1 <= rh <= in_h and 1 <= rw <= in_w):
        raise ValueError(f"a {H}x{W} frame does not letterbox into {in_h}x{in_w}")
    return r, rh, rw


def _check_lb_args(shape, dtype, input_size, mean, std):
    """The checks of ``letterbox`` that need no device; returns (F, H, W, in_h, in_w, r, rh, rw,
    mean, std)."""
    if np.dtype(dtype) != np.uint8:
        raise ValueError("frames must be uint8")
    if len(shape) == 3:
        shape = (1,) + tuple(shape)
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError(f"frames must be [F, H, W, 3], got {tuple(shape)}")
    if len(input_size) != 2:
        raise ValueError("input_size must be (in_h, in_w)")
    F, H, W = (int(s) for s in shape[:3])
    r, rh, rw = letterbox_geometry(H, W, input_size)
    mean = None if mean is None else _three(mean, "mean")
    std = None if std is None else _three(std, "std")
    if mean is not None and not np.all(np.isfinite(mean)):
        raise ValueError("mean must be finite")
    if std is not None and not (np.all(np.isfinite(std)) and all(std)):
        raise ValueError("std must be finite and non-zero")
    return F, H, W, int(input_size[0]), int(input_size[1]), r, rh, rw, mean, std


def letterbox(frames, input_size, half=False, mean=YOLOX_MEAN, std=YOLOX_STD, swap_rb=True,
              out=None):
    """The reference's ``yolox_preprocess`` of every frame in one launch on the current stream.

    frames: uint8 BGR ``[F, H, W, 3]`` (or ``[H, W, 3]``), a CUDA tensor or a numpy array (copied
    up first).  Returns ``(tensor, r)``: the CUDA tensor ``[F, 3, in_h, in_w]``, float32 or, with
    ``half``, float16, and the ratio ``r`` (a Python float; every frame of a call has one size, so
    one ratio).  ``mean`` / ``std`` may be ``None``, as in the reference.  With CUDA frames
    nothing here synchronises the host with the device.
    """
    is_np = isinstance(frames, np.ndarray)
    if not is_np:
        import torch

        if not isinstance(frames, torch.Tensor):
            raise ValueError("frames must be a numpy array or a CUDA tensor of uint8")
        if frames.dtype != torch.uint8:
            raise ValueError("frames must be uint8")
    F, H, W, in_h, in_w, r, rh, rw, mean, std = _check_lb_args(
        tuple(frames.shape), np.uint8 if not is_np else frames.dtype, input_size, mean, std)
    L, torch = _device()
    from .engine import _current_stream

    if is_np:
        frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    elif not frames.is_cuda:
        raise ValueError("frames must be a numpy array or a CUDA tensor of uint8")
    frames = frames.reshape(F, H, W, 3).contiguous()
    dtype = torch.float16 if half else torch.float32
    shape = (F, 3, in_h, in_w)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device="cuda")
    elif (not out.is_cuda or out.dtype != dtype or tuple(out.shape) != shape
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous CUDA {dtype} tensor of shape {shape}")
    flags = ((_LB_HALF if half else 0) | (_LB_SWAP_RB if swap_rb else 0)
             | (_LB_NO_MEAN if mean is None else 0) | (_LB_NO_STD if std is None else 0))
    N.check(L.bx_det_letterbox(
        frames.data_ptr(), F, H, W, in_h, in_w, rh, rw, *(mean or (0.0, 0.0, 0.0)),
        *(std or (1.0, 1.0, 1.0)), flags, out.data_ptr(), _current_stream()), "bx_det_letterbox")
    return out, r


def _check_pp_args(shape, conf, iou, cand_cap, max_det):
    """The checks of ``postprocess`` that need no device; returns (B, A, C, max_det)."""
    if len(shape) != 3 or shape[2] < 6:
        raise ValueError(f"pred must be [B, A, 5 + C] with C >= 1, got {tuple(shape)}")
    if not 1 <= int(cand_cap) <= CAND_MAX:
        raise ValueError(f"cand_cap must lie in 1..{CAND_MAX}")
    max_det = int(cand_cap) if max_det is None else int(max_det)
    if max_det < 1:
        raise ValueError("max_det must be at least 1")
    for name, v in (("conf", conf), ("iou", iou)):
        if not 0.0 <= float(v) <= 1.0:  # (a NaN fails too)
            raise ValueError(f"{name} must lie in [0, 1]")
    return int(shape[0]), int(shape[1]), int(shape[2]) - 5, max_det


def _class_flags(classes, C_):
    """int32 [C] of 0 / 1 from a list of class indices (numpy), or None."""
    if classes is None:
        return None
    idx = np.asarray(classes).reshape(-1)
    if idx.size and (not np.issubdtype(idx.dtype, np.integer) or idx.min() < 0):
        raise ValueError("classes must be non-negative integers")
    ok = np.zeros(C_, np.int32)
    ok[idx[idx < C_].astype(np.int64)] = 1  # (a class the head does not have never shows up)
    return ok


_scratch = {}  # the scratch of each stream, grown to the largest call


def _scratch_for(L, torch, B, A, cand_cap):
    need = C.c_size_t(0)
    N.check(L.bx_det_scratch_bytes(B, A, cand_cap, C.byref(need)), "bx_det_scratch_bytes")
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < need.value:
        # (reuse from call to call is safe because the work of one stream runs in order)
        buf = _scratch[key] = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")
    return buf


def postprocess(pred, conf=0.01, iou=0.7, class_agnostic=False, classes=None, ratio=None,
                cand_cap=4096, max_det=None, out=None, frame_of=None):
    """Score filter, batched NMS and rescale of every image on the current stream.

    pred: CUDA ``[B, A, 5 + C]`` float32 or float16 (``cx, cy, w, h, obj, cls...`` in input
    pixels; the last dimension contiguous, any row or image stride).  ``classes``: class indices
    to report (a list, or a CUDA int32 ``[C]`` tensor of 0 / 1 flags), applied after NMS as the
    reference does.  ``ratio``: a float, or a CUDA float32 ``[B]`` tensor; coordinates are divided
    by it.  ``max_det`` defaults to ``cand_cap`` (no further limit).

    Returns ``(dets, det_off, anchor_of, code)``, all CUDA: ``dets [B * max_det, 6]`` float32 of
    which rows ``det_off[b]..det_off[b + 1]`` are image b's (rows from ``det_off[B]`` on are not
    written), ``det_off [B + 1]`` int32, ``anchor_of [B * max_det]`` int32 (the row of ``pred``),
    ``code [B]`` int32 (``CAND_OVERFLOW | MAX_DET``).  ``out``: the same four to fill;
    ``frame_of``: an int32 ``[B * max_det]`` tensor that receives each row's image.  With CUDA
    arguments nothing here synchronises the host with the device.
    """
    shape = tuple(getattr(pred, "shape", ()))
    B, A, C_, max_det = _check_pp_args(shape, conf, iou, cand_cap, max_det)
    L, torch = _device()
    from .engine import _current_stream

    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        raise ValueError("pred must be a CUDA tensor")
    if pred.dtype not in (torch.float32, torch.float16):
        pred = pred.float()
    # (the stride of a dimension of one element means nothing, and need not be a valid one)
    if B and A and (pred.stride(2) != 1 or (A > 1 and pred.stride(1) < 5 + C_)
                    or (B > 1 and pred.stride(0) < (A - 1) * pred.stride(1) + 5 + C_)):
        pred = pred.contiguous()
    row_stride = int(pred.stride(1)) if B and A > 1 else 5 + C_
    img_stride = int(pred.stride(0)) if B > 1 and A else A * row_stride
    if isinstance(classes, torch.Tensor):
        if (not classes.is_cuda or classes.dtype != torch.int32 or tuple(classes.shape) != (C_,)
                or not classes.is_contiguous()):
            raise ValueError(f"a classes tensor must be contiguous CUDA int32 of shape ({C_},)")
    elif classes is not None:
        classes = torch.from_numpy(_class_flags(classes, C_)).cuda()
    if ratio is not None and not isinstance(ratio, torch.Tensor):
        ratio = torch.full((B,), float(ratio), dtype=torch.float32, device="cuda")
    if ratio is not None and (not ratio.is_cuda or ratio.dtype != torch.float32
                              or tuple(ratio.shape) != (B,) or not ratio.is_contiguous()):
        raise ValueError(f"a ratio tensor must be contiguous CUDA float32 of shape ({B},)")
    rows = B * max_det
    want = (((rows, 6), torch.float32), ((B + 1,), torch.int32), ((rows,), torch.int32),
            ((B,), torch.int32))
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device="cuda") for s, d in want)
        if B == 0:
            out[1].zero_()
    else:
        if len(out) != 4:
            raise ValueError("out must be (dets, det_off, anchor_of, code)")
        for t, (s, d) in zip(out, want):
            if not t.is_cuda or t.dtype != d or tuple(t.shape) != s or not t.is_contiguous():
                raise ValueError(f"out needs a contiguous CUDA {d} tensor of shape {s}")
    if frame_of is not None and (not frame_of.is_cuda or frame_of.dtype != torch.int32
                                 or tuple(frame_of.shape) != (rows,)
                                 or not frame_of.is_contiguous()):
        raise ValueError(f"frame_of must be a contiguous CUDA int32 tensor of shape ({rows},)")
    dets, det_off, anchor_of, code = out
    scratch = _scratch_for(L, torch, B, A, int(cand_cap))
    flags = (_PRED_HALF if pred.dtype == torch.float16 else 0) | (_AGNOSTIC if class_agnostic
                                                                  else 0)
    N.check(L.bx_det_postprocess(
        pred.data_ptr(), B, A, C_, row_stride, img_stride, float(conf), float(iou),
        None if classes is None else classes.data_ptr(),
        None if ratio is None else ratio.data_ptr(), int(cand_cap), max_det, flags,
        scratch.data_ptr(), dets.data_ptr(), det_off.data_ptr(), anchor_of.data_ptr(),
        None if frame_of is None else frame_of.data_ptr(), code.data_ptr(), _current_stream()),
        "bx_det_postprocess")
    # (the launches are asynchronous; a tensor made above is freed on return, and the caching
    # allocator hands its memory out again only to work queued on this stream after them)
    return dets, det_off, anchor_of, code


class DetFrontEnd:
    """Letterbox, the caller's detector and the post-process as one object.

    ``model`` is any callable that takes a CUDA tensor ``[B, 3, h, w]`` (``half``: float16) and
    returns ``[B, A, 5 + C]`` decoded to input pixels, as a YOLOX head in eval mode does, or a
    list or tuple whose first item is that.  ``input_size`` is ``(h, w)``; ``batch`` bounds the
    frames per model call.  ``mean`` / ``std`` / ``swap_rb`` are ``letterbox``'s (the reference's
    defaults).  ``max_det`` defaults to ``cand_cap``.
    """

    def __init__(self, model, input_size=(800, 1440), conf=0.01, iou=0.7, class_agnostic=False,
                 classes=None, half: bool = False, cand_cap: int = 4096, max_det=None,
                 batch: int = 64, mean=YOLOX_MEAN, std=YOLOX_STD, swap_rb: bool = True):
        if batch < 1:
            raise ValueError("batch must be at least 1")
        _check_pp_args((1, 1, 6), conf, iou, cand_cap, max_det)
        letterbox_geometry(1, 1, input_size)
        _device()
        self.model = model
        self.input_size = (int(input_size[0]), int(input_size[1]))
        self.conf, self.iou, self.class_agnostic = float(conf), float(iou), bool(class_agnostic)
        self.classes = None if classes is None else [int(c) for c in classes]
        self.half, self.cand_cap, self.batch = bool(half), int(cand_cap), int(batch)
        self.max_det = self.cand_cap if max_det is None else int(max_det)
        self.mean, self.std, self.swap_rb = mean, std, bool(swap_rb)
        # per stream: the input buffer; per (B, r) / C: the small device constants, so that a
        # steady stream of calls makes no host-to-device copy
        self._bufs, self._ratios, self._class_ok = {}, {}, {}

    def _predict(self, frames):
        """(pred [B, A, 5 + C], r) of CUDA frames [B, H, W, 3]."""
        import torch

        key = torch.cuda.current_stream().cuda_stream
        n = int(frames.shape[0])
        preds, r = [], 1.0
        for lo in range(0, n, self.batch):
            hi = min(n, lo + self.batch)
            buf = self._bufs.get(key)
            if buf is None or buf.shape[0] < hi - lo:
                buf = self._bufs[key] = torch.empty(
                    (hi - lo, 3) + self.input_size, device="cuda",
                    dtype=torch.float16 if self.half else torch.float32)
            x, r = letterbox(frames[lo:hi], self.input_size, self.half, self.mean, self.std,
                             self.swap_rb, out=buf[:hi - lo])
            y = self.model(x)
            if isinstance(y, (list, tuple)):
                y = y[0]
            preds.append(y)
        return (preds[0] if len(preds) == 1 else torch.cat(preds)), r

    def detect(self, frames, frame_of=None):
        """The many-camera path: CUDA uint8 BGR frames ``[B, H, W, 3]``, one per camera.
        Returns ``postprocess``'s ``(dets, det_off, anchor_of, code)`` in image coordinates:
        ``dets`` / ``det_off`` are what ``Engine.step`` and ``OcsortEngine.step`` take, and
        ``dets[:, :4]`` with a ``frame_of`` tensor (int32 ``[B * max_det]``, filled when given)
        what ``ReidFrontEnd.features`` takes.  Runs under ``torch.no_grad()``; nothing
        synchronises the host (the first call of a batch size or frame size uploads two small
        constants)."""
        import torch

        if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise ValueError("detect() takes CUDA frames (front(img) takes numpy)")
        if frames.dim() != 4 or int(frames.shape[0]) < 1:
            raise ValueError(f"frames must be [B, H, W, 3] with B >= 1, got {tuple(frames.shape)}")
        with torch.no_grad():
            pred, r = self._predict(frames)
            if pred.dim() != 3 or pred.shape[0] != frames.shape[0]:
                raise ValueError(f"the model returned {tuple(pred.shape)} for "
                                 f"{int(frames.shape[0])} frames")
            B, C_ = int(pred.shape[0]), int(pred.shape[2]) - 5
            dev = torch.cuda.current_device()
            ratio = self._ratios.get((dev, B, r))
            if ratio is None:
                ratio = self._ratios[(dev, B, r)] = torch.full(
                    (B,), r, dtype=torch.float32, device="cuda")
            ok = None
            if self.classes is not None:
                ok = self._class_ok.get((dev, C_))
                if ok is None and C_ >= 1:
                    ok = self._class_ok[(dev, C_)] = torch.from_numpy(
                        _class_flags(self.classes, C_)).cuda()
            return postprocess(pred, self.conf, self.iou, self.class_agnostic, ok, ratio,
                               self.cand_cap, self.max_det, frame_of=frame_of)

    def __call__(self, img):
        """One BGR image ``[H, W, 3]`` uint8 (numpy) to its detections, numpy float32 ``[N, 6]``
        (``x1, y1, x2, y2, score, cls``): the ``dets`` of ``tracker.update(dets, img)``;
        ``np.empty((0, 6), np.float32)`` for none."""
        import torch

        img = np.ascontiguousarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("img must be a uint8 [H, W, 3] array")
        dets, det_off, _, _ = self.detect(torch.from_numpy(img).cuda()[None])
        n = int(det_off[1])
        return dets[:n].cpu().numpy() if n else np.empty((0, 6), np.float32)

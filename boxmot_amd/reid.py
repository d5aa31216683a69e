"""The ReID front end on the GPU: everything between the frames and the embeddings except the
network itself.

Reference stages replaced (``boxmot/appearance/backends/base_backend.py``): ``get_crops`` (:34-73,
a host loop with one ``cv2.resize`` and one host-to-device copy per box, then the normalisation)
and the division by ``np.linalg.norm`` that ends ``get_features`` (:84).  Both run in
libbxassoc.so (``include/bxreid.h``; DESIGN.md 2.15 is the contract): one launch cuts, resizes and
normalises every box of every camera straight into the network's input tensor, one launch turns
the network's output into the unit rows the engines take.  The network is the caller's own torch
module; weights and backbones are out of scope.

``ReidFrontEnd`` ties the two around a model: ``get_features(xyxys, img)`` is the reference's call
(assign the object to ``tracker.model`` and ``tracker.update(dets, img)`` works without ``embs``);
``features(frames, boxes, frame_of)`` is the many-camera path, which stays on the device without a
host synchronisation.  There is no CPU fallback: without the library or a HIP device the calls
raise ``NativeUnavailable``.

Agreement of the bilinear rule with OpenCV's ``INTER_LINEAR`` is unmeasured, and the float16 norm
numpy takes of float16 features is not reproduced: fp16 features are widened to float32 first
(DESIGN.md 2.15).
"""
from __future__ import annotations

import numpy as np

from . import _native as N

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# per-box result codes (include/bxreid.h)
CROP_OK, CROP_EMPTY = 0, 1
_HALF, _NHWC, _SWAP_RB = 1, 2, 4


def _device():
    """(library, torch) or NativeUnavailable."""
    import torch  # (first, as everywhere in the package: one HIP runtime per process)

    L = N.load()
    if N.device_count() == 0 or not torch.cuda.is_available():
        raise N.NativeUnavailable("the ReID front end needs a HIP device")
    return L, torch


def _three(v, what):
    v = np.asarray(v, np.float32).reshape(-1)
    if v.size != 3:
        raise ValueError(f"{what} must have 3 entries")
    return [float(x) for x in v]


def crop_batch(frames, boxes, frame_of=None, size=(256, 128), half=False, nhwc=False,
               mean=IMAGENET_MEAN, std=IMAGENET_STD, swap_rb=True, out=None, codes=None):
    """Cut, resize and normalise every box in one launch on the current stream.

    frames: uint8 ``[F, H, W, 3]`` (or ``[H, W, 3]``), boxes: ``[n, 4]`` xyxy, frame_of: the frame
    of each box (``None``: all in frame 0); each a CUDA tensor or a numpy array (copied up first;
    boxes are cast to float32).  Returns the CUDA tensor ``[n, 3, h, w]`` (``nhwc``:
    ``[n, h, w, 3]``) with ``size = (h, w)``, float32 or, with ``half``, float16.  ``out`` /
    ``codes`` (int32 ``[n]``: ``CROP_OK`` / ``CROP_EMPTY``, an empty crop is an all-zero row) are
    filled when given.  With CUDA inputs nothing here synchronises the host with the device.
    """
    L, torch = _device()
    from .engine import _current_stream

    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8:
        raise ValueError("frames must be a numpy array or a CUDA tensor of uint8")
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be [F, H, W, 3], got {tuple(frames.shape)}")
    frames = frames.contiguous()
    F, H, W = (int(s) for s in frames.shape[:3])
    if isinstance(boxes, torch.Tensor):
        boxes = boxes.to(device="cuda", dtype=torch.float32)
    else:
        boxes = torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).cuda()
    boxes = boxes.reshape(-1, 4).contiguous()
    n = int(boxes.shape[0])
    if frame_of is not None:
        if isinstance(frame_of, torch.Tensor):
            frame_of = frame_of.to(device="cuda", dtype=torch.int32)
        else:
            frame_of = torch.from_numpy(np.ascontiguousarray(frame_of, np.int32)).cuda()
        frame_of = frame_of.reshape(-1).contiguous()
        if int(frame_of.shape[0]) != n:
            raise ValueError(f"{n} boxes but {int(frame_of.shape[0])} frame indices")
    h, w = int(size[0]), int(size[1])
    shape = (n, h, w, 3) if nhwc else (n, 3, h, w)
    dtype = torch.float16 if half else torch.float32
    if out is None:
        out = torch.empty(shape, dtype=dtype, device="cuda")
    elif (not out.is_cuda or out.dtype != dtype or tuple(out.shape) != shape
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous CUDA {dtype} tensor of shape {shape}")
    if codes is not None and (not codes.is_cuda or codes.dtype != torch.int32
                              or tuple(codes.shape) != (n,) or not codes.is_contiguous()):
        raise ValueError(f"codes must be a contiguous CUDA int32 tensor of shape ({n},)")
    flags = (_HALF if half else 0) | (_NHWC if nhwc else 0) | (_SWAP_RB if swap_rb else 0)
    N.check(L.bx_reid_crops(
        frames.data_ptr(), F, H, W, boxes.data_ptr(),
        None if frame_of is None else frame_of.data_ptr(), n, h, w, *_three(mean, "mean"),
        *_three(std, "std"), flags, out.data_ptr(),
        None if codes is None else codes.data_ptr(), _current_stream()), "bx_reid_crops")
    # (the launch is asynchronous; a copy or cast made above is freed on return, and the caching
    # allocator hands its memory out again only to work queued on this stream after the kernel)
    return out


def normalize_features(feats, out_dtype=None, out=None):
    """Rows of a CUDA tensor ``[n, F]`` (float32 or float16, any row stride) divided by their
    norm, as ``features / np.linalg.norm(features, axis=-1, keepdims=True)`` computes them in
    float32 (float16 rows are widened first).  Returns a CUDA tensor of ``out_dtype``
    (``torch.float32``, the default, or ``torch.float64``: the exact widening)."""
    L, torch = _device()
    from .engine import _current_stream

    if out_dtype is None:
        out_dtype = torch.float32 if out is None else out.dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError("out_dtype must be torch.float32 or torch.float64")
    if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
        raise ValueError("feats must be a CUDA tensor")
    if feats.dim() != 2 or feats.shape[1] < 1:
        raise ValueError(f"feats must be [n, F] with F >= 1, got {tuple(feats.shape)}")
    if feats.dtype not in (torch.float32, torch.float16):
        feats = feats.float()
    n, F = int(feats.shape[0]), int(feats.shape[1])
    if n and (feats.stride(1) != 1 or feats.stride(0) < F):
        feats = feats.contiguous()
    if out is None:
        out = torch.empty((n, F), dtype=out_dtype, device="cuda")
    elif (not out.is_cuda or out.dtype != out_dtype or tuple(out.shape) != (n, F)
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous CUDA {out_dtype} tensor of shape {(n, F)}")
    N.check(L.bx_reid_normalize(
        feats.data_ptr(), int(feats.dtype == torch.float16), int(feats.stride(0)) if n else F, n,
        F, out.data_ptr(), int(out_dtype == torch.float64), _current_stream()),
        "bx_reid_normalize")
    return out


class ReidFrontEnd:
    """Crops, the caller's network and the unit rows, as one object with the reference backend's
    ``get_features(xyxys, img)``.

    ``model`` is any callable that takes a CUDA tensor ``[N, 3, h, w]`` (``nhwc``:
    ``[N, h, w, 3]``; ``half``: float16) and returns ``[N, F]``, or a list or tuple whose first
    item is that.  ``input_shape`` is ``(h, w)``: ``(256, 128)`` for most of the reference's
    models, ``(384, 128)`` for its ``lmbn`` ones.  ``batch`` bounds the crops per model call, and
    with it the crop buffer.
    """

    def __init__(self, model, input_shape=(256, 128), half: bool = False, nhwc: bool = False,
                 batch: int = 1024, mean=IMAGENET_MEAN, std=IMAGENET_STD, swap_rb: bool = True):
        if batch < 1:
            raise ValueError("batch must be at least 1")
        _device()
        self.model = model
        self.input_shape = (int(input_shape[0]), int(input_shape[1]))
        self.half, self.nhwc, self.batch = bool(half), bool(nhwc), int(batch)
        self.mean, self.std, self.swap_rb = mean, std, bool(swap_rb)
        # the crop buffer of each stream, grown to the largest chunk.  Reusing it from chunk to
        # chunk is safe because the work of one stream runs in order (the next crops are written
        # after the model has read the last); calls made on different streams get different buffers
        self._bufs = {}

    def _crops(self, frames, boxes, frame_of, codes):
        import torch

        n = int(boxes.shape[0])
        key = torch.cuda.current_stream().cuda_stream
        buf = self._bufs.get(key)
        if buf is None or buf.shape[0] < n:
            h, w = self.input_shape
            shape = (n, h, w, 3) if self.nhwc else (n, 3, h, w)
            buf = self._bufs[key] = torch.empty(
                shape, dtype=torch.float16 if self.half else torch.float32, device="cuda")
        return crop_batch(frames, boxes, frame_of, self.input_shape, self.half, self.nhwc,
                          self.mean, self.std, self.swap_rb, out=buf[:n], codes=codes)

    def features(self, frames, boxes, frame_of=None, out=None):
        """The many-camera path: frames uint8 ``[F, H, W, 3]``, boxes ``[n, 4]`` and frame_of
        ``[n]`` (or ``None``) CUDA tensors.  Returns ``(feats, codes)``: float32 unit rows
        ``[n, F]`` and int32 ``[n]`` (``CROP_EMPTY`` marks a box that had no pixels; its crop was
        all zeros, so its row is whatever the model makes of that).  Runs under
        ``torch.no_grad()`` in chunks of ``batch`` crops; nothing synchronises the host."""
        import torch

        for t in (frames, boxes) + (() if frame_of is None else (frame_of,)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError("features() takes CUDA tensors (get_features takes numpy)")
        boxes = boxes.reshape(-1, 4)
        n = int(boxes.shape[0])
        codes = torch.empty(n, dtype=torch.int32, device="cuda")
        with torch.no_grad():
            for lo in range(0, n, self.batch):
                hi = min(n, lo + self.batch)
                crops = self._crops(frames, boxes[lo:hi],
                                    None if frame_of is None else frame_of[lo:hi], codes[lo:hi])
                y = self.model(crops)
                if isinstance(y, (list, tuple)):
                    y = y[0]
                y = y.reshape(hi - lo, -1)
                if out is None:
                    out = torch.empty((n, int(y.shape[1])), dtype=torch.float32, device="cuda")
                normalize_features(y, out=out[lo:hi])
        if out is None:  # no boxes: the width is unknown
            out = torch.empty((0, 0), dtype=torch.float32, device="cuda")
        return out, codes

    def get_features(self, xyxys, img):
        """The reference's ``get_features``: boxes ``[N, 4]`` (numpy) and one BGR image
        ``[H, W, 3]`` uint8 to the float32 unit rows ``[N, F]`` as a numpy array; ``np.array([])``
        for no boxes.  Raises ``ValueError`` naming the first box whose crop is empty (the
        reference's ``cv2.resize`` raises there)."""
        import torch

        xyxys = np.asarray(xyxys)
        if xyxys.size == 0:
            return np.array([])
        img = np.ascontiguousarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("img must be a uint8 [H, W, 3] array")
        boxes = np.ascontiguousarray(xyxys, np.float32).reshape(-1, 4)
        feats, codes = self.features(torch.from_numpy(img).cuda()[None],
                                     torch.from_numpy(boxes).cuda())
        codes = codes.cpu().numpy()
        if codes.any():
            k = int(np.flatnonzero(codes)[0])
            raise ValueError(f"box {k} {boxes[k].tolist()} has an empty crop in a "
                             f"{img.shape[0]}x{img.shape[1]} image")
        return feats.cpu().numpy()

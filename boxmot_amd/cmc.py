"""Camera-motion compensation on the GPU: the ECC image alignment of ``motion/cmc/ecc.py`` and
the sparse optical flow of ``motion/cmc/sof.py``.

Reference stage replaced (``boxmot/motion/cmc/ecc.py:63-128`` with ``base_cmc.py:27-43``): grey
conversion, the resize to ``scale`` and ``cv2.findTransformECC`` against the previous frame, on the
host, once per frame.  Here both stages run in libbxassoc.so (``include/bxcmc.h``; DESIGN.md 2.14
is the contract): a preprocessing kernel in exact integer arithmetic and one persistent workgroup
per camera that runs the whole ECC iteration in fp64.  ``ECC`` is the reference's class for one
camera (``tracker.cmc = ECC()``); ``EccBatch`` aligns many cameras per call and returns the warps
as the device tensor the engines' ``warps`` argument takes (no host synchronisation when its
inputs are on the device).  ``EccChain`` aligns many consecutive frames of a camera per call and
``warp_table`` builds from it the warps of every stepped frame of a set of sequences, for the file
flow (``motio.run_sequences``).  There is no CPU fallback: without the
library or a HIP device the calls raise ``NativeUnavailable``.

``SOF`` / ``SofBatch`` replace ``motion/cmc/sof.py:64-160`` the same way (``include/bxsof.h``;
DESIGN.md 2.17 is the contract): Shi-Tomasi keypoints, pyramidal Lucas-Kanade tracking with one
wave per keypoint and a similarity fitted by a deterministic consensus, with the pyramids and the
keypoints of every camera resident on the device.  ``SofChain`` runs many consecutive frames of
a camera per call and ``sof_warp_table`` builds the file flow's warps from it.

Agreement with OpenCV's own ``findTransformECC``, ``goodFeaturesToTrack``,
``calcOpticalFlowPyrLK`` and ``estimateAffinePartial2D`` is unmeasured.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

# cv2's values
MOTION_TRANSLATION, MOTION_EUCLIDEAN, MOTION_AFFINE, MOTION_HOMOGRAPHY = 0, 1, 2, 3

# per-stream result codes (include/bxcmc.h); NO_FRAME is EccBatch's own: the stream was not listed
OK, FIRST_FRAME, NOT_CONVERGED, NO_FRAME = 0, 1, 2, 3


def _check_mode(warp_mode) -> int:
    if warp_mode == MOTION_HOMOGRAPHY:
        raise NotImplementedError("MOTION_HOMOGRAPHY is not supported: no engine takes a 3x3 warp")
    if warp_mode not in (MOTION_TRANSLATION, MOTION_EUCLIDEAN, MOTION_AFFINE):
        raise ValueError(f"unknown warp_mode {warp_mode!r}")
    return int(warp_mode)


def _scale_arg(scale) -> float:
    """The C ABI's scale: 0 for 'no resize' (None, or a ratio >= 1)."""
    if scale is None:
        return 0.0
    if isinstance(scale, (list, tuple, np.ndarray)):
        raise NotImplementedError("scale as [W, H] is not supported (the reference's preprocess "
                                  "cannot take it either): give a ratio")
    s = float(scale)
    if not s > 0:
        raise ValueError(f"scale must be positive, got {scale!r}")
    return 0.0 if s >= 1 else s


def work_size(H: int, W: int, scale) -> tuple:
    """(h, w) of the working image of an H x W frame: round-half-even of the scaled sides."""
    s = _scale_arg(scale)
    if s == 0.0:
        return int(H), int(W)
    return int(round(H * s)), int(round(W * s))


def _frame_dims(shape, grayscale: bool):
    """(n, H, W, channels) of a frame batch [n, H, W, 3] or [n, H, W]."""
    if len(shape) == 3:
        return int(shape[0]), int(shape[1]), int(shape[2]), 1
    if len(shape) == 4 and shape[3] in (1, 3):
        if shape[3] == 3 and not grayscale:
            raise NotImplementedError("ECC aligns single-channel images: grayscale=False needs "
                                      "grey frames")
        return int(shape[0]), int(shape[1]), int(shape[2]), int(shape[3])
    raise ValueError(f"frames must be [n, H, W, 3] or [n, H, W], got {tuple(shape)}")


class _Handle:
    """One ``bx_ecc`` handle."""

    def __init__(self, n_streams: int, max_h: int, max_w: int):
        import torch  # (first, as everywhere in the package: one HIP runtime per process)

        self._h = C.c_void_p()
        self._L = N.load()
        if N.device_count() == 0 or not torch.cuda.is_available():
            raise N.NativeUnavailable("ECC needs a HIP device")
        self.n_streams, self.max_h, self.max_w = int(n_streams), int(max_h), int(max_w)
        N.check(self._L.bx_ecc_create(self.n_streams, self.max_h, self.max_w, C.byref(self._h)),
                "bx_ecc_create")

    def close(self):
        if self._h:
            self._L.bx_ecc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream: int = -1):
        from .engine import _current_stream

        N.check(self._L.bx_ecc_reset(self._h, int(stream), _current_stream()), "bx_ecc_reset")

    def status(self) -> int:
        st = C.c_int(0)
        N.check(self._L.bx_ecc_status(self._h, C.byref(st)), "bx_ecc_status")
        return st.value

    def state(self, stream: int = 0, planes: bool = True):
        """(has_prev, grey uint8 [h, w], gx float32 [h, w], gy float32 [h, w]) of a stream: its
        previous image and the gradients of the last frame it was given (synchronises)."""
        hp, hh, ww = C.c_int(0), C.c_int(0), C.c_int(0)
        cap = self.max_h * self.max_w
        g = np.zeros(cap, np.uint8)
        gx, gy = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        N.check(self._L.bx_ecc_state_host(
            self._h, int(stream), C.byref(hp), C.byref(hh), C.byref(ww),
            g.ctypes.data if planes else None, gx.ctypes.data if planes else None,
            gy.ctypes.data if planes else None), "bx_ecc_state_host")
        h, w = hh.value, ww.value
        if not planes or not hp.value:
            return bool(hp.value), None, None, None
        cut = lambda a: a[: h * w].reshape(h, w).copy()  # noqa: E731
        return True, cut(g), cut(gx), cut(gy)


class EccBatch:
    """ECC for ``n_streams`` cameras: one ``apply`` aligns a frame of each listed stream to that
    stream's previous frame, all on the current stream.  With device inputs (frames a CUDA tensor,
    ``streams`` ``None`` or a CUDA tensor, ``init_warps`` ``None`` or a CUDA tensor) nothing inside
    synchronises the host with the device: two launches and a few device fills are enqueued.  A
    numpy ``frames`` array, a list of ``streams`` or host ``init_warps`` are copied to the device
    first, and that copy waits for the stream.

    ``max_h`` / ``max_w`` bound the working image (after the resize); left ``None`` they are taken
    from the first frames.  The other arguments are ``ECC``'s.
    """

    def __init__(self, n_streams: int, warp_mode: int = MOTION_TRANSLATION, eps: float = 1e-5,
                 max_iter: int = 100, scale=0.15, align: bool = False, grayscale: bool = True,
                 max_h: int | None = None, max_w: int | None = None):
        if align:
            raise NotImplementedError("align=True (prev_img_aligned) is not supported")
        if n_streams < 1:
            raise ValueError("n_streams must be at least 1")
        self.n_streams = int(n_streams)
        self.warp_mode, self.eps, self.max_iter = warp_mode, float(eps), int(max_iter)
        self.scale, self.grayscale = scale, grayscale
        self._cap = (max_h, max_w)
        self._handle = None
        self._all = None  # device arange(n_streams)
        self._eye = None  # device [n_streams, 6] identity warps

    def _ensure(self, H: int, W: int) -> _Handle:
        if self._handle is None:
            h, w = work_size(H, W, self.scale)
            self._handle = _Handle(self.n_streams, self._cap[0] or h, self._cap[1] or w)
        return self._handle

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None

    def reset(self, stream: int = -1):
        """Forget the previous image of one stream (default: of all)."""
        if self._handle is not None:
            self._handle.reset(stream)

    def status(self) -> int:
        return 0 if self._handle is None else self._handle.status()

    def state(self, stream: int = 0):
        if self._handle is None:
            return False, None, None, None
        return self._handle.state(stream)

    def apply(self, frames, streams=None, init_warps=None):
        """frames: numpy array or CUDA uint8 tensor ``[n, H, W, 3]`` (BGR) or ``[n, H, W]``
        (grey); streams: the stream of each frame (default ``0..n-1``), all different.  A list or
        numpy ``streams`` is checked here (range, duplicates: ``ValueError``).  A CUDA tensor
        cannot be read without a synchronisation, so it is not checked: an index out of range
        skips that frame and latches ``status()``; an index listed twice is undefined behaviour
        (two workgroups race on that stream's images; the results of that stream are garbage, the
        accesses stay in bounds).

        Returns CUDA tensors over all streams: warps float64 ``[n_streams, 6]`` (row-major 2x3,
        the engines' ``warps`` argument), rho float64, iterations int32, code int32 ``[n_streams]``
        (``OK`` / ``FIRST_FRAME`` / ``NOT_CONVERGED``; ``NO_FRAME`` with the identity warp for a
        stream that was not listed).  ``init_warps`` (``[n_streams, 6]``, working scale) starts
        the iterations elsewhere than at the identity.
        """
        import torch

        from .engine import _current_stream

        mode = _check_mode(self.warp_mode)
        scale = _scale_arg(self.scale)
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8:
                raise ValueError("frames must be uint8")
            n, H, W, ch = _frame_dims(frames.shape, self.grayscale)
            hd = self._ensure(H, W)
            frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        else:
            if frames.dtype != torch.uint8 or not frames.is_cuda:
                raise ValueError("frames must be a numpy array or a CUDA uint8 tensor")
            n, H, W, ch = _frame_dims(frames.shape, self.grayscale)
            hd = self._ensure(H, W)
            frames = frames.contiguous()
        S = self.n_streams
        if streams is None:
            if n > S:
                raise ValueError(f"capacity exceeded: {n} frames for {S} streams")
            if self._all is None:
                self._all = torch.arange(S, dtype=torch.int32, device="cuda")
            sd = self._all
        elif isinstance(streams, torch.Tensor) and streams.is_cuda:
            sd = streams.to(torch.int32).contiguous()
        else:
            sh = np.asarray(streams, np.int64).reshape(-1)
            if sh.size and (sh.min() < 0 or sh.max() >= S):
                raise ValueError("invalid argument: stream index out of range")
            if np.unique(sh).size != sh.size:
                raise ValueError("invalid argument: a stream is listed twice")
            sd = torch.from_numpy(sh.astype(np.int32)).cuda()
        if streams is not None and sd.numel() != n:
            raise ValueError(f"{n} frames but {sd.numel()} stream indices")
        iw = None
        if init_warps is not None:
            iw = torch.as_tensor(np.asarray(init_warps, np.float64).reshape(S, 6)
                                 if not isinstance(init_warps, torch.Tensor) else init_warps)
            iw = iw.to(device="cuda", dtype=torch.float64).reshape(S, 6).contiguous()
        if self._eye is None:  # device fills only: a tensor built from host values would copy
            self._eye = torch.zeros(S, 6, dtype=torch.float64, device="cuda")  # and synchronise
            self._eye[:, 0] = 1.0
            self._eye[:, 4] = 1.0
        warps = self._eye.clone()
        rho = torch.zeros(S, dtype=torch.float64, device="cuda")
        iters = torch.zeros(S, dtype=torch.int32, device="cuda")
        code = torch.full((S,), NO_FRAME, dtype=torch.int32, device="cuda")
        N.check(hd._L.bx_ecc_apply(
            hd._h, n, H, W, ch, frames.data_ptr(), sd.data_ptr(), mode, self.eps, self.max_iter,
            scale, None if iw is None else iw.data_ptr(), warps.data_ptr(), rho.data_ptr(),
            iters.data_ptr(), code.data_ptr(), _current_stream()), "bx_ecc_apply")
        self._keep = (frames, sd, iw)  # alive until the next call: the launches are asynchronous
        return warps, rho, iters, code


class ECC:
    """The reference's ``ECC`` (``motion/cmc/ecc.py``): ``apply(img, dets)`` returns the 2x3
    float32 warp from the previous frame to this one, the identity on the first frame and when the
    iteration does not converge.  ``dets`` is ignored, as in the reference.  One camera; the device
    handle is built at the first frame from the image size.  ``last`` holds the float64 warp, rho,
    the iteration count and the code of the last call."""

    def __init__(self, warp_mode: int = MOTION_TRANSLATION, eps: float = 1e-5, max_iter: int = 100,
                 scale: float = 0.15, align: bool = False, grayscale: bool = True) -> None:
        self.align = align
        self.grayscale = grayscale
        self.scale = scale
        self.warp_mode = warp_mode
        self.termination_criteria = (3, max_iter, eps)  # cv2.TERM_CRITERIA_EPS | _COUNT
        self.prev_img_aligned = None
        self.last = None
        self._handle = None

    @property
    def prev_img(self):
        """The previous grey image at working scale (None before the first frame)."""
        if self._handle is None:
            return None
        return self._handle.state(0)[1]

    def reset(self):
        if self._handle is not None:
            self._handle.reset(0)

    def apply(self, img: np.ndarray, dets: np.ndarray = None, init_warp=None) -> np.ndarray:
        mode = _check_mode(self.warp_mode)
        if self.align:
            raise NotImplementedError("align=True (prev_img_aligned) is not supported")
        scale = _scale_arg(self.scale)
        img = np.ascontiguousarray(img)
        if img.dtype != np.uint8:
            raise ValueError("img must be uint8")
        if img.ndim == 2:
            H, W, ch = img.shape[0], img.shape[1], 1
        else:
            _, H, W, ch = _frame_dims((1,) + img.shape, self.grayscale)
        if self._handle is None:
            h, w = work_size(H, W, self.scale)
            self._handle = _Handle(1, h, w)
        hd = self._handle
        _, max_iter, eps = self.termination_criteria
        streams = np.zeros(1, np.int32)
        warp = np.zeros((1, 6), np.float64)
        rho = np.zeros(1, np.float64)
        iters, code = np.zeros(1, np.int32), np.zeros(1, np.int32)
        iw = None if init_warp is None else np.ascontiguousarray(init_warp, np.float64).reshape(1, 6)
        from .engine import _current_stream

        N.check(hd._L.bx_ecc_apply_host(
            hd._h, 1, H, W, ch, img.ctypes.data, streams.ctypes.data, mode, float(eps),
            int(max_iter), scale, None if iw is None else iw.ctypes.data, warp.ctypes.data,
            rho.ctypes.data, iters.ctypes.data, code.ctypes.data, _current_stream()),
            "bx_ecc_apply_host")
        self.last = {"warp": warp.reshape(2, 3).copy(), "rho": float(rho[0]),
                     "iterations": int(iters[0]), "code": int(code[0])}
        return warp.reshape(2, 3).astype(np.float32)


# ------------------------------------------------------------------------------ chained ECC
class EccChain:
    """ECC over many consecutive frames of a camera per call (``bx_ecc_apply_chain``; DESIGN.md
    2.19): frame i of a call is aligned to frame i - 1 when both are of one stream, otherwise to
    its stream's stored previous image, one workgroup per pair.  Warps, rho, iterations, codes and
    the streams' final state are bit for bit those of ``EccBatch.apply`` called one frame at a
    time.

    ``batch`` is the ``EccBatch`` whose handle the chain shares: ``chain.batch.apply`` is the
    plain apply on the same streams, and the two may be mixed.  ``max_frames`` bounds a call's
    frames (``reserve`` grows it); the other arguments are ``EccBatch``'s."""

    def __init__(self, n_streams: int, max_frames: int = 64, warp_mode: int = MOTION_TRANSLATION,
                 eps: float = 1e-5, max_iter: int = 100, scale=0.15, grayscale: bool = True,
                 max_h: int | None = None, max_w: int | None = None):
        if max_frames < 1:
            raise ValueError("max_frames must be at least 1")
        self.batch = EccBatch(n_streams, warp_mode, eps, max_iter, scale, False, grayscale,
                              max_h, max_w)
        self.n_streams = self.batch.n_streams
        self.max_frames = int(max_frames)
        self._reserved = 0
        self._keep = None

    def _ensure(self, H: int, W: int) -> _Handle:
        hd = self.batch._ensure(H, W)
        if self._reserved < self.max_frames:
            N.check(hd._L.bx_ecc_chain_reserve(hd._h, self.max_frames), "bx_ecc_chain_reserve")
            self._reserved = self.max_frames
        return hd

    def reserve(self, max_frames: int):
        """Room for ``max_frames`` frames per call (never shrinks)."""
        self.max_frames = max(self.max_frames, int(max_frames))
        if self.batch._handle is not None:
            self._ensure(0, 0)

    def close(self):
        self.batch.close()
        self._reserved = 0

    def reset(self, stream: int = -1):
        self.batch.reset(stream)

    def status(self) -> int:
        return self.batch.status()

    def state(self, stream: int = 0):
        return self.batch.state(stream)

    def _frames(self, frames):
        import torch

        b = self.batch
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8:
                raise ValueError("frames must be uint8")
            dims = _frame_dims(frames.shape, b.grayscale)
            return torch.from_numpy(np.ascontiguousarray(frames)).cuda(), dims
        if frames.dtype != torch.uint8 or not frames.is_cuda:
            raise ValueError("frames must be a numpy array or a CUDA uint8 tensor")
        return frames.contiguous(), _frame_dims(frames.shape, b.grayscale)

    def apply(self, frames, streams, dst=None, out=None):
        """frames: numpy array or CUDA uint8 tensor ``[n, H, W, 3]`` (BGR) or ``[n, H, W]``
        (grey); streams: the stream of each frame, the frames of one stream adjacent and in time
        order.  A list or numpy ``streams`` is checked here (range, adjacency: ``ValueError``); a
        CUDA tensor is not: an index out of range skips its frame and latches ``status()``, a
        stream in two separate groups is undefined behaviour (in bounds).

        Frame i writes row ``dst[i]`` (default: row i) of ``out``, the tuple ``(warps [rows, 6]
        float64, rho [rows] float64, iterations [rows] int32, code [rows] int32)`` of CUDA
        tensors; other rows are untouched.  Without ``out`` fresh ``[n]``-row tensors are made
        (identity, 0, 0, ``NO_FRAME``).  Returns ``out``.  With device inputs nothing inside
        synchronises the host with the device."""
        import torch

        from .engine import _current_stream

        b = self.batch
        mode = _check_mode(b.warp_mode)
        scale = _scale_arg(b.scale)
        frames, (n, H, W, ch) = self._frames(frames)
        hd = self._ensure(H, W)
        S = self.n_streams
        if isinstance(streams, torch.Tensor) and streams.is_cuda:
            sd = streams.to(torch.int32).contiguous()
        else:
            sh = np.asarray(streams, np.int64).reshape(-1)
            if sh.size and (sh.min() < 0 or sh.max() >= S):
                raise ValueError("invalid argument: stream index out of range")
            starts = sh[np.r_[True, sh[1:] != sh[:-1]]] if sh.size else sh
            if np.unique(starts).size != starts.size:
                raise ValueError("invalid argument: the frames of a stream are not adjacent")
            sd = torch.from_numpy(sh.astype(np.int32)).cuda()
        if sd.numel() != n:
            raise ValueError(f"{n} frames but {sd.numel()} stream indices")
        if out is None:
            if dst is not None:
                raise ValueError("dst needs the out tensors it points into")
            warps = torch.zeros(n, 6, dtype=torch.float64, device="cuda")
            warps[:, 0] = 1.0
            warps[:, 4] = 1.0
            out = (warps, torch.zeros(n, dtype=torch.float64, device="cuda"),
                   torch.zeros(n, dtype=torch.int32, device="cuda"),
                   torch.full((n,), NO_FRAME, dtype=torch.int32, device="cuda"))
        warps, rho, iters, code = out
        rows = int(rho.numel())
        want = ((warps, torch.float64, rows * 6), (rho, torch.float64, rows),
                (iters, torch.int32, rows), (code, torch.int32, rows))
        for t, dt, ne in want:
            if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == ne):
                raise ValueError("out must be contiguous CUDA tensors: warps [rows, 6] float64, "
                                 "rho float64, iterations int32, code int32 [rows]")
        dd = None
        if dst is None:
            if n > rows:
                raise ValueError(f"{n} frames but {rows} result rows")
        elif isinstance(dst, torch.Tensor) and dst.is_cuda:
            dd = dst.to(torch.int64).contiguous()
        else:
            dh = np.asarray(dst, np.int64).reshape(-1)
            if dh.size and (dh.min() < 0 or dh.max() >= rows):
                raise ValueError("invalid argument: dst row out of range")
            dd = torch.from_numpy(dh).cuda()
        if dd is not None and dd.numel() != n:
            raise ValueError(f"{n} frames but {dd.numel()} dst rows")
        N.check(hd._L.bx_ecc_apply_chain(
            hd._h, n, H, W, ch, frames.data_ptr(), sd.data_ptr(),
            None if dd is None else dd.data_ptr(), mode, b.eps, b.max_iter, scale,
            warps.data_ptr(), rho.data_ptr(), iters.data_ptr(), code.data_ptr(),
            _current_stream()), "bx_ecc_apply_chain")
        self._keep = (frames, sd, dd)  # alive until the next call: the launches are asynchronous
        return out

    def apply_host(self, frames, streams):
        """The host entry (``bx_ecc_apply_chain_host``): numpy ``frames`` and ``streams`` in,
        numpy ``(warps [n, 6], rho, iterations, code)`` out, one synchronisation.  The library
        itself refuses a stream index out of range or a stream whose frames are not adjacent
        (``ValueError``, nothing launched)."""
        from .engine import _current_stream

        b = self.batch
        mode = _check_mode(b.warp_mode)
        scale = _scale_arg(b.scale)
        frames = np.ascontiguousarray(frames)
        if frames.dtype != np.uint8:
            raise ValueError("frames must be uint8")
        n, H, W, ch = _frame_dims(frames.shape, b.grayscale)
        sh = np.ascontiguousarray(np.asarray(streams).reshape(-1), np.int32)
        if sh.size != n:
            raise ValueError(f"{n} frames but {sh.size} stream indices")
        hd = self._ensure(H, W)
        warps, rho = np.zeros((n, 6), np.float64), np.zeros(n, np.float64)
        iters, code = np.zeros(n, np.int32), np.zeros(n, np.int32)
        N.check(hd._L.bx_ecc_apply_chain_host(
            hd._h, n, H, W, ch, frames.ctypes.data, sh.ctypes.data, mode, b.eps, b.max_iter,
            scale, warps.ctypes.data, rho.ctypes.data, iters.ctypes.data, code.ctypes.data,
            _current_stream()), "bx_ecc_apply_chain_host")
        return warps, rho, iters, code


NOT_STEPPED = -1  # a warp table's code for a frame its sequence is not stepped at


def chain_plan(stepped, sizes, chunk: int = 64) -> list:
    """The calls that chain every stepped frame of S sequences, a pure function of its arguments.

    stepped: per sequence a bool mask over its iterated frames; sizes: per sequence its frame
    size, any hashable (``None`` is fine for a sequence that is never stepped).  Returns a list of
    ``(size, seq, t)`` with ``seq`` and ``t`` int64 arrays of at most ``chunk`` entries: frame
    ``t[i]`` of sequence ``seq[i]`` is frame i of that call.  Sequences are grouped by size, in
    order of first appearance; within a group the sequences' stepped frames are laid end to end
    (sequence by sequence, each in time order) and cut every ``chunk`` frames, so a call never
    mixes sizes, each sequence is one contiguous run of a call, and a sequence cut by a call's
    end goes on at the start of the next one, from the state the first left."""
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    if len(stepped) != len(sizes):
        raise ValueError("one size per sequence")
    groups = {}
    for k, m in enumerate(stepped):
        ts = np.flatnonzero(np.asarray(m, bool).reshape(-1))
        if ts.size:
            groups.setdefault(sizes[k], []).append((k, ts))
    calls = []
    for size, members in groups.items():
        seq = np.concatenate([np.full(ts.size, k, np.int64) for k, ts in members])
        t = np.concatenate([ts for _, ts in members]).astype(np.int64)
        for a in range(0, seq.size, chunk):
            calls.append((size, seq[a: a + chunk], t[a: a + chunk]))
    return calls


class WarpTable:
    """The warps of every iterated frame of S sequences in device memory, frame-major:
    ``warps [T, S, 6]`` float64, ``rho [T, S]`` float64, ``iterations`` and ``code [T, S]`` int32
    (CUDA tensors).  The warps of the sequences ``[seq0, seq0 + nseq)`` at frame index t are the
    contiguous block at ``(t * S + seq0) * 6``: what every engine's ``step(..., warps, ...)``
    takes.  A frame its sequence is not stepped at holds the identity and ``NOT_STEPPED``."""

    def __init__(self, warps, rho, iterations, code):
        self.warps, self.rho, self.iterations, self.code = warps, rho, iterations, code
        self.n_frames, self.n_seq = int(warps.shape[0]), int(warps.shape[1])

    def host(self) -> dict:
        """Numpy copies (synchronises)."""
        return {k: getattr(self, k).cpu().numpy() for k in ("warps", "rho", "iterations", "code")}

    def close(self):
        self.warps = self.rho = self.iterations = self.code = None


def _empty_table(T: int, S: int) -> WarpTable:
    import torch

    warps = torch.zeros(T, S, 6, dtype=torch.float64, device="cuda")
    warps[:, :, 0] = 1.0
    warps[:, :, 4] = 1.0
    return WarpTable(warps, torch.zeros(T, S, dtype=torch.float64, device="cuda"),
                     torch.zeros(T, S, dtype=torch.int32, device="cuda"),
                     torch.full((T, S), NOT_STEPPED, dtype=torch.int32, device="cuda"))


def warp_table(images, stepped, *, warp_mode: int = MOTION_TRANSLATION, eps: float = 1e-5,
               max_iter: int = 100, scale=0.15, chunk: int = 64) -> WarpTable:
    """The ECC warp of every stepped frame of S sequences, computed by chained calls of at most
    ``chunk`` frames (``chain_plan``) and left in device memory.

    images: per sequence a uint8 array ``[frames, H, W]`` or ``[frames, H, W, 3]`` (BGR) over
    the frames the sequence iterates, or a callable ``index -> frame`` (``[H, W]`` or ``[H, W,
    3]``, index the position among the iterated frames); only stepped frames are read.  stepped:
    per sequence a bool mask over its iterated frames.  The template of a stepped frame is the
    previous stepped frame of its sequence (the reference runs its CMC inside ``update`` only);
    a sequence's first stepped frame has code ``FIRST_FRAME``.  The defaults are ``ECC()``'s.  A
    call stages ``chunk`` whole frames on the host and on the device."""
    mode = _check_mode(warp_mode)
    _scale_arg(scale)
    S = len(images)
    stepped, fetch, sizes = _table_frames(images, stepped)
    calls = chain_plan(stepped, sizes, chunk)
    tab = _empty_table(max([m.size for m in stepped] + [0]), S)
    if not calls:
        return tab
    work = [work_size(sz[0], sz[1], scale) for sz in sizes if sz is not None]
    ecc = EccChain(S, max_frames=max(c[1].size for c in calls), warp_mode=mode, eps=eps,
                   max_iter=max_iter, scale=scale, max_h=max(h for h, _ in work),
                   max_w=max(w for _, w in work))
    try:
        out = (tab.warps.view(-1, 6), tab.rho.view(-1), tab.iterations.view(-1),
               tab.code.view(-1))
        for size, seq, t in calls:
            frames = np.stack([fetch(int(k), int(x)) for k, x in zip(seq, t)])
            if frames.shape[1:] != tuple(size):
                raise ValueError(f"sequence {int(seq[0])}: frames of more than one size")
            ecc.apply(frames, seq, dst=t * S + seq, out=out)
        st = ecc.status()  # (synchronises: the staged frames may go)
        if st != 0:
            raise RuntimeError(f"ecc status {st}")
    finally:
        ecc.close()
    return tab


# per-stream result codes of the sparse optical flow (include/bxsof.h); SOF_NO_FRAME is SofBatch's
# own: the stream was not listed
SOF_OK, SOF_FIRST_FRAME, SOF_TOO_FEW, SOF_NO_MODEL, SOF_NO_KEYPOINTS, SOF_NO_FRAME = 0, 1, 2, 3, 4, 5
SOF_MAX_CORNERS, SOF_MAX_LEVELS, SOF_HYPOTHESES = 1024, 4, 256


class _SofHandle:
    """One ``bx_sof`` handle."""

    def __init__(self, n_streams: int, max_h: int, max_w: int):
        import torch  # (first, as everywhere in the package: one HIP runtime per process)

        self._h = C.c_void_p()
        self._L = N.load()
        if N.device_count() == 0 or not torch.cuda.is_available():
            raise N.NativeUnavailable("SOF needs a HIP device")
        self.n_streams, self.max_h, self.max_w = int(n_streams), int(max_h), int(max_w)
        N.check(self._L.bx_sof_create(self.n_streams, self.max_h, self.max_w, C.byref(self._h)),
                "bx_sof_create")
        nb = C.c_size_t(0)
        N.check(self._L.bx_sof_pyramid_bytes(self._h, C.byref(nb)), "bx_sof_pyramid_bytes")
        self.pyramid_bytes = int(nb.value)

    def close(self):
        if self._h:
            self._L.bx_sof_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream: int = -1):
        from .engine import _current_stream

        N.check(self._L.bx_sof_reset(self._h, int(stream), _current_stream()), "bx_sof_reset")

    def status(self) -> int:
        st = C.c_int(0)
        N.check(self._L.bx_sof_status(self._h, C.byref(st)), "bx_sof_status")
        return st.value

    def state(self, stream: int = 0):
        """``{"has_prev", "levels": [uint8 [h_l, w_l], ...], "keypoints": float64 [n, 2] (x, y),
        "lam": float64 [h, w]}`` of a stream: its previous pyramid, the keypoints it holds and the
        minimum-eigenvalue plane of the last frame it was given (synchronises)."""
        hp, nl, nk = C.c_int(0), C.c_int(0), C.c_int(0)
        lh, lw = (C.c_int * SOF_MAX_LEVELS)(), (C.c_int * SOF_MAX_LEVELS)()
        pyr = np.zeros(self.pyramid_bytes, np.uint8)
        kp = np.zeros((SOF_MAX_CORNERS, 2), np.float64)
        lam = np.zeros(self.max_h * self.max_w, np.float64)
        N.check(self._L.bx_sof_state_host(
            self._h, int(stream), C.byref(hp), C.byref(nl), lh, lw, pyr.ctypes.data, C.byref(nk),
            kp.ctypes.data, lam.ctypes.data), "bx_sof_state_host")
        out = {"has_prev": bool(hp.value), "levels": [], "keypoints": kp[: nk.value].copy(),
               "lam": None}
        off = 0
        for l in range(nl.value):
            out["levels"].append(pyr[off: off + lh[l] * lw[l]].reshape(lh[l], lw[l]).copy())
            off += lh[l] * lw[l]
        if out["levels"]:
            out["lam"] = lam[: lh[0] * lw[0]].reshape(lh[0], lw[0]).copy()
        return out

    def points(self, stream: int = 0):
        """The tracking record of a stream's last apply: ``{"prev", "next": float64 [n, 2],
        "tracked": bool [n], "iterations": int32 [n], "inlier": bool [n], "winner": int}``
        (synchronises)."""
        n, win = C.c_int(0), C.c_int(0)
        prev, nxt = np.zeros((SOF_MAX_CORNERS, 2)), np.zeros((SOF_MAX_CORNERS, 2))
        ok, inl = np.zeros(SOF_MAX_CORNERS, np.uint8), np.zeros(SOF_MAX_CORNERS, np.uint8)
        it = np.zeros(SOF_MAX_CORNERS, np.int32)
        N.check(self._L.bx_sof_points_host(
            self._h, int(stream), C.byref(n), prev.ctypes.data, nxt.ctypes.data, ok.ctypes.data,
            it.ctypes.data, inl.ctypes.data, C.byref(win)), "bx_sof_points_host")
        k = n.value
        return {"prev": prev[:k].copy(), "next": nxt[:k].copy(), "tracked": ok[:k].astype(bool),
                "iterations": it[:k].copy(), "inlier": inl[:k].astype(bool), "winner": win.value}


class _SofSettings:
    """The reference's feature and Lucas-Kanade parameters as attributes (``sof.py:44-58``)."""

    def _init_settings(self, scale):
        self.scale = scale
        self.grayscale = True
        self.max_corners = 1000
        self.quality_level = 0.01
        self.min_distance = 1
        self.block_size = 3
        self.win_size = 21
        self.max_level = 3
        self.criteria = (30, 0.01)  # LK: most iterations per level, the step that ends them
        self.ransac_threshold = 3.0  # consensus threshold in working pixels

    def _params(self) -> N.BxSofParams:
        """The C parameters; the refusals need no device."""
        if self.min_distance > 1:
            raise NotImplementedError("min_distance above 1 is not supported (the reference "
                                      "never uses it)")
        if self.block_size != 3:
            raise NotImplementedError("block_size other than 3 is not supported")
        win = int(self.win_size)
        if win % 2 == 0 or not 5 <= win <= 31:
            raise ValueError(f"win_size must be odd and within 5..31, got {self.win_size!r}")
        if not 1 <= int(self.max_corners) <= SOF_MAX_CORNERS:
            raise ValueError(f"max_corners must be within 1..{SOF_MAX_CORNERS}")
        if not 0 <= int(self.max_level) < SOF_MAX_LEVELS:
            raise ValueError(f"max_level must be within 0..{SOF_MAX_LEVELS - 1}")
        if not 0 < float(self.quality_level) <= 1:
            raise ValueError("quality_level must be within (0, 1]")
        max_iter, eps = self.criteria
        if int(max_iter) < 0 or not float(eps) >= 0 or not float(self.ransac_threshold) > 0:
            raise ValueError("criteria / ransac_threshold out of range")
        return N.BxSofParams(int(self.max_corners), win, int(self.max_level), int(max_iter),
                             float(self.quality_level), float(eps), float(self.ransac_threshold),
                             _scale_arg(self.scale))


class SofBatch(_SofSettings):
    """Sparse optical flow for ``n_streams`` cameras: one ``apply`` tracks every listed stream's
    keypoints from its previous frame into its new one and fits a similarity, all on the current
    stream.  With device inputs (frames a CUDA tensor, ``streams`` ``None`` or a CUDA tensor)
    nothing inside synchronises the host with the device.  A numpy ``frames`` array or a list of
    ``streams`` is copied to the device first, and that copy waits for the stream.

    ``max_h`` / ``max_w`` bound the working image (after the resize); left ``None`` they are taken
    from the first frames.  The parameters are ``SOF``'s attributes."""

    def __init__(self, n_streams: int, scale=0.15, max_h: int | None = None,
                 max_w: int | None = None):
        if n_streams < 1:
            raise ValueError("n_streams must be at least 1")
        self.n_streams = int(n_streams)
        self._init_settings(scale)
        self._cap = (max_h, max_w)
        self._handle = None
        self._all = None  # device arange(n_streams)
        self._eye = None  # device [n_streams, 6] identity warps

    def _ensure(self, H: int, W: int) -> _SofHandle:
        if self._handle is None:
            h, w = work_size(H, W, self.scale)
            self._handle = _SofHandle(self.n_streams, self._cap[0] or h, self._cap[1] or w)
        return self._handle

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None

    def reset(self, stream: int = -1):
        """Forget the previous frame of one stream (default: of all)."""
        if self._handle is not None:
            self._handle.reset(stream)

    def status(self) -> int:
        return 0 if self._handle is None else self._handle.status()

    def state(self, stream: int = 0):
        if self._handle is None:
            return {"has_prev": False, "levels": [], "keypoints": np.zeros((0, 2)), "lam": None}
        return self._handle.state(stream)

    def points(self, stream: int = 0):
        return self._handle.points(stream)

    def apply(self, frames, streams=None):
        """frames, streams: as ``EccBatch.apply`` (same checks; a CUDA ``streams`` tensor is not
        checked: an index out of range skips that frame and latches ``status()``).

        Returns CUDA tensors over all streams: warps float64 ``[n_streams, 6]`` (row-major 2x3,
        the engines' ``warps`` argument), code int32 (``SOF_OK`` / ``SOF_FIRST_FRAME`` /
        ``SOF_TOO_FEW`` / ``SOF_NO_MODEL`` / ``SOF_NO_KEYPOINTS``; ``SOF_NO_FRAME`` with the
        identity warp for a stream that was not listed), n_keypoints, n_tracked, n_inliers int32
        ``[n_streams]``."""
        import torch

        from .engine import _current_stream

        params = self._params()
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8:
                raise ValueError("frames must be uint8")
            n, H, W, ch = _frame_dims(frames.shape, self.grayscale)
            hd = self._ensure(H, W)
            frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        else:
            if frames.dtype != torch.uint8 or not frames.is_cuda:
                raise ValueError("frames must be a numpy array or a CUDA uint8 tensor")
            n, H, W, ch = _frame_dims(frames.shape, self.grayscale)
            hd = self._ensure(H, W)
            frames = frames.contiguous()
        S = self.n_streams
        if streams is None:
            if n > S:
                raise ValueError(f"capacity exceeded: {n} frames for {S} streams")
            if self._all is None:
                self._all = torch.arange(S, dtype=torch.int32, device="cuda")
            sd = self._all
        elif isinstance(streams, torch.Tensor) and streams.is_cuda:
            sd = streams.to(torch.int32).contiguous()
        else:
            sh = np.asarray(streams, np.int64).reshape(-1)
            if sh.size and (sh.min() < 0 or sh.max() >= S):
                raise ValueError("invalid argument: stream index out of range")
            if np.unique(sh).size != sh.size:
                raise ValueError("invalid argument: a stream is listed twice")
            sd = torch.from_numpy(sh.astype(np.int32)).cuda()
        if streams is not None and sd.numel() != n:
            raise ValueError(f"{n} frames but {sd.numel()} stream indices")
        if self._eye is None:  # device fills only: a tensor built from host values would copy
            self._eye = torch.zeros(S, 6, dtype=torch.float64, device="cuda")  # and synchronise
            self._eye[:, 0] = 1.0
            self._eye[:, 4] = 1.0
        warps = self._eye.clone()
        code = torch.full((S,), SOF_NO_FRAME, dtype=torch.int32, device="cuda")
        nkp = torch.zeros(S, dtype=torch.int32, device="cuda")
        ntrk = torch.zeros(S, dtype=torch.int32, device="cuda")
        ninl = torch.zeros(S, dtype=torch.int32, device="cuda")
        N.check(hd._L.bx_sof_apply(
            hd._h, n, H, W, ch, frames.data_ptr(), sd.data_ptr(), C.byref(params),
            warps.data_ptr(), code.data_ptr(), nkp.data_ptr(), ntrk.data_ptr(), ninl.data_ptr(),
            _current_stream()), "bx_sof_apply")
        self._keep = (frames, sd)  # alive until the next call: the launches are asynchronous
        return warps, code, nkp, ntrk, ninl


class SOF(_SofSettings):
    """The reference's ``SOF`` (``motion/cmc/sof.py``): ``apply(img, detections)`` returns the 2x3
    float32 warp from the previous frame to this one, the identity on the first frame and on any
    failure.  ``detections`` is ignored, as in the reference.  One camera; the device handle is
    built at the first frame from the image size.  The feature and Lucas-Kanade parameters are
    attributes with the reference's values (``max_corners``, ``quality_level``, ``min_distance``,
    ``block_size``, ``win_size``, ``max_level``, ``criteria``, ``ransac_threshold``).  ``last``
    holds the float64 warp, the code and the numbers of keypoints, tracked points and inliers of
    the last call."""

    def __init__(self, scale=0.15):
        self._init_settings(scale)
        self.last = None
        self._handle = None

    def reset(self):
        if self._handle is not None:
            self._handle.reset(0)

    def apply(self, img, detections=None):
        params = self._params()
        img = np.ascontiguousarray(img)
        if img.dtype != np.uint8:
            raise ValueError("img must be uint8")
        if img.ndim == 2:
            H, W, ch = img.shape[0], img.shape[1], 1
        else:
            _, H, W, ch = _frame_dims((1,) + img.shape, self.grayscale)
        if self._handle is None:
            h, w = work_size(H, W, self.scale)
            self._handle = _SofHandle(1, h, w)
        hd = self._handle
        streams = np.zeros(1, np.int32)
        warp = np.zeros((1, 6), np.float64)
        ints = np.zeros((4, 1), np.int32)
        from .engine import _current_stream

        N.check(hd._L.bx_sof_apply_host(
            hd._h, 1, H, W, ch, img.ctypes.data, streams.ctypes.data, C.byref(params),
            warp.ctypes.data, ints[0].ctypes.data, ints[1].ctypes.data, ints[2].ctypes.data,
            ints[3].ctypes.data, _current_stream()), "bx_sof_apply_host")
        self.last = {"warp": warp.reshape(2, 3).copy(), "code": int(ints[0, 0]),
                     "n_keypoints": int(ints[1, 0]), "n_tracked": int(ints[2, 0]),
                     "n_inliers": int(ints[3, 0])}
        return warp.reshape(2, 3).astype(np.float32)


# ------------------------------------------------------------------------------ chained SOF
_SOF_SETTINGS = ("max_corners", "quality_level", "min_distance", "block_size", "win_size",
                 "max_level", "criteria", "ransac_threshold")


class SofChain(_SofSettings):
    """Sparse optical flow over many consecutive frames of a camera per call
    (``bx_sof_apply_chain``): frame i of a call is tracked from frame i - 1 when
    both are of one stream, otherwise from its stream's stored state.  Warps, codes, the three
    counts and the streams' final state are bit for bit those of ``SofBatch.apply`` called one
    frame at a time.

    ``batch`` is the ``SofBatch`` whose handle the chain shares: ``chain.batch.apply`` is the
    plain apply on the same streams with the chain's settings, and the two may be mixed.  The
    parameters are ``SOF``'s attributes, read from the chain at every call (``scale`` is fixed at
    construction).  ``max_frames`` bounds a call's frames
    (``reserve`` grows it); the other arguments are ``SofBatch``'s."""

    def __init__(self, n_streams: int, max_frames: int = 64, scale=0.15,
                 max_h: int | None = None, max_w: int | None = None):
        if max_frames < 1:
            raise ValueError("max_frames must be at least 1")
        self._batch = SofBatch(n_streams, scale, max_h, max_w)
        self.n_streams = self._batch.n_streams
        self._init_settings(scale)
        self.max_frames = int(max_frames)
        self._reserved = 0
        self._keep = None

    @property
    def batch(self) -> SofBatch:
        for k in _SOF_SETTINGS:  # the chain's attributes are the settings of both
            setattr(self._batch, k, getattr(self, k))
        return self._batch

    def _ensure(self, H: int, W: int) -> _SofHandle:
        hd = self._batch._ensure(H, W)
        if self._reserved < self.max_frames:
            N.check(hd._L.bx_sof_chain_reserve(hd._h, self.max_frames), "bx_sof_chain_reserve")
            self._reserved = self.max_frames
        return hd

    def reserve(self, max_frames: int):
        """Room for ``max_frames`` frames per call (never shrinks)."""
        self.max_frames = max(self.max_frames, int(max_frames))
        if self._batch._handle is not None:
            self._ensure(0, 0)

    def close(self):
        self._batch.close()
        self._reserved = 0

    def reset(self, stream: int = -1):
        self._batch.reset(stream)

    def status(self) -> int:
        return self._batch.status()

    def state(self, stream: int = 0):
        return self._batch.state(stream)

    def points(self, stream: int = 0):
        return self._batch.points(stream)

    def _frames(self, frames):
        import torch

        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8:
                raise ValueError("frames must be uint8")
            dims = _frame_dims(frames.shape, self.grayscale)
            return torch.from_numpy(np.ascontiguousarray(frames)).cuda(), dims
        if frames.dtype != torch.uint8 or not frames.is_cuda:
            raise ValueError("frames must be a numpy array or a CUDA uint8 tensor")
        return frames.contiguous(), _frame_dims(frames.shape, self.grayscale)

    def apply(self, frames, streams, dst=None, out=None):
        """frames, streams, dst: as ``EccChain.apply`` (same checks).

        Frame i writes row ``dst[i]`` (default: row i) of ``out``, the tuple ``(warps [rows, 6]
        float64, code, n_keypoints, n_tracked, n_inliers [rows] int32)`` of CUDA tensors; other
        rows are untouched.  Without ``out`` fresh ``[n]``-row tensors are made (identity,
        ``SOF_NO_FRAME``, 0, 0, 0).  Returns ``out``.  With device inputs nothing inside
        synchronises the host with the device."""
        import torch

        from .engine import _current_stream

        params = self._params()
        frames, (n, H, W, ch) = self._frames(frames)
        hd = self._ensure(H, W)
        S = self.n_streams
        if isinstance(streams, torch.Tensor) and streams.is_cuda:
            sd = streams.to(torch.int32).contiguous()
        else:
            sh = np.asarray(streams, np.int64).reshape(-1)
            if sh.size and (sh.min() < 0 or sh.max() >= S):
                raise ValueError("invalid argument: stream index out of range")
            starts = sh[np.r_[True, sh[1:] != sh[:-1]]] if sh.size else sh
            if np.unique(starts).size != starts.size:
                raise ValueError("invalid argument: the frames of a stream are not adjacent")
            sd = torch.from_numpy(sh.astype(np.int32)).cuda()
        if sd.numel() != n:
            raise ValueError(f"{n} frames but {sd.numel()} stream indices")
        if out is None:
            if dst is not None:
                raise ValueError("dst needs the out tensors it points into")
            warps = torch.zeros(n, 6, dtype=torch.float64, device="cuda")
            warps[:, 0] = 1.0
            warps[:, 4] = 1.0
            out = (warps, torch.full((n,), SOF_NO_FRAME, dtype=torch.int32, device="cuda"),
                   torch.zeros(n, dtype=torch.int32, device="cuda"),
                   torch.zeros(n, dtype=torch.int32, device="cuda"),
                   torch.zeros(n, dtype=torch.int32, device="cuda"))
        warps, code, nkp, ntrk, ninl = out
        rows = int(code.numel())
        want = ((warps, torch.float64, rows * 6), (code, torch.int32, rows),
                (nkp, torch.int32, rows), (ntrk, torch.int32, rows), (ninl, torch.int32, rows))
        for t, dt, ne in want:
            if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == ne):
                raise ValueError("out must be contiguous CUDA tensors: warps [rows, 6] float64, "
                                 "code, n_keypoints, n_tracked, n_inliers int32 [rows]")
        dd = None
        if dst is None:
            if n > rows:
                raise ValueError(f"{n} frames but {rows} result rows")
        elif isinstance(dst, torch.Tensor) and dst.is_cuda:
            dd = dst.to(torch.int64).contiguous()
        else:
            dh = np.asarray(dst, np.int64).reshape(-1)
            if dh.size and (dh.min() < 0 or dh.max() >= rows):
                raise ValueError("invalid argument: dst row out of range")
            dd = torch.from_numpy(dh).cuda()
        if dd is not None and dd.numel() != n:
            raise ValueError(f"{n} frames but {dd.numel()} dst rows")
        N.check(hd._L.bx_sof_apply_chain(
            hd._h, n, H, W, ch, frames.data_ptr(), sd.data_ptr(),
            None if dd is None else dd.data_ptr(), C.byref(params), warps.data_ptr(),
            code.data_ptr(), nkp.data_ptr(), ntrk.data_ptr(), ninl.data_ptr(),
            _current_stream()), "bx_sof_apply_chain")
        self._keep = (frames, sd, dd)  # alive until the next call: the launches are asynchronous
        return out

    def apply_host(self, frames, streams):
        """The host entry (``bx_sof_apply_chain_host``): numpy ``frames`` and ``streams`` in,
        numpy ``(warps [n, 6], code, n_keypoints, n_tracked, n_inliers)`` out, one
        synchronisation.  The library itself refuses a stream index out of range or a stream whose
        frames are not adjacent (``ValueError``, nothing launched)."""
        from .engine import _current_stream

        params = self._params()
        frames = np.ascontiguousarray(frames)
        if frames.dtype != np.uint8:
            raise ValueError("frames must be uint8")
        n, H, W, ch = _frame_dims(frames.shape, self.grayscale)
        sh = np.ascontiguousarray(np.asarray(streams).reshape(-1), np.int32)
        if sh.size != n:
            raise ValueError(f"{n} frames but {sh.size} stream indices")
        hd = self._ensure(H, W)
        warps = np.zeros((n, 6), np.float64)
        ints = np.zeros((4, n), np.int32)
        N.check(hd._L.bx_sof_apply_chain_host(
            hd._h, n, H, W, ch, frames.ctypes.data, sh.ctypes.data, C.byref(params),
            warps.ctypes.data, ints[0].ctypes.data, ints[1].ctypes.data, ints[2].ctypes.data,
            ints[3].ctypes.data, _current_stream()), "bx_sof_apply_chain_host")
        return warps, ints[0], ints[1], ints[2], ints[3]


class SofWarpTable(WarpTable):
    """A ``WarpTable`` of sparse-optical-flow warps: ``code`` holds ``SOF_*`` values
    (``NOT_STEPPED`` for a frame its sequence is not stepped at), and ``n_keypoints``,
    ``n_tracked``, ``n_inliers`` ``[T, S]`` int32 are the counts of every stepped frame.  ``rho``
    and ``iterations`` are the zeros of an empty table: sparse optical flow has neither."""

    def __init__(self, warps, rho, iterations, code, n_keypoints, n_tracked, n_inliers):
        super().__init__(warps, rho, iterations, code)
        self.n_keypoints, self.n_tracked, self.n_inliers = n_keypoints, n_tracked, n_inliers

    def host(self) -> dict:
        out = super().host()
        for k in ("n_keypoints", "n_tracked", "n_inliers"):
            out[k] = getattr(self, k).cpu().numpy()
        return out

    def close(self):
        super().close()
        self.n_keypoints = self.n_tracked = self.n_inliers = None


def _table_frames(images, stepped):
    """warp_table's frame fetching: the masks as bool arrays, ``fetch(k, t)`` and every
    sequence's frame size (``None`` for one that is never stepped)."""
    S = len(images)
    if len(stepped) != S:
        raise ValueError(f"{S} image sources but {len(stepped)} stepped masks")
    stepped = [np.asarray(m, bool).reshape(-1) for m in stepped]
    first = {}  # a callable's first stepped frame, read for its size and used once

    def fetch(k: int, t: int) -> np.ndarray:
        if k in first and first[k][0] == t:
            return first.pop(k)[1]
        src = images[k]
        f = np.asarray(src(int(t)) if callable(src) else src[int(t)])
        if f.dtype != np.uint8 or f.ndim not in (2, 3) or (f.ndim == 3 and f.shape[2] != 3):
            raise ValueError(f"sequence {k}: frames must be uint8 [H, W] or [H, W, 3]")
        return f

    sizes = []
    for k, m in enumerate(stepped):
        if not callable(images[k]) and len(images[k]) < m.size:
            raise ValueError(f"sequence {k}: {len(images[k])} frames for a mask of {m.size}")
        if not m.any():
            sizes.append(None)
            continue
        t0 = int(np.flatnonzero(m)[0])
        first[k] = (t0, fetch(k, t0))
        sizes.append(first[k][1].shape)
    return stepped, fetch, sizes


def sof_warp_table(images, stepped, *, sof=None, chunk: int = 64) -> SofWarpTable:
    """The sparse-optical-flow warp of every stepped frame of S sequences, computed by chained
    calls of at most ``chunk`` frames (``chain_plan``) and left in device memory.

    images, stepped: as ``warp_table``.  sof: an object that carries ``SOF``'s settings as
    attributes (a ``SOF``, ``SofBatch`` or ``SofChain``; only ``scale`` and the settings are read,
    the object is neither run nor changed); ``None`` means ``SOF()``'s defaults.  The template of a
    stepped frame is the previous stepped frame of its sequence; a sequence's first stepped frame
    has code ``SOF_FIRST_FRAME`` (``SOF_NO_KEYPOINTS`` without a corner).  ``rho`` and
    ``iterations`` of the table are unused (zeros)."""
    import torch

    src = SOF() if sof is None else sof
    carrier = SOF(scale=src.scale)
    for k in _SOF_SETTINGS:
        setattr(carrier, k, getattr(src, k))
    carrier._params()  # the refusals, before anything is built
    stepped, fetch, sizes = _table_frames(images, stepped)
    S = len(images)
    calls = chain_plan(stepped, sizes, chunk)
    T = max([m.size for m in stepped] + [0])
    base = _empty_table(T, S)
    tab = SofWarpTable(base.warps, base.rho, base.iterations, base.code,
                       *(torch.zeros(T, S, dtype=torch.int32, device="cuda") for _ in range(3)))
    if not calls:
        return tab
    work = [work_size(sz[0], sz[1], carrier.scale) for sz in sizes if sz is not None]
    ch = SofChain(S, max_frames=max(c[1].size for c in calls), scale=carrier.scale,
                  max_h=max(h for h, _ in work), max_w=max(w for _, w in work))
    for k in _SOF_SETTINGS:
        setattr(ch, k, getattr(carrier, k))
    try:
        out = (tab.warps.view(-1, 6), tab.code.view(-1), tab.n_keypoints.view(-1),
               tab.n_tracked.view(-1), tab.n_inliers.view(-1))
        for size, seq, t in calls:
            frames = np.stack([fetch(int(k), int(x)) for k, x in zip(seq, t)])
            if frames.shape[1:] != tuple(size):
                raise ValueError(f"sequence {int(seq[0])}: frames of more than one size")
            ch.apply(frames, seq, dst=t * S + seq, out=out)
        st = ch.status()  # (synchronises: the staged frames may go)
        if st != 0:
            raise RuntimeError(f"sof status {st}")
    finally:
        ch.close()
    return tab


def get_cmc_method(cmc_method):
    """``motion/cmc/__init__.py``'s lookup: the class of a method name, ``None`` for an unknown
    one.  ECC is returned as the reference does; "sof" keeps its refusal (the lookup's behaviour
    is pinned) and points to the class that runs it; ORB and SIFT are OpenCV's."""
    if cmc_method == "ecc":
        return ECC
    if cmc_method == "sof":
        raise NotImplementedError("cmc method 'sof' is not returned by this lookup: assign "
                                  "boxmot_amd.SOF() to tracker.cmc")
    if cmc_method in ("orb", "sift"):
        raise NotImplementedError(f"cmc method '{cmc_method}' is not supported: it is feature-based "
                                  "and defined by OpenCV; assign your own object to tracker.cmc")
    return None

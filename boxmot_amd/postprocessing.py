"""GSI post-processing on the GPU: Gaussian-smoothed interpolation of MOT result files.

Reference path replaced (``boxmot/postprocessing/gsi.py``, from StrongSORT++): per file, one CPU
process runs ``linear_interpolation`` (a Python loop over the rows) and ``gaussian_smooth`` (one
scikit-learn ``GaussianProcessRegressor`` fit and predict, i.e. one dense Cholesky, per
tracklet).  Here the rows of all files go through one interpolation (sort, count + prefix, fill)
and one smoothing launch (one workgroup per tracklet) of libbxassoc.so (``include/bxgsi.h``).
Names, signatures and the file contract follow the reference; the process pool and the progress
bar are not reproduced.  There is no CPU fallback: without the library or a HIP device the calls
raise ``NativeUnavailable``.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _native as N

MOT_FMT = "%d %d %d %d %d %d %d %d %d"  # the reference's np.savetxt format (space-separated)


def _rows(data) -> np.ndarray:
    a = np.asarray(data, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"tracking results must be a 2-D array, got {a.ndim}-D")
    if a.shape[1] < 8:
        raise ValueError(f"tracking results need at least 8 columns, got {a.shape[1]}")
    return np.ascontiguousarray(a)


def _device():
    import torch

    L = N.load()
    if N.device_count() == 0 or not torch.cuda.is_available():
        raise N.NativeUnavailable("GSI post-processing needs a HIP device")
    return L, torch, torch.cuda.current_stream().cuda_stream


def _interpolate_device(rows: np.ndarray, seq: np.ndarray | None, interval: int):
    """rows [R][C] (host) -> (interpolated rows on the device [n][C], their sequence [n] or None,
    tracklet offsets [T+1] on the host)."""
    L, torch, st = _device()
    R, ncol = rows.shape
    dev = torch.device("cuda")
    d_rows = torch.from_numpy(rows).to(dev)
    d_seq = torch.from_numpy(np.ascontiguousarray(seq, np.int32)).to(dev) if seq is not None \
        else None
    nbytes = C.c_size_t()
    N.check(L.bx_gsi_plan_workspace_bytes(R, C.byref(nbytes)), "bx_gsi_plan_workspace_bytes")
    plan = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    N.check(L.bx_gsi_interpolate_plan(d_rows.data_ptr(), d_seq.data_ptr() if d_seq is not None
                                      else None, R, ncol, int(interval), plan.data_ptr(),
                                      nbytes.value, counts.data_ptr(), st),
            "bx_gsi_interpolate_plan")
    n_out, n_tracks = (int(v) for v in counts.cpu())
    out = torch.empty((n_out, ncol), dtype=torch.float64, device=dev)
    out_seq = torch.empty(n_out, dtype=torch.int32, device=dev) if seq is not None else None
    off = torch.zeros(n_tracks + 1, dtype=torch.int32, device=dev)
    N.check(L.bx_gsi_interpolate(d_rows.data_ptr(), R, ncol, plan.data_ptr(), out.data_ptr(),
                                 out_seq.data_ptr() if out_seq is not None else None, n_out,
                                 off.data_ptr(), st), "bx_gsi_interpolate")
    return out, out_seq, off.cpu().numpy()


def _smooth_device(d_rows, off: np.ndarray, tau: float, force_blocked: bool = False):
    """Device rows [n][C] grouped by tracklet (prefix offsets `off`, host) -> smoothed [n][9]."""
    L, torch, st = _device()
    dev = torch.device("cuda")
    off = np.ascontiguousarray(off, np.int32)
    n_tracks = off.shape[0] - 1
    n = d_rows.shape[0]
    nbytes = C.c_size_t()
    N.check(L.bx_gsi_workspace_bytes(off.ctypes.data, n_tracks, int(force_blocked),
                                     C.byref(nbytes)), "bx_gsi_workspace_bytes")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 9), dtype=torch.float64, device=dev)
    status = torch.zeros(max(n_tracks, 1), dtype=torch.int32, device=dev)
    N.check(L.bx_gsi_smooth(d_rows.data_ptr(), d_rows.shape[1], off.ctypes.data, n_tracks,
                            float(tau), int(force_blocked), ws.data_ptr(), nbytes.value,
                            out.data_ptr(), status.data_ptr(), st), "bx_gsi_smooth")
    bad = np.flatnonzero(status.cpu().numpy()[:n_tracks])  # (synchronises: `off` was read by now)
    if bad.size:
        k = int(bad[0])
        ident = d_rows[int(off[k]), 1].item()
        raise np.linalg.LinAlgError(
            f"the kernel matrix of id {ident:g} ({int(off[k + 1] - off[k])} rows) is not positive "
            "definite: duplicate or non-finite frames?")
    return out


def linear_interpolation(data: np.ndarray, interval: int) -> np.ndarray:
    """gsi.py:13-54: rows sorted by (id, frame), every gap ``prev+1 < cur < prev+interval`` of one
    id filled with linearly interpolated rows (bitwise the reference's float64 values)."""
    rows = _rows(data)
    if rows.shape[0] == 0:
        return rows.copy()
    out, _, _ = _interpolate_device(rows, None, interval)
    return out.cpu().numpy()


def gaussian_smooth(data: np.ndarray, tau: float) -> np.ndarray:
    """gsi.py:57-93: per id (ascending; rows keep their order within an id) columns 2..5 replaced
    by the mean of a Gaussian process with the reference's fixed RBF kernel; rows are ``[frame,
    id, 4 smoothed, col 6, col 7, -1]``."""
    return _gaussian_smooth(data, tau)


def _gaussian_smooth(data, tau, force_blocked: bool = False) -> np.ndarray:
    """gaussian_smooth; ``force_blocked`` sends every tracklet through the blocked factorisation
    (a test hook: the two paths agree within the solver tolerance)."""
    import torch

    rows = _rows(data)
    if rows.shape[0] == 0:
        return np.empty((0, 9))
    order = np.argsort(rows[:, 1], kind="stable")
    rows = rows[order]
    starts = np.flatnonzero(np.r_[True, rows[1:, 1] != rows[:-1, 1]])
    off = np.r_[starts, rows.shape[0]].astype(np.int32)
    _device()
    return _smooth_device(torch.from_numpy(rows).to("cuda"), off, tau, force_blocked).cpu().numpy()


def gsi_batch(arrays, interval: int = 20, tau: float = 10) -> list:
    """``gaussian_smooth(linear_interpolation(a, interval), tau)`` for every array of the list,
    with all their tracklets in one interpolation and one smoothing launch.  An array without
    rows yields an empty ``[0, 9]`` result."""
    arrs = [_rows(a) for a in arrays]
    live = [k for k, a in enumerate(arrs) if a.shape[0]]
    res = [np.empty((0, 9)) for _ in arrs]
    if not live:
        return res
    ncol = min(arrs[k].shape[1] for k in live)  # (files of one run share their width)
    rows = np.concatenate([arrs[k][:, :ncol] for k in live])
    seq = np.concatenate([np.full(arrs[k].shape[0], q, np.int32) for q, k in enumerate(live)])
    d_interp, d_seq, off = _interpolate_device(np.ascontiguousarray(rows), seq, interval)
    out = _smooth_device(d_interp, off, tau).cpu().numpy()
    bounds = np.searchsorted(d_seq.cpu().numpy(), np.arange(len(live) + 1))
    for q, k in enumerate(live):
        res[k] = out[bounds[q]: bounds[q + 1]]
    return res


def gsi_device(rows, base, n, n_seq: int | None = None, interval: int = 20, tau: float = 10,
               row_stride: int = 9, truncate: bool = True):
    """GSI of result slots in device memory (``SequenceFeeder.results_device``) into rows in
    device memory that ``MotEvaluator.run_device`` takes as they are: sequence ``q`` owns rows
    ``[base[q], base[q] + n[q])`` of ``rows`` (``[., row_stride]`` float64, ``row_stride >= 8``),
    and rows outside the slots are never read.  ``rows`` / ``base`` / ``n`` are contiguous CUDA
    tensors (float64, int64, int64) or raw integer device pointers; ``n_seq`` is needed with raw
    pointers only (a pointer carries no length) and defaults to ``n.numel()``.

    Returns CUDA tensors ``(out_rows [n_out, 9] float64, out_base [n_seq] int64, out_n [n_seq]
    int64)``: the sequences consecutively in input order, each holding the bits
    ``gsi_batch([its rows], interval, tau)[0]`` holds, and with ``truncate`` every value truncated
    toward zero (a zero is ``+0.0``), which is what ``np.loadtxt`` reads from the file ``gsi``
    leaves.  Equal ids in different sequences are different tracklets.  No row crosses to the
    host; the counts, the tracklet offsets and ``base`` / ``n`` do (include/bxgsi.h).
    ``LinAlgError`` / ``ValueError`` as in the host path."""
    L, torch, st = _device()
    dev = torch.device("cuda")
    S = None if n_seq is None else int(n_seq)
    ptr = []
    for name, x, dt in (("rows", rows, torch.float64), ("base", base, torch.int64),
                        ("n", n, torch.int64)):
        if isinstance(x, torch.Tensor):
            if not x.is_cuda or x.dtype != dt or not x.is_contiguous():
                raise ValueError(f"gsi_device: {name} must be a contiguous CUDA {dt} tensor")
            if name == "n" and S is None:
                S = x.numel()
            if name != "rows" and S is not None and x.numel() < S:
                raise ValueError(f"gsi_device: {name} needs n_seq = {S} entries")
            ptr.append(x.data_ptr() if x.numel() else None)
        else:
            ptr.append(int(x) or None)
    if S is None:
        raise ValueError("gsi_device: raw pointers carry no length: give n_seq")
    if S < 0 or int(row_stride) < 8:
        raise ValueError("gsi_device: n_seq must not be negative and row_stride at least 8")
    if isinstance(rows, torch.Tensor):
        if rows.numel() % int(row_stride):
            raise ValueError("gsi_device: rows is not a whole number of row_stride columns")
        if S and isinstance(base, torch.Tensor) and isinstance(n, torch.Tensor):
            have = rows.numel() // int(row_stride)
            b, c = base[:S], n[:S]
            if bool(((b < 0) | (c < 0) | (b + c > have)).any()):
                raise ValueError("gsi_device: base / n reach outside the rows tensor")
    counts = (C.c_int64 * 2)()
    plan = C.c_void_p()
    N.check(L.bx_gsi_device_plan(ptr[0], int(row_stride), ptr[1], ptr[2], S, int(interval),
                                 counts, C.byref(plan), st), "bx_gsi_device_plan")
    try:
        out = torch.empty((counts[0], 9), dtype=torch.float64, device=dev)
        out_base = torch.zeros(S, dtype=torch.int64, device=dev)
        out_n = torch.zeros(S, dtype=torch.int64, device=dev)
        rc = L.bx_gsi_device_run(plan, float(tau), int(bool(truncate)),
                                 out.data_ptr() if counts[0] else None, counts[0],
                                 out_base.data_ptr() if S else None,
                                 out_n.data_ptr() if S else None, st)
        if rc == 1 and b"not positive definite" in L.bx_last_error():
            raise np.linalg.LinAlgError(L.bx_last_error().decode(errors="replace"))
        N.check(rc, "bx_gsi_device_run")
    finally:
        L.bx_gsi_device_free(plan)
    return out, out_base, out_n


def gsi(mot_results_folder: Path, interval: int = 20, tau: float = 10):
    """gsi.py:115-142: apply GSI in place to every ``MOT*.txt`` of the folder (comma-separated in,
    the reference's space-separated ``%d`` rows out; a file without rows is left untouched)."""
    files = sorted(Path(mot_results_folder).glob("MOT*.txt"))
    loaded = []
    for f in files:
        a = np.loadtxt(f, delimiter=",", ndmin=2) if f.stat().st_size else np.empty((0, 0))
        if a.size:
            loaded.append((f, a))
    if not loaded:
        return
    for (f, _), smoothed in zip(loaded, gsi_batch([a for _, a in loaded], interval, tau)):
        np.savetxt(f, smoothed, fmt=MOT_FMT)

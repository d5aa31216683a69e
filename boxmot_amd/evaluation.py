"""MOT evaluation on the GPU: HOTA, CLEAR and Identity metrics of MOT result files.

Reference stage replaced (``boxmot/engine/val.py:224-267``): a TrackEval subprocess per run, whose
printed COMBINED row ``parse_mot_results`` (``val.py:190-219``) reads back.  Here the gt and result
rows of all sequences go through one handle of libbxassoc.so (``include/bxeval.h``): similarity,
the MOT16/17/20 distractor preprocessing, the per-frame assignments of HOTA and CLEAR and the
per-sequence assignment of Identity all run on the device (DESIGN.md 2.13 is the contract).  Text
parsing is host code.  There is no CPU fallback: without the library or a HIP device the calls
raise ``NativeUnavailable``.
"""
from __future__ import annotations

import ctypes as C
import io
import os
from pathlib import Path

import numpy as np

from . import _native as N

BENCHMARKS = {"MOT16": 16, "MOT17": 17, "MOT20": 20}
METRICS = ("HOTA", "CLEAR", "Identity")
N_ALPHA = 19
ALPHAS = np.arange(0.05, 0.99, 0.05)

# the record layout of include/bxeval.h (BX_EVAL_*)
HOTA_FIELDS = ("HOTA_TP", "HOTA_FN", "HOTA_FP", "AssA", "AssRe", "AssPr", "LocA", "DetA", "DetRe",
               "DetPr", "HOTA")
HOTA_INT = ("HOTA_TP", "HOTA_FN", "HOTA_FP")
CLEAR_FIELDS = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag", "MOTP_sum",
                "CLR_Frames", "MOTA", "MOTP", "MODA", "sMOTA", "CLR_Re", "CLR_Pr", "MTR", "PTR",
                "MLR")
CLEAR_INT = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag", "CLR_Frames")
IDENTITY_FIELDS = ("IDTP", "IDFN", "IDFP", "IDF1", "IDR", "IDP")
IDENTITY_INT = ("IDTP", "IDFN", "IDFP")
COUNT_FIELDS = ("Dets", "GT_Dets", "IDs", "GT_IDs")
CLEAR_AT, IDENTITY_AT, COUNT_AT, RECORD = 209, 228, 234, 238


def load_mot_rows(src, min_cols: int) -> np.ndarray:
    """Rows of a MOT text file (comma- or whitespace-separated), or of an array, as float64
    ``[n, >= min_cols]``.  A missing or empty file has no rows."""
    if isinstance(src, (str, os.PathLike)):
        p = Path(src)
        text = p.read_text() if p.exists() else ""
        if not text.strip():
            return np.empty((0, min_cols))
        a = np.loadtxt(io.StringIO(text.replace(",", " ")), dtype=np.float64, ndmin=2)
    else:
        a = np.asarray(src, dtype=np.float64)
        if a.size == 0:
            return np.empty((0, min_cols))
    if a.ndim != 2 or a.shape[1] < min_cols:
        raise ValueError(f"MOT rows need at least {min_cols} columns, got shape {a.shape}")
    return a


def _check_rows(name: str, what: str, rows: np.ndarray, frames: int) -> None:
    """The host layer's own input checks (the native entry repeats them)."""
    if rows.shape[0] == 0:
        return
    fr, ids = rows[:, 0], rows[:, 1]
    if np.any(fr != np.floor(fr)) or np.any(ids != np.floor(ids)):
        raise ValueError(f"{name}: {what} frames and ids must be integers")
    if fr.min() < 1 or fr.max() > frames:
        bad = fr[(fr < 1) | (fr > frames)][0]
        raise ValueError(f"{name}: {what} frame {bad:g} is outside 1..{frames}")
    lo = ids.min()
    key = fr.astype(np.int64) * np.int64(ids.max() - lo + 1) + (ids - lo).astype(np.int64)
    if np.unique(key).shape[0] != key.shape[0]:
        raise ValueError(f"{name}: {what} has an id twice in one frame")


def prepare_inputs(gt: dict, results, seq_lengths: dict | None = None):
    """(names, frames [S], gt rows per sequence [n, 9], result rows per sequence [n, 6]) of an
    ``evaluate_mot`` call, parsed and checked."""
    names = list(gt)
    if not names:
        raise ValueError("evaluate_mot needs at least one sequence")
    if isinstance(results, (str, os.PathLike)):
        root = Path(results)
        results = {n: root / f"{n}.txt" for n in names}
    gts, trs, frames = [], [], []
    for n in names:
        g = load_mot_rows(gt[n], 9)[:, :9]
        t = load_mot_rows(results[n], 7)[:, :6] if n in results else np.empty((0, 6))
        if seq_lengths is not None and n in seq_lengths:
            T = int(seq_lengths[n])
        elif g.shape[0]:
            T = int(g[:, 0].max())
        else:
            raise ValueError(f"{n}: no gt rows and no seq_lengths entry to take the length from")
        if T < 1:
            raise ValueError(f"{n}: sequence length {T}")
        _check_rows(n, "gt", g, T)
        _check_rows(n, "results", t, T)
        gts.append(np.ascontiguousarray(g))
        trs.append(np.ascontiguousarray(t))
        frames.append(T)
    return names, np.asarray(frames, np.int32), gts, trs


class MotEvaluator:
    """One ``bx_eval`` handle: capacities (``None`` = the header's defaults) and a device arena
    that is reused from run to run."""

    def __init__(self, max_boxes: int | None = None, max_ids: int | None = None,
                 max_frames: int | None = None):
        import torch  # (first, as everywhere in the package: one HIP runtime per process)

        self._h = C.c_void_p()
        self._L = N.load()
        if N.device_count() == 0 or not torch.cuda.is_available():
            raise N.NativeUnavailable("MOT evaluation needs a HIP device")
        N.check(self._L.bx_eval_create(int(max_boxes or 0), int(max_ids or 0),
                                       int(max_frames or 0), C.byref(self._h)), "bx_eval_create")

    def close(self):
        if self._h:
            self._L.bx_eval_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def capacity(self) -> dict:
        v = [C.c_int() for _ in range(4)]
        N.check(self._L.bx_eval_capacity(self._h, *[C.byref(x) for x in v]), "bx_eval_capacity")
        return dict(zip(("max_boxes", "max_ids", "max_frames", "lds_n"), (x.value for x in v)))

    def run(self, frames: np.ndarray, gts: list, trs: list, benchmark: int) -> np.ndarray:
        """Records ``[S + 1, RECORD]`` (the last one COMBINED) of S sequences."""
        S = len(gts)
        frames = np.ascontiguousarray(frames, np.int32)
        goff = np.zeros(S + 1, np.int64)
        toff = np.zeros(S + 1, np.int64)
        goff[1:] = np.cumsum([g.shape[0] for g in gts])
        toff[1:] = np.cumsum([t.shape[0] for t in trs])
        grow = np.ascontiguousarray(np.concatenate(gts), np.float64) if goff[-1] else \
            np.zeros((1, 9))
        trow = np.ascontiguousarray(np.concatenate(trs), np.float64) if toff[-1] else \
            np.zeros((1, 6))
        out = np.zeros((S + 1, RECORD))
        N.check(self._L.bx_eval_run_host(self._h, S, int(benchmark), frames.ctypes.data,
                                         goff.ctypes.data, grow.ctypes.data, toff.ctypes.data,
                                         trow.ctypes.data, out.ctypes.data, None),
                "bx_eval_run_host")
        return out

    def set_gt(self, frames: np.ndarray, gts: list) -> None:
        """Bucket and upload the gt of S sequences once; ``run_device`` scores against it until
        the next call replaces it.  ``run`` ignores it."""
        S = len(gts)
        frames = np.ascontiguousarray(frames, np.int32)
        goff = np.zeros(S + 1, np.int64)
        goff[1:] = np.cumsum([g.shape[0] for g in gts])
        grow = np.ascontiguousarray(np.concatenate(gts), np.float64) if S and goff[-1] else \
            np.zeros((1, 9))
        N.check(self._L.bx_eval_set_gt_host(self._h, S, frames.ctypes.data, goff.ctypes.data,
                                            grow.ctypes.data), "bx_eval_set_gt_host")
        self._gt_seqs = S

    def run_device(self, rows, base, n, n_groups: int, benchmark: int,
                   row_stride: int = 9) -> np.ndarray:
        """Records ``[n_groups, S + 1, RECORD]`` of tracker rows in device memory against the gt
        of ``set_gt``: evaluator sequence ``k * S + s`` is rows ``[base[q], base[q] + n[q])`` of
        ``rows`` (``[., row_stride]`` float64: frame, id, x, y, w, h, ...), scored against gt
        sequence ``s``; each group's last record is its COMBINED.  ``rows`` / ``base`` / ``n``
        are contiguous CUDA tensors (float64, int64, int64) or raw integer device pointers; the
        rows stay on the device.  Bit-identical to ``run`` on the same rows in the same order."""
        import torch

        S = getattr(self, "_gt_seqs", 0)
        K = int(n_groups)
        ptr = []
        for name, x, dt in (("rows", rows, torch.float64), ("base", base, torch.int64),
                            ("n", n, torch.int64)):
            if isinstance(x, torch.Tensor):
                if not x.is_cuda or x.dtype != dt or not x.is_contiguous():
                    raise ValueError(f"run_device: {name} must be a contiguous CUDA {dt} tensor")
                if name != "rows" and S and x.numel() < K * S:
                    raise ValueError(f"run_device: {name} needs n_groups * S = {K * S} entries")
                if name == "rows" and x.numel() == 0:
                    # (an empty tensor has no storage to point at; no row of it is ever read)
                    x = pad = torch.zeros(int(row_stride), dtype=dt, device=x.device)
                ptr.append(x.data_ptr())
            else:
                ptr.append(int(x))
        if isinstance(rows, torch.Tensor):
            if rows.numel() % int(row_stride):
                raise ValueError("run_device: rows is not a whole number of row_stride columns")
            if S and K >= 1 and isinstance(base, torch.Tensor) and isinstance(n, torch.Tensor):
                have = rows.numel() // int(row_stride)
                b, c = base[:K * S], n[:K * S]
                if bool(((b < 0) | (c < 0) | (b + c > have)).any()):
                    raise ValueError("run_device: base / n reach outside the rows tensor")
            torch.cuda.current_stream().synchronize()  # (the rows' producer, before our stream)
        out = np.zeros((max(K, 1), S + 1, RECORD))
        N.check(self._L.bx_eval_run_device(self._h, K, int(benchmark), ptr[0], int(row_stride),
                                           ptr[1], ptr[2], out.ctypes.data, None),
                "bx_eval_run_device")
        return out


def _unpack(rec: np.ndarray, metrics) -> dict:
    res = {}
    if "HOTA" in metrics:
        h = {}
        for k, f in enumerate(HOTA_FIELDS):
            v = rec[k * N_ALPHA: (k + 1) * N_ALPHA]
            h[f + "_alpha"] = v.astype(np.int64) if f in HOTA_INT else v.copy()
            h[f] = float(np.mean(v))
        res["HOTA"] = h
    if "CLEAR" in metrics:
        res["CLEAR"] = {f: int(rec[CLEAR_AT + k]) if f in CLEAR_INT else float(rec[CLEAR_AT + k])
                        for k, f in enumerate(CLEAR_FIELDS)}
    if "Identity" in metrics:
        res["Identity"] = {f: int(rec[IDENTITY_AT + k]) if f in IDENTITY_INT
                           else float(rec[IDENTITY_AT + k])
                           for k, f in enumerate(IDENTITY_FIELDS)}
    res["Count"] = {f: int(rec[COUNT_AT + k]) for k, f in enumerate(COUNT_FIELDS)}
    return res


def evaluate_mot(gt: dict, results, benchmark: str = "MOT17", seq_lengths: dict | None = None,
                 metrics=METRICS, max_boxes: int | None = None, max_ids: int | None = None,
                 max_frames: int | None = None) -> dict:
    """TrackEval's HOTA / CLEAR / Identity of MOT16/17/20 pedestrian results, on the GPU.

    ``gt``: name -> ``gt.txt``-style file or ``[n, 9]`` array (frame, id, x, y, w, h, zero_marked,
    class, visibility).  ``results``: a folder holding ``<name>.txt``, or name -> file or
    ``[n, >= 7]`` array (frame, id, x, y, w, h, conf, ...); a missing or empty file is a sequence
    without tracker detections.  ``seq_lengths``: name -> frames (``seqinfo.ini``), default the
    largest gt frame.  Returns name -> {"HOTA", "CLEAR", "Identity", "Count"} and "COMBINED";
    every HOTA field is the mean over the 19 alphas, with the per-alpha vector under
    ``<field>_alpha``.  ``max_boxes`` / ``max_ids`` / ``max_frames`` are the handle's capacities
    (boxes of one side per frame, ids of one side per sequence, frames per sequence); exceeding
    one is a ``ValueError``.
    """
    if benchmark not in BENCHMARKS:
        raise ValueError(f"benchmark must be one of {sorted(BENCHMARKS)}, got {benchmark!r}")
    metrics = tuple(metrics)
    for m in metrics:
        if m not in METRICS:
            raise ValueError(f"unknown metric family {m!r} (known: {METRICS})")
    names, frames, gts, trs = prepare_inputs(gt, results, seq_lengths)
    if "COMBINED" in names:
        raise ValueError("a sequence cannot be called COMBINED")
    ev = MotEvaluator(max_boxes, max_ids, max_frames)
    try:
        out = ev.run(frames, gts, trs, BENCHMARKS[benchmark])
    finally:
        ev.close()
    res = {n: _unpack(out[k], metrics) for k, n in enumerate(names)}
    res["COMBINED"] = _unpack(out[len(names)], metrics)
    return res


def evaluate_mot_device(gt: dict, rows, base, n, n_groups: int = 1, benchmark: str = "MOT17",
                        seq_lengths: dict | None = None, metrics=METRICS,
                        max_boxes: int | None = None, max_ids: int | None = None,
                        max_frames: int | None = None, row_stride: int = 9) -> list:
    """``evaluate_mot`` for tracker rows that already lie in device memory, ``n_groups`` result
    sets at once (the configurations of a sweep): ``rows`` / ``base`` / ``n`` as
    ``MotEvaluator.run_device`` takes them, sequence ``k * S + s`` being gt sequence ``s`` (in
    ``gt``'s order) of group ``k``.  Returns one dict per group, shaped like ``evaluate_mot``'s.
    The rows never leave the device."""
    if benchmark not in BENCHMARKS:
        raise ValueError(f"benchmark must be one of {sorted(BENCHMARKS)}, got {benchmark!r}")
    metrics = tuple(metrics)
    for m in metrics:
        if m not in METRICS:
            raise ValueError(f"unknown metric family {m!r} (known: {METRICS})")
    if int(n_groups) < 1:
        raise ValueError("n_groups must be at least 1")
    names, frames, gts, _ = prepare_inputs(gt, {}, seq_lengths)
    if "COMBINED" in names:
        raise ValueError("a sequence cannot be called COMBINED")
    ev = MotEvaluator(max_boxes, max_ids, max_frames)
    try:
        ev.set_gt(frames, gts)
        out = ev.run_device(rows, base, n, int(n_groups), BENCHMARKS[benchmark], row_stride)
    finally:
        ev.close()
    res = []
    for rec in out:
        r = {nm: _unpack(rec[k], metrics) for k, nm in enumerate(names)}
        r["COMBINED"] = _unpack(rec[len(names)], metrics)
        res.append(r)
    return res


def mot_summary(res: dict) -> dict:
    """The COMBINED row under ``parse_mot_results``' keys (``val.py:190-219``): floats x100 for
    the ratio metrics, integer counts for IDSW and IDs (its ``int_fields``)."""
    c = res["COMBINED"]
    return {"HOTA": 100.0 * c["HOTA"]["HOTA"], "AssA": 100.0 * c["HOTA"]["AssA"],
            "AssRe": 100.0 * c["HOTA"]["AssRe"], "MOTA": 100.0 * c["CLEAR"]["MOTA"],
            "IDSW": int(c["CLEAR"]["IDSW"]), "IDF1": 100.0 * c["Identity"]["IDF1"],
            "IDs": int(c["Count"]["IDs"])}

"""MOT evaluation I/O and the many-sequence runner.

Reference path replaced (muntherr/boxmot @ /root/reference):
  * detections / embeddings: ``engine/val.py:157-187`` appends ``np.savetxt(fmt='%f')`` text (a
    ``#`` header line, rows ``frame x1 y1 x2 y2 conf cls`` and ``F`` floats per row);
    ``utils/dataloaders/MOT17.py:147-200`` reloads them with ``np.loadtxt`` and selects each
    frame's rows by mask.  Here the text is parsed once by ``bx_txt_read`` (strtod: the same
    correctly rounded doubles as numpy) and packed into one binary file per sequence — header,
    frame table, float64 detection rows grouped by frame, float64 embeddings — that later runs
    memory-map.
  * results: ``engine/utils.py:101-173`` ``convert_to_mot_format`` + ``write_mot_results``
    (``bx_mot_format`` / ``bx_mot_write``, byte-identical lines).
  * the process pool of ``engine/val.py:357-405`` (one tracker per sequence per process):
    ``run_sequences`` drives ALL sequences through one batched engine handle, frame index by
    frame index; a sequence without detections at a frame is not updated (``val.py:347``).
    With ``resident=True`` (DeepOcSort, HybridSort) the per-frame assembly and the row formatting run on the
    device too (``include/bxfeed.h``): one upload, one copy back.

Everything else here is host code in libbxassoc.so; the trackers run on the MI355X engine.
"""
from __future__ import annotations

import ctypes as C
import struct
from pathlib import Path

import numpy as np

from . import _native as N

MAGIC = b"BXMOTSEQ"
_HDR = struct.Struct("<8sIIqII")  # magic, version, header bytes, rows, emb_dim, frames


def load_txt(path) -> np.ndarray:
    """``np.loadtxt(path, comments='#')`` as a 2-D float64 array (bit-identical values)."""
    L = N.load()
    rows, cols = C.c_int64(), C.c_int32()
    N.check(L.bx_txt_shape(str(path).encode(), C.byref(rows), C.byref(cols)), "bx_txt_shape")
    out = np.empty((rows.value, cols.value), np.float64)
    N.check(L.bx_txt_read(str(path).encode(), out.ctypes.data if out.size else None, rows.value,
                          cols.value), "bx_txt_read")
    return out


def pack_sequence(det_txt, emb_txt, out_path) -> Path:
    """Pack one sequence's det / emb text files (val.py's format) into the binary layout."""
    dets = load_txt(det_txt)
    embs = load_txt(emb_txt) if emb_txt is not None else np.empty((dets.shape[0], 0))
    if dets.shape[0] != embs.shape[0]:
        raise ValueError(f"Row mismatch in {det_txt}")  # MOT17.py:152-153
    return pack_arrays(dets, embs, out_path)


def pack_arrays(dets, embs, out_path) -> Path:
    """Pack one sequence from arrays: dets [rows, 7] (frame, x1, y1, x2, y2, conf, cls) and embs
    [rows, F] or None, values kept as float64 (no round trip through text)."""
    dets = np.asarray(dets, np.float64)
    dets = dets.reshape(dets.shape[0], -1) if dets.size else np.empty((0, 7))
    embs = np.empty((dets.shape[0], 0)) if embs is None else np.asarray(embs, np.float64)
    if dets.shape[0] != embs.shape[0]:
        raise ValueError("detections and embeddings differ in rows")
    if dets.shape[0] and dets.shape[1] != 7:
        raise ValueError("detection rows must be frame, x1, y1, x2, y2, conf, cls")
    fid = dets[:, 0].astype(int) if dets.shape[0] else np.empty(0, int)
    order = np.argsort(fid, kind="stable")  # per frame, the rows in file order (the mask's order)
    frames, first = np.unique(fid[order], return_index=True)
    offs = np.append(first, len(order)).astype(np.int64)
    out_path = Path(out_path)
    hdr_bytes = _HDR.size + 8 * len(frames) + 8 * len(offs)
    with open(out_path, "wb") as f:
        f.write(_HDR.pack(MAGIC, 1, hdr_bytes, dets.shape[0], embs.shape[1], len(frames)))
        f.write(frames.astype(np.int64).tobytes())
        f.write(offs.tobytes())
        f.write(np.ascontiguousarray(dets[order][:, 1:7], np.float64).tobytes())
        f.write(np.ascontiguousarray(embs[order], np.float64).tobytes())
    return out_path


class BinSequence:
    """A packed sequence, memory-mapped: ``frame(fid) -> (dets [n,6], embs [n,F])`` exactly as
    MOT17Sequence yields them (``dets[mask, 1:]``, ``embs[mask]``)."""

    def __init__(self, path):
        self.path = Path(path)
        with open(self.path, "rb") as f:
            magic, ver, hdr, rows, F, nf = _HDR.unpack(f.read(_HDR.size))
        if magic != MAGIC or ver != 1:
            raise ValueError(f"{path}: not a packed MOT sequence")
        self.rows, self.emb_dim, self.n_frames = rows, F, nf
        self.frame_ids = np.fromfile(self.path, np.int64, nf, offset=_HDR.size)
        self.offsets = np.fromfile(self.path, np.int64, nf + 1, offset=_HDR.size + 8 * nf)
        self._index = {int(k): i for i, k in enumerate(self.frame_ids)}
        self.dets = np.memmap(self.path, np.float64, "r", offset=hdr, shape=(rows, 6)) \
            if rows else np.empty((0, 6))
        self.embs = np.memmap(self.path, np.float64, "r", offset=hdr + 48 * rows,
                              shape=(rows, F)) if rows and F else np.empty((rows, F))

    def frame(self, fid: int):
        i = self._index.get(int(fid))
        if i is None:
            return np.empty((0, 6)), np.empty((0, self.emb_dim))
        a, b = self.offsets[i], self.offsets[i + 1]
        return np.asarray(self.dets[a:b]), np.asarray(self.embs[a:b])


def convert_to_mot_format(tracks: np.ndarray, frame_idx: int) -> np.ndarray:
    """engine/utils.py:101-133 (numpy branch): [n, >=7] tracker rows -> [n, 9] float64."""
    t = np.ascontiguousarray(np.asarray(tracks, np.float64))
    if t.size == 0:
        return np.empty((0, 9))
    t = t.reshape(t.shape[0], -1)
    out = np.empty((t.shape[0], 9), np.float64)
    N.check(N.load().bx_mot_format(t.ctypes.data, t.shape[0], t.shape[1], int(frame_idx),
                                   out.ctypes.data), "bx_mot_format")
    return out


def write_mot_results(txt_path, mot_results: np.ndarray | None) -> None:
    """engine/utils.py:152-173: create the file (and its directory), append the rows."""
    if mot_results is None:
        return
    p = Path(txt_path)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.touch(exist_ok=True)
    m = np.ascontiguousarray(np.asarray(mot_results, np.float64))
    if m.size:
        N.check(N.load().bx_mot_write(str(p).encode(), m.ctypes.data, m.shape[0], 1),
                "bx_mot_write")


# ------------------------------------------------------------------------------ the runner
def _batched_engine(tracker_type: str, n_seq: int, emb_dim: int, tracker_kwargs: dict,
                    n_classes: int = 0, occlusion: str = "host"):
    """One engine handle for n_seq sequences, parameterised exactly as the drop-in tracker
    `tracker_type` is by `tracker_kwargs` (create_tracker's YAML defaults when empty).
    n_classes > 0 (deepocsort, hybridsort): the per_class mode, n_classes class sequences per
    sequence (step_classes)."""
    if n_classes and tracker_type not in ("deepocsort", "hybridsort"):
        raise NotImplementedError(
            f"run_sequences(n_classes=...) is the per_class mode of deepocsort and hybridsort; "
            f"for {tracker_type} pass per_class in tracker_kwargs")
    if tracker_type == "deepocsort":
        # not in create_tracker's table and without a YAML: the drop-in's constructor (its
        # defaults with empty tracker_kwargs) decides the parameters; per_class in tracker_kwargs
        # raises there, the mode is asked for with n_classes
        from .engine import DeepOcsortEngine
        from .trackers.deepocsort import DeepOcSort, DeepOcSortPerClass

        tr = DeepOcSortPerClass(nr_classes=n_classes, **tracker_kwargs) if n_classes \
            else DeepOcSort(**tracker_kwargs)
        if tr.engine is not None:  # (embedding_off builds the drop-in's own engine at once)
            tr.engine.close()
        tc, dc = tr._caps
        eng = DeepOcsortEngine(n_seq=n_seq * (tr.nr_classes if tr.per_class else 1), track_cap=tc,
                               det_cap=dc, emb_dim=emb_dim, params=tr._params)
        eng.n_classes = tr.nr_classes if tr.per_class else 0
        return eng, np.float32, 8
    if tracker_type == "hybridsort":
        # as deepocsort; det_thresh has no default in the reference's constructor: the drop-in's
        # engine parameters' 0.3 stands in when tracker_kwargs leaves it out
        import dataclasses

        from .engine import (HybridsortCmcEngine, HybridsortCmcParams, HybridsortEngine,
                             HybridsortParams)
        from .trackers.hybridsort import HybridSort, HybridSortPerClass

        kw = dict(reid_weights=None, device=None, half=False,
                  det_thresh=HybridsortParams().det_thresh)
        kw.update(tracker_kwargs)
        # ECC is an attribute of the drop-in, not a constructor argument (as in the reference):
        # in tracker_kwargs it asks for the engine that takes warps, every sequence's switch on
        ecc = bool(kw.pop("ECC", False))
        tr = HybridSortPerClass(nr_classes=n_classes, **kw) if n_classes else HybridSort(**kw)
        tc, dc = tr._caps
        cls, par = HybridsortEngine, tr._params
        if ecc:
            cls = HybridsortCmcEngine
            par = HybridsortCmcParams(**dataclasses.asdict(par), ECC=True)
        eng = cls(n_seq=n_seq * (tr.nr_classes if tr.per_class else 1), track_cap=tc, det_cap=dc,
                  emb_dim=emb_dim, params=par)
        eng.n_classes = tr.nr_classes if tr.per_class else 0
        return eng, np.float32, 8
    from .engine import BoostEngine, Engine, OcsortEngine, SsEngine
    from .tracker_zoo import create_tracker

    tr = create_tracker(tracker_type, evolve_param_dict=tracker_kwargs or None) \
        if tracker_kwargs else create_tracker(tracker_type)
    if tracker_type == "bytetrack":
        e = tr.engine
        return Engine("bytetrack", n_seq=n_seq, track_cap=e.track_cap, det_cap=e.det_cap,
                      params=e.params), np.float32, 8
    if tracker_type == "botsort":
        tc, dc = tr._caps
        return Engine("botsort", n_seq=n_seq, track_cap=tc, det_cap=dc, emb_dim=emb_dim,
                      emb_f64=True, params=tr._params), np.float32, 8
    if tracker_type == "ocsort":
        e = tr.engine
        return OcsortEngine(n_seq=n_seq, track_cap=e.track_cap, det_cap=e.det_cap,
                            params=e.params), np.float32, 8
    if tracker_type == "boosttrack":
        tc, dc = tr._caps
        return BoostEngine(n_seq=n_seq, track_cap=tc, det_cap=dc,
                           emb_dim=emb_dim if tr._params.with_reid else 0,
                           params=tr._params), np.float32, 8
    if tracker_type == "strongsort":
        tc, dc, vc = tr._caps
        if occlusion == "device" and tr.handle_occlusions:
            # the occlusion pass closes every frame on the device: no host handler
            from .engine import SsTableEngine

            eng = SsTableEngine(n_seq=n_seq, track_cap=tc, det_cap=dc, emb_dim=emb_dim,
                                vec_cap=vc, params=tr._params)
            eng.set_occlusion(0, True, tr.occlusion_threshold)
            eng.occlusion_threshold = None
            return eng, np.float64, 10
        eng = SsEngine(n_seq=n_seq, track_cap=tc, det_cap=dc, emb_dim=emb_dim, vec_cap=vc,
                       params=tr._params)
        # handle_occlusions: the host post-process runs per sequence after each batched step
        eng.occlusion_threshold = tr.occlusion_threshold if tr.handle_occlusions else None
        return eng, np.float64, 10
    raise NotImplementedError(f"{tracker_type} is not on the engine")


RESIDENT_TRACKERS = ("deepocsort", "hybridsort")  # trackers run_sequences(resident=True) drives


def _step(eng, tracker_type: str, dets, det_off, embs, out, out_count, seq0: int, nseq: int,
          warps=None):
    """One frame of sequences [seq0, seq0 + nseq) on a DeepOcsortEngine / HybridsortEngine:
    ``step``, or ``step_classes`` on a per_class engine.  warps: the run's [nseq, 6] block of a
    warp table (never with a per_class engine).  The two families differ in where ``step`` takes
    its warps: DeepOCSort's as the fourth argument, HybridSort's as a keyword."""
    C = getattr(eng, "n_classes", 0)
    if tracker_type == "hybridsort":
        if C:
            eng.step_classes(dets, det_off, embs, out, out_count, C, seq0=seq0, nseq=nseq)
        else:
            kw = {} if warps is None else {"warps": warps}  # (a plain engine takes none)
            eng.step(dets, det_off, embs, out, out_count, seq0=seq0, nseq=nseq, **kw)
    elif C:
        eng.step_classes(dets, det_off, embs, None, out, out_count, C, seq0=seq0, nseq=nseq)
    else:
        eng.step(dets, det_off, embs, warps, out, out_count, seq0=seq0, nseq=nseq)


def _resident_results(eng, tracker_type: str, seqs, fids, F: int, ddt, warps=None) -> list:
    """The frame loop of run_sequences with the sequences resident in HBM (engine.SequenceFeeder):
    one upload, per frame index one gather launch, the steps of its runs and one append launch,
    one copy back.  Returns each sequence's MOT rows [n, 9].  warps: [T, S, 6] device tensor or
    None; a run's block goes to its step."""
    from .engine import SequenceFeeder

    feed_emb = F if getattr(eng, "emb_dim", 0) else 0
    dets, embs, tables = [], [], []
    for s, f in zip(seqs, fids):
        if F and s.rows and s.emb_dim not in (0, F):
            raise ValueError(f"{s.path}: embedding dim {s.emb_dim} != {F}")
        start, cnt = np.zeros(len(f), np.int64), np.zeros(len(f), np.int64)
        # (a sequence packed without embeddings among ones that have them is never stepped)
        for i, x in enumerate(f if (s.emb_dim or not F) else ()):
            j = s._index.get(int(x))
            if j is not None:
                start[i], cnt[i] = s.offsets[j], s.offsets[j + 1] - s.offsets[j]
        tables.append((start, cnt, np.asarray(f, np.int64)))
        dets.append(np.asarray(s.dets).astype(ddt))
        embs.append(s.embs if s.emb_dim == feed_emb else np.zeros((s.rows, feed_emb)))
    feed = SequenceFeeder(dets, embs, tables, feed_emb)
    try:
        for t in range(feed.n_frames):
            runs = feed.schedule[t]
            if not runs:
                continue
            feed.gather(t)
            for k, ns, _, pd, po, pe, pout, pcnt in runs:
                _step(eng, tracker_type, pd, po, pe, pout, pcnt, k, ns,
                      None if warps is None else warps[t, k: k + ns])
            feed.append(t)
        if eng.status() != 0:
            raise RuntimeError(f"engine status {eng.status()} (capacity overflow)")
        return feed.results()
    finally:
        feed.close()


def check_occlusion(tracker_type: str, occlusion) -> None:
    """The refusals of the ``occlusion=`` argument of run_sequences and the StrongSort sweeps."""
    if occlusion not in ("host", "device"):
        raise ValueError(f'occlusion must be "host" or "device", got {occlusion!r}')
    if occlusion == "device" and tracker_type != "strongsort":
        raise ValueError(f'occlusion="device" is StrongSort\'s occlusion pass; {tracker_type} has '
                         "no occlusion handling")


def raise_device_occlusion(eng, names) -> None:
    """After a run with the occlusion pass on the device: the reference's TypeError for the first
    sequence with a latched mutual occlusion, RuntimeError for a full buffer pool."""
    if not hasattr(eng, "occ_cap"):  # (handle_occlusions=False: no pass on this engine)
        return
    for q in range(eng.n_seq):
        mf = eng.occlusion(q)["mutual_frame"]
        if mf:
            raise TypeError(f"'int' object is not iterable (mutual occlusion in sequence "
                            f"{names[q % len(names)]}, engine sequence {q}, at its update {mf}: "
                            "the reference's _resolve_mutual_occlusion)")
    # status 2 is also what a frame with more detections than det_cap latches: the pool is named
    # only where a sequence's pool is in fact full
    if eng.status() == 2 and any(eng.occlusion(q)["n_buffered"] >= eng.occ_cap
                                 for q in range(eng.n_seq)):
        raise RuntimeError(f"engine status 2 (capacity): the occlusion buffer pool of a sequence "
                           f"is full, occ_cap = {eng.occ_cap} tracks with buffered features at "
                           "once (or a frame's detections exceeded det_cap)")


WARP_TRACKERS = ("botsort", "boosttrack", "strongsort", "deepocsort")  # run_sequences(warps=...)
_ECC_KEYS = ("warp_mode", "eps", "max_iter", "scale", "chunk")


def _check_warp_args(tracker_type: str, tracker_kwargs: dict, n_classes: int, warps, images,
                     cmc):
    """The refusals of run_sequences' warps / images / cmc that need no sequence, no engine and
    no device; returns warp_table's keyword arguments, or ``{"sof": instance}`` for a SOF
    instance (None without ``images``)."""
    if warps is None and images is None:
        if cmc is not None:
            raise ValueError("cmc names how warps are computed from images: give images too")
        return None
    # hybridsort applies warps iff its ECC switch is on (the reference's attribute, False by
    # default): a condition of its own, WARP_TRACKERS names the trackers that always take them
    if tracker_type not in WARP_TRACKERS and not (
            tracker_type == "hybridsort" and tracker_kwargs.get("ECC")):
        raise ValueError(
            f"{tracker_type} takes no camera-motion warp (its engine has none and the "
            f"reference's tracker runs no CMC): warps / images are for {', '.join(WARP_TRACKERS)}")
    if n_classes or tracker_kwargs.get("per_class"):
        raise ValueError("warps / images in a per_class run are not supported: the reference "
                         "calls its CMC once per class call")
    if tracker_kwargs.get("cmc_off") or tracker_kwargs.get("use_ecc") is False:
        raise ValueError("the tracker's camera-motion compensation is switched off in "
                         "tracker_kwargs (cmc_off / use_ecc): it would not apply the warps")
    if images is None:
        if cmc is not None:
            raise ValueError("cmc goes with images; warps are taken as they are")
        return None
    if warps is not None:
        raise ValueError("give images (with cmc) or warps, not both")
    if cmc is None:
        raise ValueError('images need cmc: "ecc", a dict of ECC settings or a SOF instance')
    from . import cmc as M

    if isinstance(cmc, M.SOF):
        cmc._params()  # SOF's own refusals (min_distance, block_size, ranges)
        return {"sof": cmc}
    if isinstance(cmc, str) and cmc == "ecc":
        return {}
    if not isinstance(cmc, dict) or set(cmc) - set(_ECC_KEYS):
        raise ValueError(f'cmc must be "ecc", a dict with keys among {", ".join(_ECC_KEYS)} or '
                         "a boxmot_amd.SOF instance")
    return dict(cmc)


def _flow_warps(names, seqs, fids, F: int, warps, images, ecc_kw):
    """The [T, S, 6] float64 device tensor run_sequences hands its engines, T the most iterated
    frames of a sequence: a WarpTable's warps, plain per-sequence arrays, or the table computed
    from images, each value rounded to float32 (what the reference's cmc.apply returns).  The
    shapes are checked before anything touches the device."""
    from . import cmc as M

    S, T = len(seqs), max([len(f) for f in fids] + [0])
    if images is not None:
        missing = [nm for nm in names if nm not in images]
        if missing:
            raise ValueError(f"no images for {', '.join(missing)}")
        stepped = []
        for s, f in zip(seqs, fids):  # the flow's own stepping rule
            m = np.zeros(len(f), bool)
            for t, x in enumerate(f):
                d, e = s.frame(x)
                m[t] = bool(d.size and (e.size or not F))
            stepped.append(m)
        for nm, m in zip(names, stepped):
            if not callable(images[nm]) and len(images[nm]) != m.size:
                raise ValueError(f"{nm}: {len(images[nm])} images for {m.size} iterated frames")
        if "sof" in ecc_kw:
            tab = M.sof_warp_table([images[nm] for nm in names], stepped, sof=ecc_kw["sof"])
        else:
            tab = M.warp_table([images[nm] for nm in names], stepped, **ecc_kw)
        try:
            return tab.warps.to(dtype=_torch().float32).to(dtype=_torch().float64).contiguous()
        finally:
            tab.close()
    if isinstance(warps, M.WarpTable):
        if warps.warps is None or tuple(warps.warps.shape) != (T, S, 6):
            raise ValueError(f"the warp table is not [{T}, {S}, 6]: it was built for other "
                             "sequences or frames")
        return warps.warps.to(dtype=_torch().float32).to(dtype=_torch().float64).contiguous()
    if not hasattr(warps, "keys"):
        raise ValueError("warps must be a cmc.WarpTable or a mapping name -> [n_frames, 6]")
    host = np.zeros((T, S, 6), np.float64)
    host[:, :, 0] = host[:, :, 4] = 1.0
    for k, (nm, f) in enumerate(zip(names, fids)):
        if nm not in warps:
            raise ValueError(f"no warps for {nm}")
        w = np.asarray(warps[nm], np.float64)
        if w.shape not in ((len(f), 6), (len(f), 2, 3)):
            raise ValueError(f"{nm}: warps of shape {w.shape} for {len(f)} iterated frames")
        host[: len(f), k] = w.reshape(len(f), 6).astype(np.float32)
    return _torch().from_numpy(host).cuda()


def _torch():
    import torch

    return torch


def run_sequences(tracker_type: str, sequences: dict, exp_dir, frame_ids: dict | None = None,
                  frame_sizes: dict | None = None, tracker_kwargs: dict | None = None,
                  gsi: bool = False, gsi_interval: int = 20, gsi_tau: float = 10,
                  resident: bool = False, n_classes: int = 0, occlusion: str = "host", warps=None,
                  images: dict | None = None, cmc=None) -> dict:
    """process_sequence (val.py:304-354) for every sequence at once.

    sequences: name -> packed file (pack_sequence) or BinSequence; frame_ids: name -> the frames
    to iterate (the image list; default: the frames that have detections); frame_sizes: name ->
    (w, h) of its images (OCSort's centroid mode).  Writes ``exp_dir/<name>.txt`` and returns
    name -> the frame ids iterated.  Sequence k's track ids start at 1, as in a fresh process.
    gsi: apply the GSI post-processing (postprocessing.gsi, with gsi_interval / gsi_tau) to
    exp_dir after the files are written, as the reference's evaluation flow does last.
    resident: keep the sequences' detections and embeddings and the result rows in device memory
    for the whole run (include/bxfeed.h) instead of assembling every frame on the host; the files
    are byte-identical.  Only for the trackers in RESIDENT_TRACKERS.
    n_classes: > 0 runs deepocsort / hybridsort in their per_class mode over classes
    0..n_classes-1 (DeepOcSortPerClass / HybridSortPerClass per sequence; ``per_class`` in
    tracker_kwargs raises for these two, as their plain constructors do), with the class split and
    the id merge on the device, resident or not.
    Camera-motion compensation (the reference's ``tracker.update(dets, img, embs)`` runs its CMC
    on every stepped frame), for the trackers in WARP_TRACKERS and for hybridsort with
    ``ECC=True`` in tracker_kwargs (the reference's switch; without it hybridsort is refused as
    before), resident or not; left out, no warp is applied, as before:
    warps: a ``cmc.WarpTable`` over these sequences (in their order) and their iterated frames,
    or a mapping name -> ``[n_frames, 6]`` (or ``[n_frames, 2, 3]``) array of the warp at every
    iterated frame of that sequence (rows of frames that are not stepped are not read), e.g.
    from ``SofBatch``.
    images, cmc: name -> the sequence's images (``cmc.warp_table``'s array or callable), and
    ``"ecc"`` or a dict of ECC settings (warp_mode, eps, max_iter, scale, chunk): the flow derives
    the stepped frames, builds the table with ``cmc.warp_table``, runs and closes it.  A
    ``boxmot_amd.SOF`` instance as ``cmc`` means what a drop-in with ``tracker.cmc = SOF(...)``
    does (the reference's DeepOCSort default): the table comes from ``cmc.sof_warp_table`` with
    the instance's settings; the instance itself is neither run nor changed, and its own refusals
    (``min_distance`` above 1, ``block_size`` other than 3, ranges) are raised first.  The string
    ``"sof"`` is not accepted.
    Every warp reaches the engine rounded to float32, the type the reference's ``cmc.apply``
    returns and the drop-ins pass on.  ValueError, before anything is built: a tracker outside
    WARP_TRACKERS, a per_class run, ``images`` without ``cmc`` or with ``warps``, a table or an
    array that does not match the sequences and their iterated frames.
    occlusion: where StrongSort's ``handle_occlusions`` runs.  ``"host"`` (default): an
    ``OcclusionHandler`` per sequence after every step, reading tracks back and writing edits.
    ``"device"`` (strongsort only): the engine's occlusion pass (``SsTableEngine.set_occlusion``)
    ends every frame on the device and no handler is built; the files are byte-identical.
    Ignored when the config has ``handle_occlusions=False``.  Where the host handler raises the
    reference's ``TypeError`` on a mutual occlusion in the middle of the run, the device flow
    raises it after the run, naming the sequence and its update count; either way before any
    file is written.  A full buffer pool is a ``RuntimeError`` naming ``occ_cap``.  ``ValueError``,
    before anything is built, for another tracker or another value.
    """
    check_occlusion(tracker_type, occlusion)
    if resident and tracker_type not in RESIDENT_TRACKERS:
        raise NotImplementedError(
            f"run_sequences(resident=True) is not available for {tracker_type}: the "
            f"device-resident feeder drives {', '.join(RESIDENT_TRACKERS)} only")
    ecc_kw = _check_warp_args(tracker_type, tracker_kwargs or {}, n_classes, warps, images, cmc)
    import torch

    names = list(sequences)
    seqs = [s if isinstance(s, BinSequence) else BinSequence(s) for s in sequences.values()]
    S = len(seqs)
    F = max([s.emb_dim for s in seqs] + [0])
    fids = [np.asarray(frame_ids[nm]) if frame_ids and nm in frame_ids else s.frame_ids
            for nm, s in zip(names, seqs)]
    table = None
    if warps is not None or images is not None:
        table = _flow_warps(names, seqs, fids, F, warps, images, ecc_kw)
    if occlusion == "device":
        eng, ddt, ncol = _batched_engine(tracker_type, S, F, tracker_kwargs or {}, n_classes,
                                         occlusion=occlusion)
    else:
        eng, ddt, ncol = _batched_engine(tracker_type, S, F, tracker_kwargs or {}, n_classes) \
            if n_classes else _batched_engine(tracker_type, S, F, tracker_kwargs or {})
    if tracker_type == "ocsort" and frame_sizes:
        for k, nm in enumerate(names):
            if nm in frame_sizes:
                eng.set_frame_size(k, *frame_sizes[nm])
    if tracker_type in ("deepocsort", "hybridsort") and frame_sizes:
        C = getattr(eng, "n_classes", 0) or 1  # (per_class: every class sequence of the sequence)
        for k, nm in enumerate(names):
            if nm in frame_sizes:
                for q in range(k * C, (k + 1) * C):
                    eng.set_frame_size(q, *frame_sizes[nm])
    if resident:
        exp_dir = Path(exp_dir)
        for nm, res in zip(names, _resident_results(eng, tracker_type, seqs, fids, F, ddt, table)):
            write_mot_results(exp_dir / f"{nm}.txt", res if res.size else np.empty((0, 0)))
        if gsi:
            from . import postprocessing

            postprocessing.gsi(exp_dir, interval=gsi_interval, tau=gsi_tau)
        return {nm: list(map(int, f)) for nm, f in zip(names, fids)}
    results = [[] for _ in range(S)]
    occ = None
    if getattr(eng, "occlusion_threshold", None) is not None:
        from .occlusion import OcclusionHandler

        occ = [OcclusionHandler(eng, k, eng.occlusion_threshold) for k in range(S)]
    nupd = [0] * S
    dev = torch.device("cuda")
    for t in range(max([len(f) for f in fids] + [0])):
        frame = []
        for k in range(S):
            if t < len(fids[k]):
                d, e = seqs[k].frame(fids[k][t])
                frame.append((d, e) if d.size and (e.size or not F) else None)
            else:
                frame.append(None)
        k = 0
        while k < S:  # contiguous runs of sequences with an update at this frame index
            if frame[k] is None:
                k += 1
                continue
            k1 = k
            while k1 < S and frame[k1] is not None:
                k1 += 1
            ds = [frame[q][0] for q in range(k, k1)]
            off = np.zeros(k1 - k + 1, np.int32)
            off[1:] = np.cumsum([d.shape[0] for d in ds])
            dd = torch.from_numpy(np.concatenate(ds).astype(ddt)).to(dev)
            od = torch.from_numpy(off).to(dev)
            out = torch.empty((int(off[-1]), ncol), dtype=torch.float64, device=dev)
            cnt = torch.empty(k1 - k, dtype=torch.int32, device=dev)
            wk = None if table is None else table[t, k: k1]  # the run's [nseq, 6] block
            if tracker_type == "ocsort":
                eng.step(dd, od, out, cnt, seq0=k, nseq=k1 - k)
            elif tracker_type in ("deepocsort", "hybridsort"):
                emb = None
                if F and eng.emb_dim:
                    emb = torch.from_numpy(np.concatenate([frame[q][1] for q in range(k, k1)])
                                           .astype(np.float64)).to(dev)
                _step(eng, tracker_type, dd, od, emb, out, cnt, k, k1 - k, wk)
            else:
                emb = None
                if F and getattr(eng, "with_reid", True) and not (
                        tracker_type == "boosttrack" and not eng.emb_dim):
                    emb = torch.from_numpy(np.concatenate([frame[q][1] for q in range(k, k1)])
                                           .astype(np.float64)).to(dev)
                eng.step(dd, od, emb, wk, out, cnt, seq0=k, nseq=k1 - k)
            o, c = out.cpu().numpy(), cnt.cpu().numpy()
            for q in range(k, k1):
                rows = o[off[q - k]: off[q - k] + c[q - k]]
                nupd[q] += 1
                if occ is not None:
                    rows = occ[q](nupd[q], rows)
                if rows.shape[0]:
                    results[q].append(convert_to_mot_format(rows, int(fids[q][t])))
            k = k1
    if occlusion == "device":
        raise_device_occlusion(eng, names)
    if eng.status() != 0:
        raise RuntimeError(f"engine status {eng.status()} (capacity overflow)")
    exp_dir = Path(exp_dir)
    for nm, res in zip(names, results):
        write_mot_results(exp_dir / f"{nm}.txt", np.vstack(res) if res else np.empty((0, 0)))
    if gsi:
        from . import postprocessing

        postprocessing.gsi(exp_dir, interval=gsi_interval, tau=gsi_tau)
    return {nm: list(map(int, f)) for nm, f in zip(names, fids)}

"""Python handle over the native engine (``bx_engine_*`` in include/bxassoc.h).

An ``Engine`` holds ``n_seq`` independent sequences resident in HBM.  ``step`` advances one frame
of a contiguous range of sequences in a single kernel launch (device tensors in, device tensors
out); ``update_host`` is the single-sequence numpy path the drop-in tracker classes use.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
from dataclasses import dataclass

import numpy as np

from . import _native as N

KINDS = {"bytetrack": 0, "botsort": 1}


@dataclass
class EngineParams:
    """Tracker parameters with the reference constructors' defaults."""

    # ByteTrack (bytetrack.py:132-140)
    min_conf: float = 0.1
    track_thresh: float = 0.45
    match_thresh: float = 0.8
    track_buffer: int | None = None  # None → the tracker's own default: 25 ByteTrack, 30 BoT-SORT
    frame_rate: int = 30
    # BoT-SORT (botsort.py:49-66)
    track_high_thresh: float = 0.5
    track_low_thresh: float = 0.1
    new_track_thresh: float = 0.6
    proximity_thresh: float = 0.5
    appearance_thresh: float = 0.25
    fuse_first_associate: bool = False
    with_reid: bool = True


class _NativeHandle:
    """A handle over a ``<prefix>_*`` family of the C ABI: its life and its status."""

    _PREFIX = ""   # "bx_ocsort", ...: every entry point of the family is <prefix>_<name>

    def _fn(self, name):
        return getattr(self._L, f"{self._PREFIX}_{name}")

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._fn("destroy")(h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def status(self) -> int:
        s = C.c_int(0)
        N.check(self._fn("status")(self._h, C.byref(s)), f"{self._PREFIX}_status")
        return s.value


class _NativeEngine(_NativeHandle):
    """What the six tracker engines share on top: create, the sequence-range / stream preamble
    of ``step``, reset and the timing probe.  A class whose C signature or returned keys differ
    keeps its own method."""

    STAGES: list = []  # the probe's stage names, in the C stage order

    def _create(self, cfg) -> None:
        self._L = N.load()
        h = C.c_void_p()
        N.check(self._fn("create")(C.byref(cfg), C.byref(h)), f"{self._PREFIX}_create")
        self._h = h

    def _range(self, seq0, nseq, stream):
        """(nseq, stream) with their defaults: every sequence from seq0, the current stream."""
        return (self.n_seq - seq0 if nseq is None else nseq,
                _current_stream() if stream is None else stream)

    def reset(self, seq0: int = 0, nseq: int | None = None, stream=None):
        nseq = self.n_seq - seq0 if nseq is None else nseq
        N.check(self._fn("reset")(self._h, seq0, nseq, stream), f"{self._PREFIX}_reset")

    def slots_used(self, seq: int = 0) -> int:
        return self.counters(seq)["n_tracks"]

    def probe(self, stage) -> None:
        """Time every launch of one stage with HIP events (name from STAGES or index);
        None/-1 = off."""
        idx = -1 if stage is None else (self.STAGES.index(stage) if isinstance(stage, str)
                                        else int(stage))
        N.check(self._fn("probe")(self._h, idx), f"{self._PREFIX}_probe")

    def probe_read(self):
        """(total ms, launches) of the probed stage since the last read."""
        t, n = C.c_double(), C.c_int()
        N.check(self._fn("probe_read")(self._h, C.byref(t), C.byref(n)), "probe_read")
        return t.value, n.value


class _TrackListEngine(_NativeEngine):
    """The engines whose counter row is (frame_count, id_count, n_tracks): OCSort's family and
    BoostTrack."""

    def counters(self, seq: int = 0) -> dict:
        fc, idc, nt = C.c_int(), C.c_int(), C.c_int()
        N.check(self._fn("counters_host")(self._h, seq, C.byref(fc), C.byref(idc), C.byref(nt)),
                "counters")
        return {"frame_count": fc.value, "id_count": idc.value, "n_tracks": nt.value}

    def set_id_count(self, seq: int, value: int):
        N.check(self._fn("set_id_count")(self._h, seq, int(value), None), "set_id_count")


class _OcsFamilyEngine(_TrackListEngine):
    """OCSort, DeepOCSort and HybridSort: the per-sequence frame size of the centroid mode and
    the three-number frame statistics."""

    def set_frame_size(self, seq: int, w: float, h: float):
        N.check(self._fn("set_frame_size")(self._h, seq, float(w), float(h), None),
                "set_frame_size")

    def frame_stats(self, seq0: int = 0, nseq: int | None = None) -> dict:
        """Last frame over sequences [seq0, seq0+nseq): live tracks, output rows, frame."""
        nseq = self.n_seq - seq0 if nseq is None else nseq
        a = (C.c_int64 * 3)()
        N.check(self._fn("frame_stats_host")(self._h, seq0, nseq, a), "frame_stats")
        return dict(zip(["tracks", "outputs", "frame"], [int(x) for x in a]))


class _SeqTable:
    """Mixin of the six table engines: an engine whose sequences may each run on parameters of
    their own (``<prefix>_set_seq_params_host`` / ``<prefix>_seq_params_host``), the engine of a
    hyper-parameter sweep, K configs x S sequences as K*S sequences of one handle (boxmot_amd.tune).

    The family names ``_SEQ_STRUCT``, the ctypes struct of one entry, and supplies
    ``_seq_struct(p)``, the struct of its parameter dataclass (``ValueError`` for an entry that
    differs from the engine in a field that stays engine-wide), and ``_seq_params_of(o)``, the
    dataclass of a struct, with the engine-wide fields from ``self.params``.  The three stand on
    the plain engine class, beside its mapping of the dataclass to the C config: ``seq_params``
    also serves a plain engine (``TableEngine.seq_params(engine, seq)``), whose handle answers
    the getter without a table."""

    @functools.cached_property
    def _seq_over(self) -> dict:
        """sequence -> its own parameters as they were given, for ``_retable``."""
        return {}

    def set_seq_params(self, seq0: int, params, nseq: int | None = None) -> None:
        """Give sequences [seq0, seq0 + len(params)) parameters of their own: ``params`` is a list
        of the engine's parameter dataclass.  ``None`` clears the override of ``nseq`` sequences
        from seq0 (default: all from seq0).  For use between sequences, at frame 0.  An entry the
        class or the library refuses changes nothing."""
        if params is None:
            n = self.n_seq - seq0 if nseq is None else nseq
            arr = None
        else:
            n = len(params)
            arr = (self._SEQ_STRUCT * max(n, 1))(*[self._seq_struct(p) for p in params])
        N.check(self._fn("set_seq_params_host")(self._h, int(seq0), int(n), arr, None),
                f"{self._PREFIX}_set_seq_params_host")
        for k in range(n):
            if params is None:
                self._seq_over.pop(seq0 + k, None)
            else:
                self._seq_over[seq0 + k] = params[k]

    def seq_params(self, seq: int):
        """The parameters sequence ``seq`` runs on: its own when set, else the engine's."""
        o = self._SEQ_STRUCT()
        N.check(self._fn("seq_params_host")(self._h, int(seq), C.byref(o)),
                f"{self._PREFIX}_seq_params_host")
        return self._seq_params_of(o)

    def _retable(self, e):
        """``grown()``'s tail: copy_state carries no table, so it is set again on ``e``."""
        for k, p in sorted(self._seq_over.items()):
            e.set_seq_params(k, [p])
        return e


class Engine(_NativeEngine):
    _PREFIX = "bx_engine"

    def __init__(self, kind: str, n_seq: int = 1, track_cap: int = 1024, det_cap: int = 384,
                 emb_dim: int = 0, emb_f64: bool = False, params: EngineParams | None = None):
        if kind not in KINDS:
            raise KeyError(kind)
        p = params or EngineParams()
        if p.track_buffer is None:
            p = EngineParams(**{**p.__dict__, "track_buffer": 25 if kind == "bytetrack" else 30})
        self.kind, self.n_seq, self.track_cap, self.det_cap = kind, n_seq, track_cap, det_cap
        self.emb_dim, self.emb_f64, self.params = emb_dim, bool(emb_f64), p
        self.with_reid = kind == "botsort" and p.with_reid
        cfg = N.BxConfig(
            kind=KINDS[kind], n_seq=n_seq, track_cap=track_cap, det_cap=det_cap,
            emb_dim=emb_dim if self.with_reid else 0, emb_f64=int(emb_f64),
            min_conf=p.min_conf, track_thresh=p.track_thresh, match_thresh=p.match_thresh,
            track_buffer=int(p.track_buffer), frame_rate=int(p.frame_rate),
            track_high_thresh=p.track_high_thresh, track_low_thresh=p.track_low_thresh,
            new_track_thresh=p.new_track_thresh, proximity_thresh=p.proximity_thresh,
            appearance_thresh=p.appearance_thresh,
            fuse_first_associate=int(bool(p.fuse_first_associate)), with_reid=int(self.with_reid))
        self._overlap, self._inflight = False, None
        self._create(cfg)

    # ----------------------------------------------------------------------------- lifecycle
    def reset(self, seq0: int = 0, nseq: int | None = None, stream: int | None = None):
        nseq = self.n_seq - seq0 if nseq is None else nseq
        N.check(self._L.bx_engine_reset(self._h, seq0, nseq, stream), "bx_engine_reset")

    # ------------------------------------------------------------------------------- frames
    def step(self, dets, det_off, embs=None, warps=None, out=None, out_count=None, seq0: int = 0,
             nseq: int | None = None, stream=None):
        """One frame for sequences [seq0, seq0+nseq): torch device tensors (or raw pointers).

        dets [sum N,6] float32, det_off [nseq+1] int32, embs [sum N,F] float32/64 or None,
        warps [nseq,6] float64 or None, out [sum N,8] float64, out_count [nseq] int32.
        """
        nseq, stream = self._range(seq0, nseq, stream)
        ptr = _ptr
        N.check(self._L.bx_engine_step(self._h, seq0, nseq, ptr(dets), ptr(det_off), ptr(embs),
                                       ptr(warps), ptr(out), ptr(out_count), stream),
                "bx_engine_step")
        # overlap mode: this step's K5 still reads its inputs after the call returns — hold them
        # so the caching allocator cannot hand their memory out before the next step
        self._inflight = (dets, det_off, embs) if self._overlap else None

    def slots_used(self, seq: int = 0) -> int:
        """Track slots of sequence ``seq`` in use (bx_engine_slots_used_host)."""
        u = C.c_int(0)
        N.check(self._L.bx_engine_slots_used_host(self._h, seq, C.byref(u)), "slots_used")
        return u.value

    # ---- one entry of the per-sequence parameter table (_SeqTable)
    _SEQ_STRUCT = N.BxEngineSeqParams

    def _seq_struct(self, p: EngineParams):
        tb = p.track_buffer
        if tb is None:  # the tracker's own default, as Engine.__init__ resolves it
            tb = 25 if self.kind == "bytetrack" else 30
        return N.BxEngineSeqParams(
            min_conf=p.min_conf, track_thresh=p.track_thresh,
            track_high_thresh=p.track_high_thresh, track_low_thresh=p.track_low_thresh,
            new_track_thresh=p.new_track_thresh, proximity_thresh=p.proximity_thresh,
            appearance_thresh=p.appearance_thresh,
            fuse_first_associate=int(bool(p.fuse_first_associate)),
            match_thresh=p.match_thresh, track_buffer=int(tb), frame_rate=int(p.frame_rate))

    def _seq_params_of(self, o) -> EngineParams:
        return EngineParams(
            min_conf=o.min_conf, track_thresh=o.track_thresh, match_thresh=o.match_thresh,
            track_buffer=o.track_buffer, frame_rate=o.frame_rate,
            track_high_thresh=o.track_high_thresh, track_low_thresh=o.track_low_thresh,
            new_track_thresh=o.new_track_thresh, proximity_thresh=o.proximity_thresh,
            appearance_thresh=o.appearance_thresh,
            fuse_first_associate=bool(o.fuse_first_associate), with_reid=self.params.with_reid)

    def grown(self, track_cap: int, det_cap: int) -> "Engine":
        """A new engine with larger capacities holding this one's tracker state
        (bx_engine_copy_state): the reference's lists are unbounded."""
        e = Engine(self.kind, self.n_seq, track_cap, det_cap, self.emb_dim, self.emb_f64,
                   self.params)
        N.check(self._L.bx_engine_copy_state(e._h, self._h), "bx_engine_copy_state")
        if self._overlap:
            e.set_overlap(True)
        return e

    def inputs_released(self, stream=None) -> None:
        """Overlap mode: order ``stream`` after the last step's last read of its inputs
        (bx_engine_inputs_released) — before refilling a reused input buffer in place."""
        if stream is None:
            stream = _current_stream()
        N.check(self._L.bx_engine_inputs_released(self._h, stream), "bx_engine_inputs_released")

    def lap_ties(self, seq0: int = 0, nseq: int | None = None) -> int:
        """Associations re-solved by lapx's lapjv because their optimum was tied
        (bx_engine_lap_ties_host), summed over sequences [seq0, seq0+nseq)."""
        nseq = self.n_seq - seq0 if nseq is None else nseq
        t = C.c_int64(0)
        N.check(self._L.bx_engine_lap_ties_host(self._h, seq0, nseq, C.byref(t)), "lap_ties")
        return int(t.value)

    def lap_components(self, seq0: int = 0, nseq: int | None = None) -> dict:
        """LAP components solved by the per-lane SSP (past the register path) and by the
        wave-parallel SSP (more than 3 rows) since creation (bx_engine_lap_components_host), over
        [seq0, seq0+nseq)."""
        nseq = self.n_seq - seq0 if nseq is None else nseq
        a = (C.c_int64 * 3)()
        N.check(self._L.bx_engine_lap_components_host(self._h, seq0, nseq, a), "lap_components")
        return {"lane": int(a[0]), "wave": int(a[1]), "helper": int(a[2])}

    def force_assoc_build(self, mode: int) -> None:
        """-1: the association kernel build is picked per launch from the helper-wave cue
        (default); 0 / 1: always the wave-0-only / helper-wave build (bx_engine_force_assoc_build)."""
        N.check(self._L.bx_engine_force_assoc_build(self._h, int(mode)), "force_assoc_build")

    def set_lap_stats(self, on: bool = True) -> None:
        """Count LAP components for lap_components (bx_engine_set_lap_stats; off by default)."""
        N.check(self._L.bx_engine_set_lap_stats(self._h, int(bool(on))), "bx_engine_set_lap_stats")

    def update_host(self, seq: int, dets: np.ndarray, embs: np.ndarray | None = None,
                    warp: np.ndarray | None = None) -> np.ndarray:
        """One frame of one sequence from host arrays; returns float64 [M, 8]."""
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        e = None
        if self.with_reid and n:
            if embs is None:
                raise ValueError("BoT-SORT with_reid needs embeddings (ReID inference is outside "
                                 "the association engine)")
            e = np.ascontiguousarray(embs, dtype=np.float64 if self.emb_f64 else np.float32)
            if e.shape != (n, self.emb_dim):
                raise ValueError(f"embs shape {e.shape} != ({n}, {self.emb_dim})")
        w = None if warp is None else np.ascontiguousarray(warp, np.float64).reshape(6)
        out = np.empty((max(n, 1), 8), np.float64)
        m = C.c_int(0)
        N.check(self._L.bx_engine_update_host(
            self._h, seq, d.ctypes.data if n else None, n,
            e.ctypes.data if e is not None else None, w.ctypes.data if w is not None else None,
            out.ctypes.data, C.byref(m), None), "bx_engine_update_host")
        return out[: m.value].copy()

    def update_classes_host(self, seq: int, dets: np.ndarray, embs: np.ndarray | None = None,
                            warp: np.ndarray | None = None, n_classes: int = 80) -> np.ndarray:
        """per_class=True frame of one sequence (bx_engine_update_classes_host): one update per
        class id on that class's detections, active lists per class, lost list shared.  ``warp``:
        None, one 2x3 warp for every class call, or [n_classes, 2, 3] — the reference calls
        cmc.apply once per class call (botsort.py:218)."""
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        e = None
        if self.with_reid and n:
            if embs is None:
                raise ValueError("BoT-SORT with_reid needs embeddings (ReID inference is outside "
                                 "the association engine)")
            e = np.ascontiguousarray(embs, dtype=np.float64 if self.emb_f64 else np.float32)
            if e.shape != (n, self.emb_dim):
                raise ValueError(f"embs shape {e.shape} != ({n}, {self.emb_dim})")
        w = _class_warps(warp, n_classes)
        out = np.empty((max(n, 1), 8), np.float64)
        m = C.c_int(0)
        N.check(self._L.bx_engine_update_classes_host(
            self._h, seq, d.ctypes.data if n else None, n,
            e.ctypes.data if e is not None else None, w.ctypes.data if w is not None else None,
            int(n_classes), out.ctypes.data, C.byref(m), None), "bx_engine_update_classes_host")
        return out[: m.value].copy()

    # ---------------------------------------------------------------------------- state I/O
    STAGES = ["det_features", "predict", "gate", "cosine", "assoc", "update", "cov_predict",
              "features", "finish"]  # bx_stage order (include/bxassoc.h)

    def set_early_features(self, on: bool = True) -> None:
        """Start each full step's detection-feature kernel at once on a stream of its own
        (bx_engine_set_early_features): the caller guarantees a step's inputs are complete when
        the step is called."""
        N.check(self._L.bx_engine_set_early_features(self._h, int(bool(on))),
                "bx_engine_set_early_features")

    def set_cosine_mode(self, mode: int) -> None:
        """0: the embedding-distance kernel picked from the feature width (default); 1: always
        the element-by-element restatement (bx_engine_set_cosine_mode).  Same bits either way."""
        N.check(self._L.bx_engine_set_cosine_mode(self._h, int(mode)), "bx_engine_set_cosine_mode")

    def embdist_host(self, seq: int = 0):
        """(pair words uint32 [n] = slot << 16 | detection, distances float64 [n]) of the last
        step's gated pairs of sequence ``seq`` (bx_engine_embdist_host), in the gate's order."""
        cap = self.track_cap * self.det_cap
        pairs, dist = np.empty(cap, np.uint32), np.empty(cap, np.float64)
        n = C.c_int(0)
        N.check(self._L.bx_engine_embdist_host(self._h, seq, cap, pairs.ctypes.data,
                                               dist.ctypes.data, C.byref(n)),
                "bx_engine_embdist_host")
        return pairs[: n.value].copy(), dist[: n.value].copy()

    def set_overlap(self, on: bool = True) -> None:
        """Leave each step's feature EMA (K5) unjoined on the side stream (bx_engine_set_overlap):
        the caller keeps a step's input tensors unmodified until the next step is enqueued."""
        N.check(self._L.bx_engine_set_overlap(self._h, int(bool(on))), "bx_engine_set_overlap")
        self._overlap = bool(on)
        if not on:
            self._inflight = None

    def frame_stats(self, seq0: int = 0, nseq: int = None) -> dict:
        """Last frame's unit counts summed over sequences (bench byte accounting)."""
        nseq = self.n_seq - seq0 if nseq is None else nseq
        a = (C.c_int64 * 7)()
        N.check(self._L.bx_engine_frame_stats_host(self._h, seq0, nseq, a), "frame_stats")
        keys = ["dets", "high", "active", "lost", "records", "pairs", "frame"]
        return dict(zip(keys, [int(x) for x in a]))

    def counters(self, seq: int = 0) -> dict:
        fc, idc, na, nl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        N.check(self._L.bx_engine_counters_host(self._h, seq, C.byref(fc), C.byref(idc),
                                                C.byref(na), C.byref(nl)), "counters")
        return {"frame_count": fc.value, "id_count": idc.value, "n_active": na.value,
                "n_lost": nl.value}

    def set_id_count(self, seq: int, value: int):
        N.check(self._L.bx_engine_set_id_count(self._h, seq, int(value), None), "set_id_count")

    def tracks(self, seq: int = 0) -> dict:
        """Host snapshot of the live tracks: active list then lost list."""
        cap = self.track_cap
        ids = np.zeros(cap, np.int32)
        st = np.zeros(cap, np.int32)
        act = np.zeros(cap, np.int32)
        fid = np.zeros(cap, np.int32)
        sf = np.zeros(cap, np.int32)
        mean = np.zeros((cap, 8))
        cov = np.zeros((cap, 8, 8))
        na, nl = C.c_int(), C.c_int()
        N.check(self._L.bx_engine_tracks_host(
            self._h, seq, cap, ids.ctypes.data, st.ctypes.data, act.ctypes.data, fid.ctypes.data,
            sf.ctypes.data, mean.ctypes.data, cov.ctypes.data, C.byref(na), C.byref(nl)),
            "tracks")
        n = na.value + nl.value
        return {"n_active": na.value, "n_lost": nl.value, "id": ids[:n], "state": st[:n],
                "is_activated": act[:n].astype(bool), "frame_id": fid[:n],
                "start_frame": sf[:n], "mean": mean[:n], "covariance": cov[:n]}

    def class_tracks(self, seq: int, n_classes: int) -> list:
        """per_class mode: each class's active list (``per_class_active_tracks``), as
        ``tracks``-style dicts in class order."""
        cap = self.track_cap
        off = np.zeros(n_classes + 1, np.int32)
        ids = np.zeros(cap, np.int32)
        st = np.zeros(cap, np.int32)
        act = np.zeros(cap, np.int32)
        fid = np.zeros(cap, np.int32)
        sf = np.zeros(cap, np.int32)
        mean = np.zeros((cap, 8))
        cov = np.zeros((cap, 8, 8))
        N.check(self._L.bx_engine_class_tracks_host(
            self._h, seq, n_classes, cap, off.ctypes.data, ids.ctypes.data, st.ctypes.data,
            act.ctypes.data, fid.ctypes.data, sf.ctypes.data, mean.ctypes.data, cov.ctypes.data),
            "class_tracks")
        out = []
        for c in range(n_classes):
            a, b = int(off[c]), int(off[c + 1])
            out.append({"n_active": b - a, "n_lost": 0, "id": ids[a:b], "state": st[a:b],
                        "is_activated": act[a:b].astype(bool), "frame_id": fid[a:b],
                        "start_frame": sf[a:b], "mean": mean[a:b], "covariance": cov[a:b]})
        return out

    def state_set(self, seq: int, ids, mean=None, covariance=None) -> None:
        """Write the Kalman mean [n,8] / covariance [n,8,8] of live tracks by id (host code
        editing STrack.mean / .covariance in the reference)."""
        n, ids, m, c = _state_arrays(ids, mean, covariance, 8, 64)
        N.check(self._L.bx_engine_state_set_host(self._h, seq, n, ids.ctypes.data, _p(m), _p(c)),
                "state_set")



class TableEngine(_SeqTable, Engine):
    """An ``Engine`` with per-sequence ``EngineParams`` (``_SeqTable``; include/bxassoc.h,
    boxmot_amd.tune.sweep_bot).  ``with_reid``, which is not part of the table, the capacities and
    the embedding width stay the engine's."""

    def grown(self, track_cap: int, det_cap: int) -> "TableEngine":
        """As Engine.grown, with the table."""
        e = TableEngine(self.kind, self.n_seq, track_cap, det_cap, self.emb_dim, self.emb_f64,
                        self.params)
        N.check(self._L.bx_engine_copy_state(e._h, self._h), "bx_engine_copy_state")
        if self._overlap:
            e.set_overlap(True)
        return self._retable(e)


def _class_warps(warp, n_classes: int):
    """Per-class-call warps as the C ABI takes them: [n_classes][6] float64 or None."""
    if warp is None:
        return None
    w = np.asarray(warp, np.float64)
    if w.size == 6:
        w = np.broadcast_to(w.reshape(1, 6), (int(n_classes), 6))
    if w.shape[0] != int(n_classes) or w.size != 6 * int(n_classes):
        raise ValueError(f"warps must be one 2x3 warp or [n_classes, 2, 3], got {w.shape}")
    return np.ascontiguousarray(w.reshape(int(n_classes), 6))


def _state_arrays(ids, a, b, na, nb):
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    n = ids.size
    a = None if a is None else np.ascontiguousarray(a, np.float64).reshape(n, na)
    b = None if b is None else np.ascontiguousarray(b, np.float64).reshape(n, nb)
    return n, ids, a, b


def _p(a):
    return None if a is None else a.ctypes.data

def _asso_kind(name: str) -> int:
    from .iou import KINDS

    if name not in KINDS:
        raise ValueError(f"Invalid association mode: {name}. Choose from {list(KINDS)}")
    return KINDS[name]


def _asso_name(kind: int) -> str:
    from .iou import KINDS

    return {v: k for k, v in KINDS.items()}[kind]


@dataclass
class OcsortParams:
    """OcSort constructor parameters (ocsort.py:197-235 names; YAML defaults)."""

    min_conf: float = 0.1
    det_thresh: float = 0.6
    max_age: int = 30
    min_hits: int = 3
    asso_threshold: float = 0.3
    delta_t: int = 3
    inertia: float = 0.1
    use_byte: bool = False
    Q_xy_scaling: float = 0.01
    Q_s_scaling: float = 0.0001
    asso_func: str = "iou"      # utils/iou.py registry mode (BaseTracker asso_func)
    frame_w: float = 1920.0     # centroid normalisation until set_frame_size latches the image
    frame_h: float = 1080.0


class OcsortEngine(_OcsFamilyEngine):
    """Handle over ``bx_ocsort_*`` (include/bxocsort.h): ``n_seq`` OCSort sequences in HBM, one
    kernel launch (one wave per sequence) per frame."""

    _PREFIX = "bx_ocsort"

    def __init__(self, n_seq: int = 1, track_cap: int = 256, det_cap: int = 256,
                 params: OcsortParams | None = None):
        p = params or OcsortParams()
        self.n_seq, self.track_cap, self.det_cap, self.params = n_seq, track_cap, det_cap, p
        cfg = N.BxOcsortConfig(
            n_seq=n_seq, track_cap=track_cap, det_cap=det_cap, min_conf=p.min_conf,
            det_thresh=p.det_thresh, asso_threshold=p.asso_threshold, inertia=p.inertia,
            q_xy_scaling=p.Q_xy_scaling, q_s_scaling=p.Q_s_scaling, max_age=int(p.max_age),
            min_hits=int(p.min_hits), delta_t=int(p.delta_t), use_byte=int(bool(p.use_byte)),
            asso_kind=_asso_kind(p.asso_func), frame_w=float(p.frame_w), frame_h=float(p.frame_h))
        self._create(cfg)

    # ---- one entry of the per-sequence parameter table (_SeqTable)
    _SEQ_STRUCT = N.BxOcsortSeqParams

    def _seq_struct(self, p: OcsortParams):
        return N.BxOcsortSeqParams(
            min_conf=p.min_conf, det_thresh=p.det_thresh, asso_threshold=p.asso_threshold,
            inertia=p.inertia, q_xy_scaling=p.Q_xy_scaling, q_s_scaling=p.Q_s_scaling,
            max_age=int(p.max_age), min_hits=int(p.min_hits), delta_t=int(p.delta_t),
            use_byte=int(bool(p.use_byte)), asso_kind=_asso_kind(p.asso_func))

    def _seq_params_of(self, o) -> OcsortParams:
        return OcsortParams(min_conf=o.min_conf, det_thresh=o.det_thresh, max_age=o.max_age,
                            min_hits=o.min_hits, asso_threshold=o.asso_threshold,
                            delta_t=o.delta_t, inertia=o.inertia, use_byte=bool(o.use_byte),
                            Q_xy_scaling=o.q_xy_scaling, Q_s_scaling=o.q_s_scaling,
                            asso_func=_asso_name(o.asso_kind), frame_w=self.params.frame_w,
                            frame_h=self.params.frame_h)

    def grown(self, track_cap: int, det_cap: int) -> "OcsortEngine":
        """A new engine with larger capacities holding this one's state (bx_ocsort_copy_state)."""
        e = OcsortEngine(self.n_seq, track_cap, det_cap, self.params)
        N.check(self._L.bx_ocsort_copy_state(e._h, self._h), "bx_ocsort_copy_state")
        return e

    def step(self, dets, det_off, out, out_count, seq0: int = 0, nseq: int | None = None,
             stream=None):
        """One frame for sequences [seq0, seq0+nseq) from device tensors (see bx_ocsort_step)."""
        nseq, stream = self._range(seq0, nseq, stream)
        N.check(self._L.bx_ocsort_step(self._h, seq0, nseq, _ptr(dets), _ptr(det_off), _ptr(out),
                                       _ptr(out_count), stream), "bx_ocsort_step")

    def update_host(self, seq: int, dets: np.ndarray) -> np.ndarray:
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        out = np.empty((max(n, 1), 8), np.float64)
        m = C.c_int(0)
        N.check(self._L.bx_ocsort_update_host(self._h, seq, d.ctypes.data if n else None, n,
                                              out.ctypes.data, C.byref(m), None),
                "bx_ocsort_update_host")
        return out[: m.value].copy()

    def update_classes_host(self, seq0: int, n_classes: int, dets: np.ndarray, id_count: int):
        """per_class=True frame (bx_ocsort_update_classes_host): class c is sequence seq0 + c, one
        launch; returns (rows with class-global ids, the advanced class-global id counter)."""
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        out = np.empty((max(n, 1), 8), np.float64)
        m, g = C.c_int(0), C.c_int(int(id_count))
        N.check(self._L.bx_ocsort_update_classes_host(
            self._h, seq0, int(n_classes), d.ctypes.data if n else None, n, C.byref(g),
            out.ctypes.data, C.byref(m), None), "bx_ocsort_update_classes_host")
        return out[: m.value].copy(), g.value

    def tracks(self, seq: int = 0) -> dict:
        """Host snapshot of the track list (list order): ids, XYSR means x [7], covariances."""
        cap = self.track_cap
        ids = np.zeros(cap, np.int32)
        x = np.zeros((cap, 7))
        P = np.zeros((cap, 7, 7))
        n = C.c_int()
        N.check(self._L.bx_ocsort_tracks_host(self._h, seq, cap, ids.ctypes.data, x.ctypes.data,
                                              P.ctypes.data, C.byref(n)), "tracks")
        k = min(n.value, cap)
        return {"id": ids[:k], "x": x[:k], "P": P[:k]}

    def state_set(self, seq: int, ids, x=None, P=None) -> None:
        """Write KalmanBoxTracker.kf.x [n,7] / .kf.P [n,7,7] of live tracks by id."""
        n, ids, a, b = _state_arrays(ids, x, P, 7, 49)
        N.check(self._L.bx_ocsort_state_set_host(self._h, seq, n, ids.ctypes.data, _p(a), _p(b)),
                "state_set")

    def probe(self, on: bool = True) -> None:
        N.check(self._L.bx_ocsort_probe(self._h, int(bool(on))), "bx_ocsort_probe")


class OcsortTableEngine(_SeqTable, OcsortEngine):
    """An ``OcsortEngine`` with per-sequence ``OcsortParams`` (``_SeqTable``; include/bxocsort.h,
    boxmot_amd.tune.sweep).  frame_w / frame_h, which are not part of the table, stay the
    engine's."""

    def grown(self, track_cap: int, det_cap: int) -> "OcsortTableEngine":
        """As OcsortEngine.grown, with the table."""
        e = OcsortTableEngine(self.n_seq, track_cap, det_cap, self.params)
        N.check(self._L.bx_ocsort_copy_state(e._h, self._h), "bx_ocsort_copy_state")
        return self._retable(e)


@dataclass
class DeepOcsortParams:
    """DeepOcSort constructor parameters (deepocsort.py:265-287 names and defaults)."""

    det_thresh: float = 0.3
    max_age: int = 30
    min_hits: int = 3
    iou_threshold: float = 0.3
    delta_t: int = 3
    asso_func: str = "iou"
    inertia: float = 0.2
    w_association_emb: float = 0.5
    alpha_fixed_emb: float = 0.95
    aw_param: float = 0.5
    embedding_off: bool = False
    aw_off: bool = False
    Q_xy_scaling: float = 0.01
    Q_s_scaling: float = 0.0001
    frame_w: float = 1920.0     # centroid normalisation until set_frame_size latches the image
    frame_h: float = 1080.0


class DeepOcsortEngine(_OcsFamilyEngine):
    """Handle over ``bx_deepoc_*`` (include/bxdeepocsort.h): ``n_seq`` DeepOCSort sequences in
    HBM; per frame the appearance contraction (fp64 MFMA), the frame kernel (one wave per
    sequence) and the embedding update.  Embeddings are float64, ``emb_dim`` wide (any positive
    width; unused with ``embedding_off``)."""

    _PREFIX = "bx_deepoc"

    STAGES = ["embcost", "frame", "feature"]

    def __init__(self, n_seq: int = 1, track_cap: int = 256, det_cap: int = 256,
                 emb_dim: int = 512, params: DeepOcsortParams | None = None):
        p = params or DeepOcsortParams()
        self.n_seq, self.track_cap, self.det_cap, self.params = n_seq, track_cap, det_cap, p
        self.emb_dim = 0 if p.embedding_off else int(emb_dim)
        cfg = N.BxDeepocConfig(
            n_seq=n_seq, track_cap=track_cap, det_cap=det_cap, emb_dim=self.emb_dim,
            det_thresh=float(p.det_thresh), iou_threshold=float(p.iou_threshold),
            inertia=float(p.inertia), q_xy_scaling=float(p.Q_xy_scaling),
            q_s_scaling=float(p.Q_s_scaling), w_association_emb=float(p.w_association_emb),
            alpha_fixed_emb=float(p.alpha_fixed_emb), aw_param=float(p.aw_param),
            max_age=int(p.max_age), min_hits=int(p.min_hits), delta_t=int(p.delta_t),
            embedding_off=int(bool(p.embedding_off)), aw_off=int(bool(p.aw_off)),
            asso_kind=_asso_kind(p.asso_func), frame_w=float(p.frame_w), frame_h=float(p.frame_h))
        self._create(cfg)

    # ---- one entry of the per-sequence parameter table (_SeqTable)
    _SEQ_STRUCT = N.BxDeepocSeqParams

    def _seq_struct(self, p: DeepOcsortParams):
        if bool(p.embedding_off) != bool(self.params.embedding_off):
            raise ValueError("embedding_off is engine-wide: a sequence cannot have its own")
        return N.BxDeepocSeqParams(
            det_thresh=float(p.det_thresh), iou_threshold=float(p.iou_threshold),
            inertia=float(p.inertia), q_xy_scaling=float(p.Q_xy_scaling),
            q_s_scaling=float(p.Q_s_scaling), w_association_emb=float(p.w_association_emb),
            alpha_fixed_emb=float(p.alpha_fixed_emb), aw_param=float(p.aw_param),
            max_age=int(p.max_age), min_hits=int(p.min_hits), delta_t=int(p.delta_t),
            aw_off=int(bool(p.aw_off)), asso_kind=_asso_kind(p.asso_func))

    def _seq_params_of(self, o) -> DeepOcsortParams:
        return DeepOcsortParams(
            det_thresh=o.det_thresh, max_age=o.max_age, min_hits=o.min_hits,
            iou_threshold=o.iou_threshold, delta_t=o.delta_t, asso_func=_asso_name(o.asso_kind),
            inertia=o.inertia,
            w_association_emb=o.w_association_emb, alpha_fixed_emb=o.alpha_fixed_emb,
            aw_param=o.aw_param, embedding_off=self.params.embedding_off, aw_off=bool(o.aw_off),
            Q_xy_scaling=o.q_xy_scaling, Q_s_scaling=o.q_s_scaling,
            frame_w=self.params.frame_w, frame_h=self.params.frame_h)

    def grown(self, track_cap: int, det_cap: int, map_cap: int | None = None) -> "DeepOcsortEngine":
        """A new engine with larger capacities holding this one's state (bx_deepoc_copy_state);
        map_cap: a larger per-class id map (per_class=True engines)."""
        e = DeepOcsortEngine(self.n_seq, track_cap, det_cap, self.emb_dim or 1, self.params)
        if map_cap is not None:
            e.classes_config(self.classes().n_classes, map_cap)
        N.check(self._L.bx_deepoc_copy_state(e._h, self._h), "bx_deepoc_copy_state")
        return e

    def step(self, dets, det_off, embs, warps, out, out_count, seq0: int = 0,
             nseq: int | None = None, stream=None):
        """One frame for sequences [seq0, seq0+nseq) from device tensors (see bx_deepoc_step):
        embs float64 [sum N, emb_dim] (None with embedding_off), warps [nseq, 6] or None."""
        nseq, stream = self._range(seq0, nseq, stream)
        N.check(self._L.bx_deepoc_step(self._h, seq0, nseq, _ptr(dets), _ptr(det_off), _ptr(embs),
                                       _ptr(warps), _ptr(out), _ptr(out_count), stream),
                "bx_deepoc_step")

    def update_host(self, seq: int, dets: np.ndarray, embs: np.ndarray | None = None,
                    warp: np.ndarray | None = None) -> np.ndarray:
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        e = None
        if self.emb_dim and n:
            if embs is None:
                raise ValueError("DeepOCSort needs embeddings unless embedding_off")
            e = np.ascontiguousarray(embs, dtype=np.float64).reshape(n, -1)
            if e.shape[1] != self.emb_dim:
                raise ValueError(f"embedding dim {e.shape[1]} != engine emb_dim {self.emb_dim}")
        w = None if warp is None else np.ascontiguousarray(warp, np.float64).reshape(6)
        out = np.empty((max(n, 1), 8), np.float64)
        m = C.c_int(0)
        N.check(self._L.bx_deepoc_update_host(
            self._h, seq, d.ctypes.data if n else None, n, _p(e), _p(w), out.ctypes.data,
            C.byref(m), None), "bx_deepoc_update_host")
        return out[: m.value].copy()

    def step_classes(self, dets, det_off, embs, warps, out, out_count, n_classes: int,
                     seq0: int = 0, nseq: int | None = None, stream=None):
        """One per_class=True frame for sequences [seq0, seq0+nseq) of ``n_classes`` classes, on
        an engine built with ``n_seq = S * n_classes`` (see bx_deepoc_step_classes): ``step``'s
        arguments per sequence, warps [nseq * n_classes, 6] or None; class split, the three
        launches over the class sequences and the id merge run on one stream."""
        nseq = self.n_seq // int(n_classes) - seq0 if nseq is None else nseq
        if stream is None:
            stream = _current_stream()
        N.check(self._L.bx_deepoc_step_classes(
            self._h, seq0, nseq, int(n_classes), _ptr(dets), _ptr(det_off), _ptr(embs),
            _ptr(warps), _ptr(out), _ptr(out_count), stream), "bx_deepoc_step_classes")

    def classes_config(self, n_classes: int, map_cap: int) -> None:
        """Build the class state ahead of the first per-class call with an id map of ``map_cap``
        births per class sequence."""
        N.check(self._L.bx_deepoc_classes_config(self._h, int(n_classes), int(map_cap)),
                "bx_deepoc_classes_config")

    def classes(self):
        """The engine's class state as a ClassSplit view (None before the first per-class call)."""
        h = C.c_void_p()
        N.check(self._L.bx_deepoc_classes(self._h, C.byref(h)), "bx_deepoc_classes")
        return ClassSplit._view(h, self) if h.value else None

    def update_classes_host(self, seq: int, n_classes: int, dets: np.ndarray,
                            embs: np.ndarray | None, id_count: int,
                            warps: np.ndarray | None = None):
        """per_class=True frame of sequence ``seq`` from host arrays
        (bx_deepoc_update_classes_host): returns (rows in class order with class-global ids, the
        advanced class-level id counter).  warps: [n_classes, 2, 3] or None."""
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        e = None
        if self.emb_dim and n:
            if embs is None:
                raise ValueError("DeepOCSort needs embeddings unless embedding_off")
            e = np.ascontiguousarray(embs, dtype=np.float64).reshape(n, -1)
            if e.shape[1] != self.emb_dim:
                raise ValueError(f"embedding dim {e.shape[1]} != engine emb_dim {self.emb_dim}")
        w = None if warps is None else np.ascontiguousarray(warps, np.float64).reshape(
            int(n_classes) * 6)
        out = np.empty((max(n, 1), 8), np.float64)
        m, g = C.c_int(0), C.c_int(int(id_count))
        N.check(self._L.bx_deepoc_update_classes_host(
            self._h, seq, int(n_classes), d.ctypes.data if n else None, n, _p(e), _p(w),
            C.byref(g), out.ctypes.data, C.byref(m), None), "bx_deepoc_update_classes_host")
        return out[: m.value].copy(), g.value

    def tracks(self, seq: int = 0) -> dict:
        """Host snapshot of the track list (list order): ids, XYSR means x [7], covariances
        [7, 7] and, unless embedding_off, embeddings [emb_dim]."""
        cap = self.track_cap
        ids = np.zeros(cap, np.int32)
        x = np.zeros((cap, 7))
        P = np.zeros((cap, 7, 7))
        E = np.zeros((cap, max(self.emb_dim, 1)))
        n = C.c_int()
        N.check(self._L.bx_deepoc_tracks_host(self._h, seq, cap, ids.ctypes.data, x.ctypes.data,
                                              P.ctypes.data, E.ctypes.data if self.emb_dim else None,
                                              C.byref(n)), "tracks")
        k = min(n.value, cap)
        snap = {"id": ids[:k], "x": x[:k], "P": P[:k]}
        if self.emb_dim:
            snap["emb"] = E[:k]
        return snap

    def state_set(self, seq: int, ids, x=None, P=None, emb=None) -> None:
        """Write kf.x [n,7] / kf.P [n,7,7] / emb [n,emb_dim] of live tracks by id."""
        n, ids, a, b = _state_arrays(ids, x, P, 7, 49)
        e = None
        if emb is not None and self.emb_dim:
            e = np.ascontiguousarray(emb, np.float64).reshape(n, self.emb_dim)
        N.check(self._L.bx_deepoc_state_set_host(self._h, seq, n, ids.ctypes.data, _p(a), _p(b),
                                                 _p(e)), "state_set")


class DeepOcsortTableEngine(_SeqTable, DeepOcsortEngine):
    """A ``DeepOcsortEngine`` with per-sequence ``DeepOcsortParams`` (``_SeqTable``;
    include/bxdeepocsort.h, boxmot_amd.tune.sweep_reid).  ``embedding_off`` stays the engine's (it
    decides the embedding width and two of the three launches: an entry's must be the engine's,
    ``ValueError``), and so do frame_w / frame_h, which are not part of the table."""

    def grown(self, track_cap: int, det_cap: int,
              map_cap: int | None = None) -> "DeepOcsortTableEngine":
        """As DeepOcsortEngine.grown, with the table."""
        e = DeepOcsortTableEngine(self.n_seq, track_cap, det_cap, self.emb_dim or 1, self.params)
        if map_cap is not None:
            e.classes_config(self.classes().n_classes, map_cap)
        N.check(self._L.bx_deepoc_copy_state(e._h, self._h), "bx_deepoc_copy_state")
        return self._retable(e)


def deepoc_embcost(dets_embs, trk_embs, out, stream=None) -> None:
    """out [nd, nt] = dets_embs [nd, F] @ trk_embs [nt, F].T on device float64 tensors, by the
    tracker's own MFMA tile (bx_deepoc_embcost)."""
    nd, F = dets_embs.shape
    nt = trk_embs.shape[0]
    if stream is None:
        stream = _current_stream()
    N.check(N.load().bx_deepoc_embcost(int(nd), int(nt), int(F), _ptr(dets_embs), _ptr(trk_embs),
                                       _ptr(out), stream), "bx_deepoc_embcost")


@dataclass
class HybridsortParams:
    """HybridSort constructor parameters (hybridsort.py:372-388 names and defaults; the
    reference gives det_thresh no default)."""

    det_thresh: float = 0.3
    max_age: int = 30
    min_hits: int = 3
    iou_threshold: float = 0.3
    delta_t: int = 3
    asso_func: str = "iou"
    inertia: float = 0.2
    longterm_reid_weight: float = 0.0
    TCM_first_step_weight: float = 0.0
    frame_w: float = 1920.0     # centroid normalisation until set_frame_size latches the image
    frame_h: float = 1080.0


class HybridsortEngine(_OcsFamilyEngine):
    """Handle over ``bx_hybrid_*`` (include/bxhybridsort.h): ``n_seq`` HybridSort sequences in
    HBM; per frame the two cosine-distance contractions (fp64 MFMA), the frame kernel (one wave
    per sequence) and the feature update.  Embeddings are float64, ``emb_dim`` wide."""

    _PREFIX = "bx_hybrid"

    STAGES = ["dist", "frame", "feature"]

    def __init__(self, n_seq: int = 1, track_cap: int = 256, det_cap: int = 256,
                 emb_dim: int = 512, params: HybridsortParams | None = None):
        p = params or HybridsortParams()
        self.n_seq, self.track_cap, self.det_cap, self.params = n_seq, track_cap, det_cap, p
        self.emb_dim = int(emb_dim)
        cfg = N.BxHybridConfig(
            n_seq=n_seq, track_cap=track_cap, det_cap=det_cap, emb_dim=self.emb_dim,
            det_thresh=float(p.det_thresh), iou_threshold=float(p.iou_threshold),
            inertia=float(p.inertia), longterm_reid_weight=float(p.longterm_reid_weight),
            tcm_first_step_weight=float(p.TCM_first_step_weight), max_age=int(p.max_age),
            min_hits=int(p.min_hits), delta_t=int(p.delta_t), asso_kind=_asso_kind(p.asso_func),
            frame_w=float(p.frame_w), frame_h=float(p.frame_h))
        self._create(cfg)

    # ---- one entry of the per-sequence parameter table (_SeqTable)
    _SEQ_STRUCT = N.BxHybridSeqParams

    def _seq_struct(self, p: HybridsortParams):
        return N.BxHybridSeqParams(
            det_thresh=float(p.det_thresh), iou_threshold=float(p.iou_threshold),
            inertia=float(p.inertia), longterm_reid_weight=float(p.longterm_reid_weight),
            tcm_first_step_weight=float(p.TCM_first_step_weight), max_age=int(p.max_age),
            min_hits=int(p.min_hits), delta_t=int(p.delta_t), asso_kind=_asso_kind(p.asso_func))

    def _seq_params_of(self, o) -> HybridsortParams:
        return HybridsortParams(
            det_thresh=o.det_thresh, max_age=o.max_age, min_hits=o.min_hits,
            iou_threshold=o.iou_threshold, delta_t=o.delta_t, asso_func=_asso_name(o.asso_kind),
            inertia=o.inertia,
            longterm_reid_weight=o.longterm_reid_weight,
            TCM_first_step_weight=o.tcm_first_step_weight, frame_w=self.params.frame_w,
            frame_h=self.params.frame_h)

    def grown(self, track_cap: int, det_cap: int, map_cap: int | None = None) -> "HybridsortEngine":
        """A new engine with larger capacities holding this one's state (bx_hybrid_copy_state);
        map_cap: a larger per-class id map (per_class=True engines)."""
        e = HybridsortEngine(self.n_seq, track_cap, det_cap, self.emb_dim, self.params)
        if map_cap is not None:
            e.classes_config(self.classes().n_classes, map_cap)
        N.check(self._L.bx_hybrid_copy_state(e._h, self._h), "bx_hybrid_copy_state")
        return e

    def step(self, dets, det_off, embs, out, out_count, seq0: int = 0, nseq: int | None = None,
             stream=None):
        """One frame for sequences [seq0, seq0+nseq) from device tensors (see bx_hybrid_step):
        embs float64 [sum N, emb_dim]."""
        nseq, stream = self._range(seq0, nseq, stream)
        N.check(self._L.bx_hybrid_step(self._h, seq0, nseq, _ptr(dets), _ptr(det_off), _ptr(embs),
                                       _ptr(out), _ptr(out_count), stream), "bx_hybrid_step")

    def update_host(self, seq: int, dets: np.ndarray, embs: np.ndarray | None = None) -> np.ndarray:
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        e = None
        if n:
            if embs is None:
                raise ValueError("HybridSort needs embeddings")
            e = np.ascontiguousarray(embs, dtype=np.float64).reshape(n, -1)
            if e.shape[1] != self.emb_dim:
                raise ValueError(f"embedding dim {e.shape[1]} != engine emb_dim {self.emb_dim}")
        out = np.empty((max(n, 1), 8), np.float64)
        m = C.c_int(0)
        N.check(self._L.bx_hybrid_update_host(
            self._h, seq, d.ctypes.data if n else None, n, _p(e), out.ctypes.data, C.byref(m),
            None), "bx_hybrid_update_host")
        return out[: m.value].copy()

    def step_classes(self, dets, det_off, embs, out, out_count, n_classes: int, seq0: int = 0,
                     nseq: int | None = None, stream=None):
        """One per_class=True frame for sequences [seq0, seq0+nseq) of ``n_classes`` classes, on
        an engine built with ``n_seq = S * n_classes`` (see bx_hybrid_step_classes): ``step``'s
        arguments per sequence; class split, the three launches over the class sequences and the
        id merge run on one stream."""
        nseq = self.n_seq // int(n_classes) - seq0 if nseq is None else nseq
        if stream is None:
            stream = _current_stream()
        N.check(self._L.bx_hybrid_step_classes(
            self._h, seq0, nseq, int(n_classes), _ptr(dets), _ptr(det_off), _ptr(embs), _ptr(out),
            _ptr(out_count), stream), "bx_hybrid_step_classes")

    def classes_config(self, n_classes: int, map_cap: int) -> None:
        """Build the class state ahead of the first per-class call with an id map of ``map_cap``
        births per class sequence."""
        N.check(self._L.bx_hybrid_classes_config(self._h, int(n_classes), int(map_cap)),
                "bx_hybrid_classes_config")

    def classes(self):
        """The engine's class state as a ClassSplit view (None before the first per-class call)."""
        h = C.c_void_p()
        N.check(self._L.bx_hybrid_classes(self._h, C.byref(h)), "bx_hybrid_classes")
        return ClassSplit._view(h, self) if h.value else None

    def update_classes_host(self, seq: int, n_classes: int, dets: np.ndarray,
                            embs: np.ndarray | None, id_count: int):
        """per_class=True frame of sequence ``seq`` from host arrays
        (bx_hybrid_update_classes_host): returns (rows in class order with class-global ids, the
        advanced class-level id counter)."""
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        e = None
        if n:
            if embs is None:
                raise ValueError("HybridSort needs embeddings")
            e = np.ascontiguousarray(embs, dtype=np.float64).reshape(n, -1)
            if e.shape[1] != self.emb_dim:
                raise ValueError(f"embedding dim {e.shape[1]} != engine emb_dim {self.emb_dim}")
        out = np.empty((max(n, 1), 8), np.float64)
        m, g = C.c_int(0), C.c_int(int(id_count))
        N.check(self._L.bx_hybrid_update_classes_host(
            self._h, seq, int(n_classes), d.ctypes.data if n else None, n, _p(e), C.byref(g),
            out.ctypes.data, C.byref(m), None), "bx_hybrid_update_classes_host")
        return out[: m.value].copy(), g.value

    def tracks(self, seq: int = 0) -> dict:
        """Host snapshot of the track list (list order): ids, the 9-state means x [9]
        (u, v, s, score, r and the velocities of the first four), covariances [9, 9], smoothed
        features [emb_dim], feature-bank means [emb_dim], the four corner velocities [4, 2]
        (lt, rt, lb, rb as (y, x)) and the number of features pushed into each track's bank."""
        cap = self.track_cap
        ids = np.zeros(cap, np.int32)
        x = np.zeros((cap, 9))
        P = np.zeros((cap, 9, 9))
        E = np.zeros((cap, self.emb_dim))
        M = np.zeros((cap, self.emb_dim))
        V = np.zeros((cap, 4, 2))
        bc = np.zeros(cap, np.int32)
        n = C.c_int()
        N.check(self._L.bx_hybrid_tracks_host(self._h, seq, cap, ids.ctypes.data, x.ctypes.data,
                                              P.ctypes.data, E.ctypes.data, M.ctypes.data,
                                              V.ctypes.data, bc.ctypes.data, C.byref(n)), "tracks")
        k = min(n.value, cap)
        return {"id": ids[:k], "x": x[:k], "P": P[:k], "emb": E[:k], "bank_mean": M[:k],
                "vel": V[:k], "bank_count": bc[:k]}

    def state_set(self, seq: int, ids, x=None, P=None) -> None:
        """Write kf.x [n,9] / kf.P [n,9,9] of live tracks by id."""
        n, ids, a, b = _state_arrays(ids, x, P, 9, 81)
        N.check(self._L.bx_hybrid_state_set_host(self._h, seq, n, ids.ctypes.data, _p(a), _p(b)),
                "state_set")

    def frame_stats(self, seq0: int = 0, nseq: int | None = None) -> dict:
        """Live tracks over sequences [seq0, seq0+nseq) after the last frame."""
        nseq = self.n_seq - seq0 if nseq is None else nseq
        return {"tracks": sum(self.counters(q)["n_tracks"] for q in range(seq0, seq0 + nseq))}

    def state_save(self, seq: int = 0) -> np.ndarray:
        """One sequence's whole tracker state as an opaque byte array (bx_hybrid_state_save_host)."""
        nb = C.c_size_t()
        N.check(self._L.bx_hybrid_state_bytes(self._h, C.byref(nb)), "state_bytes")
        blob = np.empty(nb.value, np.uint8)
        N.check(self._L.bx_hybrid_state_save_host(self._h, seq, blob.ctypes.data, nb.value),
                "state_save")
        return blob

    def state_load(self, seq: int, blob: np.ndarray) -> None:
        """Write a state_save() blob of an engine with the same track_cap and emb_dim."""
        b = np.ascontiguousarray(blob, np.uint8)
        N.check(self._L.bx_hybrid_state_load_host(self._h, seq, b.ctypes.data, b.size),
                "state_load")


def hybrid_cosdist(dets_embs, trk_embs, out, stream=None) -> None:
    """out [nd, nt] = max(0, 1 - cos(dets_embs [nd, F], trk_embs [nt, F])) on device float64
    tensors, by the tracker's own MFMA tile (bx_hybrid_cosdist)."""
    nd, F = dets_embs.shape
    nt = trk_embs.shape[0]
    if stream is None:
        stream = _current_stream()
    N.check(N.load().bx_hybrid_cosdist(int(nd), int(nt), int(F), _ptr(dets_embs), _ptr(trk_embs),
                                       _ptr(out), stream), "bx_hybrid_cosdist")


def hybrid_bank_mean(bank, pushed, out, stream=None) -> None:
    """out [nt, F] = mean of the rows present in each feature ring bank [nt, 30, F] after
    pushed [nt] (int32) pushes, on device tensors (bx_hybrid_bank_mean)."""
    nt, _, F = bank.shape
    if stream is None:
        stream = _current_stream()
    N.check(N.load().bx_hybrid_bank_mean(int(nt), int(F), _ptr(bank), _ptr(pushed), _ptr(out),
                                         stream), "bx_hybrid_bank_mean")


@dataclass
class HybridsortCmcParams(HybridsortParams):
    """HybridsortParams and the reference's ``ECC`` attribute (hybridsort.py:417), which is no
    constructor argument there: the parameters of a HybridsortCmcEngine whose sequences start
    with their camera update switched on, and an entry of HybridsortCmcTableEngine's table."""

    ECC: bool = False


def _ecc_off(p):
    """``p`` with its ECC (if it has one) off: grown() copies the switches, it does not set them."""
    return dataclasses.replace(p, ECC=False) if getattr(p, "ECC", False) else p


class HybridsortCmcEngine(HybridsortEngine):
    """A ``HybridsortEngine`` with the reference's ``ECC`` switch per sequence and the
    camera-motion warps of ``KalmanBoxTracker.camera_update`` (hybridsort.py:237-249, 448-451;
    include/bxhybridsort.h): ``set_ecc`` / ``ecc``, and ``warps`` on ``step``,
    ``update_host`` and their per-class forms.  ``params.ECC`` (HybridsortCmcParams) switches
    every sequence on at construction.  An engine on which no sequence was ever switched on launches
    ``HybridsortEngine``'s kernels and nothing else.  (A class of its own because
    HybridsortEngine's method set is pinned by tests/test_engine_api_host.py.)"""

    def __init__(self, n_seq: int = 1, track_cap: int = 256, det_cap: int = 256,
                 emb_dim: int = 512, params: HybridsortParams | None = None):
        super().__init__(n_seq, track_cap, det_cap, emb_dim, params)
        if getattr(self.params, "ECC", False):
            self.set_ecc(0, True)

    def set_ecc(self, seq0: int, flags, nseq: int | None = None) -> None:
        """The ``ECC`` attribute of sequences [seq0, seq0 + nseq) (bx_hybrid_set_ecc_host):
        ``flags`` is one value per sequence, or a scalar for ``nseq`` sequences (default: all from
        seq0).  A sequence whose switch is on starts every frame with ``camera_update`` of its
        live tracks under its row of ``warps`` (the identity without one), whatever the warp.
        Off after ``reset``; ``grown()`` carries it.  Synchronous."""
        f = np.atleast_1d(np.asarray(flags))
        if nseq is None:
            nseq = f.size if np.ndim(flags) else self.n_seq - seq0
        on = np.ascontiguousarray(np.broadcast_to(f != 0, (nseq,)), np.int32)
        N.check(self._L.bx_hybrid_set_ecc_host(self._h, int(seq0), int(nseq), on.ctypes.data),
                "bx_hybrid_set_ecc_host")

    def ecc(self, seq: int = 0) -> dict:
        """Sequence ``seq``'s switch and the number of tracks its camera updates left as they
        were for a state score of exactly 0 (where the reference raises) since the last reset.
        Synchronises the device (the count is read back); ``ecc_on`` does not."""
        on, sk = C.c_int(), C.c_int()
        N.check(self._L.bx_hybrid_ecc_host(self._h, int(seq), C.byref(on), C.byref(sk)),
                "bx_hybrid_ecc_host")
        return {"on": bool(on.value), "score_zero_skips": sk.value}

    def ecc_on(self, seq: int = 0) -> bool:
        """Sequence ``seq``'s switch from the library's host mirror: no device work."""
        on = C.c_int()
        N.check(self._L.bx_hybrid_ecc_host(self._h, int(seq), C.byref(on), None),
                "bx_hybrid_ecc_host")
        return bool(on.value)

    def grown(self, track_cap: int, det_cap: int,
              map_cap: int | None = None) -> "HybridsortCmcEngine":
        """As HybridsortEngine.grown; bx_hybrid_copy_state carries the switches."""
        e = HybridsortCmcEngine(self.n_seq, track_cap, det_cap, self.emb_dim, _ecc_off(self.params))
        e.params = self.params
        if map_cap is not None:
            e.classes_config(self.classes().n_classes, map_cap)
        N.check(self._L.bx_hybrid_copy_state(e._h, self._h), "bx_hybrid_copy_state")
        return e

    def step(self, dets, det_off, embs, out, out_count, seq0: int = 0, nseq: int | None = None,
             stream=None, warps=None):
        """HybridsortEngine.step with warps: float64 [nseq, 6] device tensor, one row-major 2x3
        affine per sequence of the call, or None (the identity); read by the sequences whose
        switch is on (bx_hybrid_step_cmc).  ``ValueError`` for another shape."""
        nseq, stream = self._range(seq0, nseq, stream)
        if warps is not None and tuple(warps.shape) not in ((nseq, 6), (nseq, 2, 3)):
            raise ValueError(f"warps of shape {tuple(warps.shape)} for {nseq} sequences: one "
                             f"2x3 affine per sequence is [{nseq}, 6]")
        N.check(self._L.bx_hybrid_step_cmc(self._h, seq0, nseq, _ptr(dets), _ptr(det_off),
                                           _ptr(embs), _ptr(warps), _ptr(out), _ptr(out_count),
                                           stream), "bx_hybrid_step")

    def _host_frame(self, dets, embs):
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        e = None
        if n:
            if embs is None:
                raise ValueError("HybridSort needs embeddings")
            e = np.ascontiguousarray(embs, dtype=np.float64).reshape(n, -1)
            if e.shape[1] != self.emb_dim:
                raise ValueError(f"embedding dim {e.shape[1]} != engine emb_dim {self.emb_dim}")
        return d, n, e

    def update_host(self, seq: int, dets: np.ndarray, embs: np.ndarray | None = None,
                    warp: np.ndarray | None = None) -> np.ndarray:
        """HybridsortEngine.update_host with warp: a 2x3 (or [6]) host array, or None."""
        d, n, e = self._host_frame(dets, embs)
        w = None if warp is None else np.ascontiguousarray(warp, np.float64).reshape(6)
        out = np.empty((max(n, 1), 8), np.float64)
        m = C.c_int(0)
        N.check(self._L.bx_hybrid_update_host_cmc(
            self._h, seq, d.ctypes.data if n else None, n, _p(e), _p(w), out.ctypes.data,
            C.byref(m), None), "bx_hybrid_update_host")
        return out[: m.value].copy()

    def step_classes(self, dets, det_off, embs, out, out_count, n_classes: int, seq0: int = 0,
                     nseq: int | None = None, stream=None, warps=None):
        """HybridsortEngine.step_classes with warps [nseq * n_classes, 6] or None, one per class
        sequence.  ``ValueError`` for another shape."""
        nseq = self.n_seq // int(n_classes) - seq0 if nseq is None else nseq
        if stream is None:
            stream = _current_stream()
        rows = nseq * int(n_classes)
        if warps is not None and tuple(warps.shape) not in ((rows, 6), (rows, 2, 3)):
            raise ValueError(f"warps of shape {tuple(warps.shape)} for {nseq} sequences of "
                             f"{n_classes} classes: one 2x3 affine per class sequence is "
                             f"[{rows}, 6]")
        N.check(self._L.bx_hybrid_step_classes_cmc(
            self._h, seq0, nseq, int(n_classes), _ptr(dets), _ptr(det_off), _ptr(embs),
            _ptr(warps), _ptr(out), _ptr(out_count), stream), "bx_hybrid_step_classes")

    def update_classes_host(self, seq: int, n_classes: int, dets: np.ndarray,
                            embs: np.ndarray | None, id_count: int,
                            warps: np.ndarray | None = None):
        """HybridsortEngine.update_classes_host with warps: [n_classes, 2, 3] or None."""
        d, n, e = self._host_frame(dets, embs)
        w = None if warps is None else np.ascontiguousarray(warps, np.float64).reshape(
            int(n_classes) * 6)
        out = np.empty((max(n, 1), 8), np.float64)
        m, g = C.c_int(0), C.c_int(int(id_count))
        N.check(self._L.bx_hybrid_update_classes_host_cmc(
            self._h, seq, int(n_classes), d.ctypes.data if n else None, n, _p(e), _p(w),
            C.byref(g), out.ctypes.data, C.byref(m), None), "bx_hybrid_update_classes_host")
        return out[: m.value].copy(), g.value


class HybridsortTableEngine(_SeqTable, HybridsortEngine):
    """A ``HybridsortEngine`` with per-sequence ``HybridsortParams`` (``_SeqTable``;
    include/bxhybridsort.h, boxmot_amd.tune.sweep_reid).  frame_w / frame_h, which are not part of
    the table, stay the engine's."""

    def grown(self, track_cap: int, det_cap: int,
              map_cap: int | None = None) -> "HybridsortTableEngine":
        """As HybridsortEngine.grown, with the table."""
        e = HybridsortTableEngine(self.n_seq, track_cap, det_cap, self.emb_dim, self.params)
        if map_cap is not None:
            e.classes_config(self.classes().n_classes, map_cap)
        N.check(self._L.bx_hybrid_copy_state(e._h, self._h), "bx_hybrid_copy_state")
        return self._retable(e)


class HybridsortCmcTableEngine(_SeqTable, HybridsortCmcEngine):
    """A ``HybridsortCmcEngine`` with per-sequence ``HybridsortParams``: the engine of a
    ``tune.sweep_reid`` in which a config sets ``ECC``.  An entry's ``ECC`` is the sequence's
    camera-update switch: ``set_seq_params`` sets it with the entry and ``seq_params`` reads it
    back, so the configs of one sweep may mix it.  (Beside HybridsortTableEngine, whose method
    set is pinned by tests/test_sweep_reid_host.py.)"""

    def set_seq_params(self, seq0: int, params, nseq: int | None = None) -> None:
        super().set_seq_params(seq0, params, nseq)
        if params is None:
            self.set_ecc(seq0, False, self.n_seq - seq0 if nseq is None else nseq)
        elif len(params):
            self.set_ecc(seq0, [bool(getattr(p, "ECC", False)) for p in params])

    def seq_params(self, seq: int):
        return HybridsortCmcParams(**dataclasses.asdict(super().seq_params(seq)),
                                   ECC=self.ecc_on(seq))

    def grown(self, track_cap: int, det_cap: int,
              map_cap: int | None = None) -> "HybridsortCmcTableEngine":
        """As HybridsortCmcEngine.grown, with the table."""
        e = HybridsortCmcTableEngine(self.n_seq, track_cap, det_cap, self.emb_dim,
                                     _ecc_off(self.params))
        e.params = self.params
        if map_cap is not None:
            e.classes_config(self.classes().n_classes, map_cap)
        N.check(self._L.bx_hybrid_copy_state(e._h, self._h), "bx_hybrid_copy_state")
        return self._retable(e)


class ClassSplit(_NativeHandle):
    """Handle over ``bx_classes_*`` (include/bxclasses.h): per_class=True on the device for
    ``n_seq`` sequences of ``n_classes`` classes — the stable class split of a frame's rows and the
    merge of the class sequences' output rows under class-global ids.  The engines'
    ``step_classes`` own one; built directly it drives the two kernels alone."""

    _PREFIX = "bx_classes"

    def __init__(self, n_seq: int, n_classes: int, emb_dim: int = 0, row_cap: int = 256,
                 map_cap: int = 4096, id0: int = 1):
        self._L = N.load()
        h = C.c_void_p()
        N.check(self._L.bx_classes_create(int(n_seq), int(n_classes), int(emb_dim), int(row_cap),
                                          int(map_cap), int(id0), C.byref(h)), "bx_classes_create")
        self._h, self._owner = h, None
        self.n_seq, self.n_classes, self.emb_dim = int(n_seq), int(n_classes), int(emb_dim)
        self.row_cap, self.map_cap, self.id0 = int(row_cap), int(map_cap), int(id0)

    @classmethod
    def _view(cls, handle, owner) -> "ClassSplit":
        v = cls.__new__(cls)
        v._L, v._h, v._owner = N.load(), handle, owner  # (the owner keeps the state alive)
        a = [C.c_int() for _ in range(6)]
        N.check(v._L.bx_classes_shape(handle, *[C.byref(x) for x in a]), "bx_classes_shape")
        v.n_seq, v.n_classes, v.emb_dim, v.row_cap, v.map_cap, v.id0 = [x.value for x in a]
        return v

    def close(self):
        h = getattr(self, "_h", None)
        if h and self._owner is None:
            self._L.bx_classes_destroy(h)
        self._h = None

    def split(self, dets, det_off, embs, o_dets, o_embs, o_off, o_src, nseq: int | None = None,
              stream=None) -> None:
        """Device tensors: dets [n, 6] float32, det_off [nseq + 1], embs [n, emb_dim] float64 or
        None -> class-major o_dets / o_embs, o_off [nseq * n_classes + 1], o_src [n]."""
        nseq = self.n_seq if nseq is None else nseq
        if stream is None:
            stream = _current_stream()
        N.check(self._L.bx_classes_split(self._h, int(nseq), _ptr(dets), _ptr(det_off), _ptr(embs),
                                         _ptr(o_dets), _ptr(o_embs), _ptr(o_off), _ptr(o_src),
                                         stream), "bx_classes_split")

    def merge(self, c_off, c_out, c_cnt, ids, det_off, out, out_count, seq0: int = 0,
              nseq: int | None = None, ids_stride: int = 1, stream=None) -> None:
        """Device tensors: the class sequences' det_off / out / out_count of one step and their
        next-id counters ``ids`` (absolute engine sequence q at ids[q * ids_stride]) -> the
        sequences' rows from out[det_off[k]] and out_count [nseq]."""
        nseq = self.n_seq - seq0 if nseq is None else nseq
        if stream is None:
            stream = _current_stream()
        N.check(self._L.bx_classes_merge(self._h, int(seq0), int(nseq), _ptr(c_off), _ptr(c_out),
                                         _ptr(c_cnt), _ptr(ids), int(ids_stride), _ptr(det_off),
                                         _ptr(out), _ptr(out_count), stream), "bx_classes_merge")

    def reset(self, seq0: int = 0, nseq: int | None = None, stream=None) -> None:
        nseq = self.n_seq - seq0 if nseq is None else nseq
        N.check(self._L.bx_classes_reset(self._h, seq0, nseq, stream), "bx_classes_reset")

    def id_count(self, seq: int = 0) -> int:
        g = C.c_int(0)
        N.check(self._L.bx_classes_id_count_host(self._h, seq, C.byref(g)), "id_count")
        return g.value

    def set_id_count(self, seq: int, value: int) -> None:
        N.check(self._L.bx_classes_set_id_count(self._h, seq, int(value), None), "set_id_count")

    def id_map(self, seq: int, cls: int) -> np.ndarray:
        """Class-global ids of the local ids id0, id0 + 1, ... class ``cls`` of ``seq`` gave out."""
        m = np.zeros(self.map_cap, np.int32)
        n = C.c_int(0)
        N.check(self._L.bx_classes_map_host(self._h, seq, cls, self.map_cap, m.ctypes.data,
                                            C.byref(n)), "bx_classes_map_host")
        return m[: n.value].copy()


class SequenceFeeder(_NativeHandle):
    """Handle over ``bx_feed_*`` (include/bxfeed.h): the packed rows of many sequences resident
    in HBM, gathered per frame index into the batched arrays a ``step`` takes, and the steps'
    output rows appended on the device as MOT rows; one copy back at the end.

    dets / embs: per sequence its packed rows ([rows, 6], [rows, emb_dim]); tables: per sequence
    ``(row_start, row_cnt, frame_id)``, one entry per frame index it iterates (``row_cnt`` 0: not
    stepped).  ``emb_dim`` 0 feeds no embeddings.  ``res_cap``: rows of each sequence's result
    buffer (default: its detection count); ``guard_rows``: extra rows behind the last buffer.
    ``schedule[t]`` lists the runs of frame index t as ``(seq0, nseq, rows, dets, det_off, embs,
    out, out_count)`` with the last five as device addresses."""

    _PREFIX = "bx_feed"
    det_f64, out_cols = False, 8  # the runs' types (SharedSequenceFeeder may choose others)

    def __init__(self, dets, embs, tables, emb_dim: int, res_cap=None, guard_rows: int = 0):
        self._build(dets, embs, tables, emb_dim, res_cap, guard_rows, None)

    def _build(self, dets, embs, tables, emb_dim, res_cap, guard_rows, source, fmt=None) -> None:
        """Create, upload and read the schedule.  ``source``: None, or SharedSequenceFeeder's
        map (only a source's rows are read and uploaded).  ``fmt``: None, or SharedSequenceFeeder's
        (det_f64, out_cols) for bx_feed_create_shared_fmt."""
        S = len(dets)
        self.n_seq, self.emb_dim = S, int(emb_dim)
        src = None if source is None else np.ascontiguousarray(source, np.int32).reshape(S)
        own = [src is None or int(src[k]) == k for k in range(S)]
        rows = np.array([int(np.shape(d)[0]) if own[k] else 0 for k, d in enumerate(dets)],
                        np.int64)
        tab_off = np.zeros(S + 1, np.int64)
        tab_off[1:] = np.cumsum([len(t[1]) for t in tables])

        def column(j, dt):
            return np.ascontiguousarray(np.concatenate(
                [np.asarray(t[j], dt).reshape(-1) for t in tables] + [np.empty(0, dt)]))

        start, cnt, fid = column(0, np.int64), column(1, np.int32), column(2, np.int32)
        cap = None if res_cap is None else np.ascontiguousarray(res_cap, np.int64).reshape(S)
        self._L = N.load()
        h = C.c_void_p()
        if src is None:
            N.check(self._L.bx_feed_create(S, self.emb_dim, rows.ctypes.data, tab_off.ctypes.data,
                                           start.ctypes.data, cnt.ctypes.data, fid.ctypes.data,
                                           _p(cap), int(guard_rows), C.byref(h)), "bx_feed_create")
        elif fmt is None:
            N.check(self._L.bx_feed_create_shared(
                S, self.emb_dim, rows.ctypes.data, tab_off.ctypes.data, start.ctypes.data,
                cnt.ctypes.data, fid.ctypes.data, _p(cap), int(guard_rows), src.ctypes.data,
                C.byref(h)), "bx_feed_create_shared")
        else:
            N.check(self._L.bx_feed_create_shared_fmt(
                S, self.emb_dim, rows.ctypes.data, tab_off.ctypes.data, start.ctypes.data,
                cnt.ctypes.data, fid.ctypes.data, _p(cap), int(guard_rows), src.ctypes.data,
                int(fmt[0]), int(fmt[1]), C.byref(h)), "bx_feed_create_shared_fmt")
            self.det_f64, self.out_cols = bool(fmt[0]), int(fmt[1])
        self._h = h
        for k in range(S):
            if not rows[k]:
                continue
            d = np.ascontiguousarray(dets[k], np.float32).reshape(-1, 6)
            e = None
            if self.emb_dim:
                e = np.ascontiguousarray(embs[k], np.float64)
                if e.shape != (rows[k], self.emb_dim):
                    raise ValueError(f"sequence {k}: embeddings {e.shape} != "
                                     f"({rows[k]}, {self.emb_dim})")
            N.check(self._L.bx_feed_upload_host(self._h, k, d.ctypes.data, _p(e)),
                    "bx_feed_upload_host")
        nf, mr = C.c_int(), C.c_int()
        N.check(self._L.bx_feed_shape(self._h, C.byref(nf), C.byref(mr)), "bx_feed_shape")
        self.n_frames, self.max_runs = nf.value, mr.value
        self.schedule = []
        i3 = [C.c_int() for _ in range(3)]
        p5 = [C.c_void_p() for _ in range(5)]
        for t in range(self.n_frames):
            nr = C.c_int()
            N.check(self._L.bx_feed_frame_runs(self._h, t, C.byref(nr)), "bx_feed_frame_runs")
            runs = []
            for r in range(nr.value):
                N.check(self._L.bx_feed_run(self._h, t, r, *[C.byref(x) for x in i3 + p5]),
                        "bx_feed_run")
                runs.append(tuple(x.value for x in i3 + p5))
            self.schedule.append(runs)

    def gather(self, t: int, stream=None) -> None:
        """Write every run's dets / embs / det_off of frame index t (one launch)."""
        if stream is None:
            stream = _current_stream()
        N.check(self._L.bx_feed_gather(self._h, int(t), stream), "bx_feed_gather")

    def append(self, t: int, stream=None) -> None:
        """Append the MOT rows of frame index t from its runs' out / out_count (one launch)."""
        if stream is None:
            stream = _current_stream()
        N.check(self._L.bx_feed_append(self._h, int(t), stream), "bx_feed_append")

    def raw_results(self):
        """The whole result allocation [rows, 9] (guard rows last), each sequence's first row
        [n_seq + 1] and the rows it appended [n_seq]: the one device-to-host copy."""
        n = C.c_int64()
        N.check(self._L.bx_feed_result_rows(self._h, C.byref(n)), "bx_feed_result_rows")
        res = np.empty((n.value, 9), np.float64)
        base = np.empty(self.n_seq + 1, np.int64)
        cnt = np.empty(self.n_seq, np.int64)
        N.check(self._L.bx_feed_results_host(self._h, res.ctypes.data if n.value else None,
                                             base.ctypes.data, cnt.ctypes.data),
                "bx_feed_results_host")
        return res, base, cnt

    def results(self) -> list:
        """Per sequence its MOT rows [n, 9]; raises when an append did not fit."""
        res, base, cnt = self.raw_results()
        if self.status() != 0:
            raise RuntimeError(f"feeder status {self.status()} (result buffer overflow)")
        return [res[base[k]: base[k] + cnt[k]] for k in range(self.n_seq)]

    @property
    def results_device(self):
        """The result buffers where they lie, as device pointers: (rows [result_rows, 9] float64,
        base [n_seq + 1] int64, n [n_seq] int64, result_rows).  No copy and no synchronisation;
        valid until ``close``.  ``MotEvaluator.run_device`` takes them as they are.  (A property:
        the class's methods are pinned by tests/test_engine_api_host.py, and this one only reads
        three pointers.)"""
        p = [C.c_void_p() for _ in range(3)]
        n = C.c_int64()
        N.check(self._L.bx_feed_results_device(self._h, *[C.byref(x) for x in p], C.byref(n)),
                "bx_feed_results_device")
        return p[0].value or 0, p[1].value or 0, p[2].value or 0, n.value

    def read_run(self, t: int, r: int):
        """Host copies of the gathered (dets, det_off, embs) of run r of frame index t."""
        _, nseq, rows = self.schedule[t][r][:3]
        d = np.empty((rows, 6), np.float64 if self.det_f64 else np.float32)
        o = np.empty(nseq + 1, np.int32)
        e = np.empty((rows, self.emb_dim), np.float64) if self.emb_dim else None
        N.check(self._L.bx_feed_read_run_host(self._h, int(t), int(r), d.ctypes.data,
                                              o.ctypes.data, _p(e)), "bx_feed_read_run_host")
        return d, o, e

    def write_run(self, t: int, r: int, out, out_count) -> None:
        """Set out [rows, 8] ([rows, out_cols]) / out_count [nseq] of run r of frame index t from
        host arrays."""
        _, nseq, rows = self.schedule[t][r][:3]
        o = np.ascontiguousarray(out, np.float64).reshape(rows, self.out_cols)
        c = np.ascontiguousarray(out_count, np.int32).reshape(nseq)
        N.check(self._L.bx_feed_write_run_host(self._h, int(t), int(r), o.ctypes.data,
                                               c.ctypes.data), "bx_feed_write_run_host")

    @property
    def device_bytes(self) -> int:
        """Bytes of device memory the feeder allocated (bx_feed_device_bytes).  (A property, as
        ``results_device``: it reads one number.)"""
        n = C.c_int64()
        N.check(self._L.bx_feed_device_bytes(self._h, C.byref(n)), "bx_feed_device_bytes")
        return n.value


class SharedSequenceFeeder(SequenceFeeder):
    """A ``SequenceFeeder`` whose sequences share packed rows (``bx_feed_create_shared``,
    include/bxfeed.h): sequence k gathers from the rows of sequence ``source[k]``
    (``source[k] <= k``, a source is its own source).  Only the sources' ``dets`` / ``embs`` are
    read and uploaded; the entries of the other sequences may be None.  Tables, runs, gathered
    arrays and results stay per sequence.  ``source=None`` is a plain SequenceFeeder.  (A class
    of its own because SequenceFeeder's constructor signature is pinned by
    tests/test_engine_api_host.py.)

    ``det_f64`` / ``out_cols`` (``bx_feed_create_shared_fmt``; they need a ``source``) choose the
    runs' types for an engine like StrongSort's: with ``det_f64`` the gathered ``dets`` are float64
    (the packed rows stay float32; the widening is exact), with ``out_cols=10`` the runs' ``out``
    rows have 10 columns, of which the append reads the first 8.  The defaults are
    ``bx_feed_create_shared`` as before."""

    def __init__(self, dets, embs, tables, emb_dim: int, res_cap=None, guard_rows: int = 0,
                 source=None, *, det_f64: bool = False, out_cols: int = 8):
        self.source = None if source is None else [int(q) for q in source]
        fmt = None
        if det_f64 or out_cols != 8:
            if source is None:
                raise ValueError("det_f64 / out_cols need a source map (bx_feed_create_shared_fmt)")
            fmt = (bool(det_f64), int(out_cols))
        self._build(dets, embs, tables, emb_dim, res_cap, guard_rows, source, fmt)


@dataclass
class BoostParams:
    """BoostTrack constructor parameters (boosttrack.py:154-181 names; YAML defaults)."""

    max_age: int = 60
    min_hits: int = 3
    det_thresh: float = 0.6
    iou_threshold: float = 0.3
    use_ecc: bool = True
    min_box_area: float = 10
    aspect_ratio_thresh: float = 1.6
    lambda_iou: float = 0.5
    lambda_mhd: float = 0.25
    lambda_shape: float = 0.25
    use_dlo_boost: bool = True
    use_duo_boost: bool = True
    dlo_boost_coef: float = 0.65
    s_sim_corr: bool = False
    use_rich_s: bool = True
    use_sb: bool = True
    use_vt: bool = True
    with_reid: bool = True


class BoostEngine(_TrackListEngine):
    """Handle over ``bx_boost_*`` (include/bxboost.h): ``n_seq`` BoostTrack sequences in HBM;
    per frame a ReID contraction (fp64 MFMA), the frame kernel (a 1-4 wave workgroup per
    sequence) and the embedding update."""

    _PREFIX = "bx_boost"

    def __init__(self, n_seq: int = 1, track_cap: int = 256, det_cap: int = 256,
                 emb_dim: int = 0, params: BoostParams | None = None):
        p = params or BoostParams()
        if p.with_reid and emb_dim <= 0:
            raise ValueError("with_reid BoostTrack needs emb_dim > 0")
        self.n_seq, self.track_cap, self.det_cap, self.params = n_seq, track_cap, det_cap, p
        self.emb_dim = emb_dim if p.with_reid else 0
        cfg = N.BxBoostConfig(
            n_seq=n_seq, track_cap=track_cap, det_cap=det_cap, emb_dim=self.emb_dim,
            max_age=int(p.max_age), min_hits=int(p.min_hits), det_thresh=float(p.det_thresh),
            iou_threshold=float(p.iou_threshold), min_box_area=float(p.min_box_area),
            aspect_ratio_thresh=float(p.aspect_ratio_thresh), lambda_iou=float(p.lambda_iou),
            lambda_mhd=float(p.lambda_mhd), lambda_shape=float(p.lambda_shape),
            dlo_boost_coef=float(p.dlo_boost_coef), use_ecc=int(bool(p.use_ecc)),
            use_dlo_boost=int(bool(p.use_dlo_boost)), use_duo_boost=int(bool(p.use_duo_boost)),
            s_sim_corr=int(bool(p.s_sim_corr)), use_rich_s=int(bool(p.use_rich_s)),
            use_sb=int(bool(p.use_sb)), use_vt=int(bool(p.use_vt)),
            with_reid=int(bool(p.with_reid)))
        self._create(cfg)

    # ---- one entry of the per-sequence parameter table (_SeqTable)
    _SEQ_STRUCT = N.BxBoostSeqParams

    def _seq_struct(self, p: BoostParams):
        if bool(p.with_reid) != bool(self.params.with_reid):
            raise ValueError("with_reid is engine-wide: a sequence cannot have its own")
        return N.BxBoostSeqParams(
            max_age=int(p.max_age), min_hits=int(p.min_hits), det_thresh=float(p.det_thresh),
            iou_threshold=float(p.iou_threshold), min_box_area=float(p.min_box_area),
            aspect_ratio_thresh=float(p.aspect_ratio_thresh), lambda_iou=float(p.lambda_iou),
            lambda_mhd=float(p.lambda_mhd), lambda_shape=float(p.lambda_shape),
            dlo_boost_coef=float(p.dlo_boost_coef), use_ecc=int(bool(p.use_ecc)),
            use_dlo_boost=int(bool(p.use_dlo_boost)), use_duo_boost=int(bool(p.use_duo_boost)),
            s_sim_corr=int(bool(p.s_sim_corr)), use_rich_s=int(bool(p.use_rich_s)),
            use_sb=int(bool(p.use_sb)), use_vt=int(bool(p.use_vt)))

    def _seq_params_of(self, o) -> BoostParams:
        return BoostParams(
            max_age=o.max_age, min_hits=o.min_hits, det_thresh=o.det_thresh,
            iou_threshold=o.iou_threshold, use_ecc=bool(o.use_ecc), min_box_area=o.min_box_area,
            aspect_ratio_thresh=o.aspect_ratio_thresh, lambda_iou=o.lambda_iou,
            lambda_mhd=o.lambda_mhd, lambda_shape=o.lambda_shape,
            use_dlo_boost=bool(o.use_dlo_boost), use_duo_boost=bool(o.use_duo_boost),
            dlo_boost_coef=o.dlo_boost_coef, s_sim_corr=bool(o.s_sim_corr),
            use_rich_s=bool(o.use_rich_s), use_sb=bool(o.use_sb), use_vt=bool(o.use_vt),
            with_reid=bool(self.params.with_reid))

    def grown(self, track_cap: int, det_cap: int) -> "BoostEngine":
        """A new engine with larger capacities holding this one's state (bx_boost_copy_state)."""
        e = BoostEngine(self.n_seq, track_cap, det_cap, self.emb_dim or 0, self.params)
        N.check(self._L.bx_boost_copy_state(e._h, self._h), "bx_boost_copy_state")
        return e

    def step(self, dets, det_off, embs, warps, out, out_count, seq0: int = 0,
             nseq: int | None = None, stream=None):
        """One frame for sequences [seq0, seq0+nseq) from device tensors (see bx_boost_step)."""
        nseq, stream = self._range(seq0, nseq, stream)
        N.check(self._L.bx_boost_step(self._h, seq0, nseq, _ptr(dets), _ptr(det_off), _ptr(embs),
                                      _ptr(warps), _ptr(out), _ptr(out_count), stream),
                "bx_boost_step")

    def update_host(self, seq: int, dets: np.ndarray, embs: np.ndarray | None = None,
                    warp: np.ndarray | None = None) -> np.ndarray:
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        e = None
        if self.emb_dim:
            if n and embs is None:
                raise ValueError("with_reid BoostTrack needs embeddings")
            if n:
                e = np.ascontiguousarray(embs, dtype=np.float64).reshape(n, -1)
                if e.shape[1] != self.emb_dim:
                    raise ValueError(f"embedding dim {e.shape[1]} != engine emb_dim {self.emb_dim}")
        w = None if warp is None else np.ascontiguousarray(warp, np.float64).reshape(6)
        out = np.empty((max(n, 1), 8), np.float64)
        m = C.c_int(0)
        N.check(self._L.bx_boost_update_host(
            self._h, seq, d.ctypes.data if n else None, n, None if e is None else e.ctypes.data,
            None if w is None else w.ctypes.data, out.ctypes.data, C.byref(m), None),
            "bx_boost_update_host")
        return out[: m.value].copy()

    def update_classes_host(self, seq: int, dets: np.ndarray, embs: np.ndarray | None = None,
                            warp: np.ndarray | None = None, n_classes: int = 80) -> np.ndarray:
        """per_class=True frame of one sequence (bx_boost_update_classes_host)."""
        d = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        n = d.shape[0]
        e = None
        if self.emb_dim and n:
            if embs is None:
                raise ValueError("with_reid BoostTrack needs embeddings")
            e = np.ascontiguousarray(embs, dtype=np.float64).reshape(n, -1)
            if e.shape[1] != self.emb_dim:
                raise ValueError(f"embedding dim {e.shape[1]} != engine emb_dim {self.emb_dim}")
        w = _class_warps(warp, n_classes)
        out = np.empty((max(n, 1), 8), np.float64)
        m = C.c_int(0)
        N.check(self._L.bx_boost_update_classes_host(
            self._h, seq, d.ctypes.data if n else None, n, None if e is None else e.ctypes.data,
            None if w is None else w.ctypes.data, int(n_classes), out.ctypes.data, C.byref(m),
            None), "bx_boost_update_classes_host")
        return out[: m.value].copy()

    def tracks(self, seq: int = 0) -> dict:
        """Host snapshot of the track list (list order): ids, means x [8], covariances [8, 8],
        embeddings [F] (with_reid)."""
        cap = self.track_cap
        ids = np.zeros(cap, np.int32)
        x = np.zeros((cap, 8))
        P = np.zeros((cap, 8, 8))
        E = np.zeros((cap, max(self.emb_dim, 1)))
        n = C.c_int()
        N.check(self._L.bx_boost_tracks_host(self._h, seq, cap, ids.ctypes.data, x.ctypes.data,
                                             P.ctypes.data, E.ctypes.data if self.emb_dim else None,
                                             C.byref(n)), "tracks")
        k = min(n.value, cap)
        snap = {"id": ids[:k], "x": x[:k], "P": P[:k]}
        if self.emb_dim:
            snap["emb"] = E[:k]
        return snap

    def state_set(self, seq: int, ids, x=None, P=None) -> None:
        """Write KalmanBoxTracker.kf.x [n,8] / .kf.covariance [n,8,8] of live tracks by id."""
        n, ids, a, b = _state_arrays(ids, x, P, 8, 64)
        N.check(self._L.bx_boost_state_set_host(self._h, seq, n, ids.ctypes.data, _p(a), _p(b)),
                "state_set")

    def frame_stats(self, seq0: int = 0, nseq: int | None = None) -> dict:
        nseq = self.n_seq - seq0 if nseq is None else nseq
        a = (C.c_int64 * 7)()
        N.check(self._L.bx_boost_frame_stats_host(self._h, seq0, nseq, a), "frame_stats")
        return dict(zip(["dets", "kept", "tracks", "outputs", "records", "frame", "pairs"],
                        [int(x) for x in a]))

    STAGES = ["embcost", "frame", "feature"]


class BoostTableEngine(_SeqTable, BoostEngine):
    """A ``BoostEngine`` with per-sequence ``BoostParams`` (``_SeqTable``; include/bxboost.h,
    boxmot_amd.tune.sweep_boost), also for cameras with thresholds and track lifetimes of their
    own.  ``with_reid`` (an entry's must be the engine's, ``ValueError``), the capacities and the
    embedding width stay the engine's.  (A class of its own because BoostEngine's method set is
    pinned by tests/test_engine_api_host.py.)"""

    def grown(self, track_cap: int, det_cap: int) -> "BoostTableEngine":
        """As BoostEngine.grown, with the table."""
        e = BoostTableEngine(self.n_seq, track_cap, det_cap, self.emb_dim or 0, self.params)
        N.check(self._L.bx_boost_copy_state(e._h, self._h), "bx_boost_copy_state")
        return self._retable(e)


@dataclass
class SsParams:
    """StrongSort constructor parameters (strongsort.py:45-66 names and defaults)."""

    min_conf: float = 0.1
    max_cos_dist: float = 0.15
    max_iou_dist: float = 0.7
    max_age: int = 50
    n_init: int = 2
    nn_budget: int = 150
    mc_lambda: float = 0.995
    ema_alpha: float = 0.9
    conf_thresh_high: float = 0.7
    conf_thresh_low: float = 0.3
    id_preservation_weight: float = 0.1
    crowd_detection: bool = True
    born_confirmed: bool = False


class SsEngine(_NativeEngine):
    """Handle over ``bx_ss_*`` (include/bxstrongsort.h): ``n_seq`` StrongSort sequences in HBM;
    per frame the detection-feature kernel, the NN-gallery distance (fp64 MFMA), the recovery
    similarities and the frame kernel (one wave per sequence)."""

    _PREFIX = "bx_ss"

    STAGES = ["prep", "nn", "recovery", "pre", "cost", "match", "update", "post", "fit"]

    def __init__(self, n_seq: int = 1, track_cap: int = 256, det_cap: int = 256,
                 emb_dim: int = 512, vec_cap: int = 32, params: SsParams | None = None):
        p = params or SsParams()
        self.n_seq, self.track_cap, self.det_cap, self.params = n_seq, track_cap, det_cap, p
        self.emb_dim = emb_dim
        cfg = N.BxSsConfig(
            n_seq=n_seq, track_cap=track_cap, det_cap=det_cap, emb_dim=emb_dim, vec_cap=vec_cap,
            min_conf=float(p.min_conf), max_cos_dist=float(p.max_cos_dist),
            max_iou_dist=float(p.max_iou_dist), max_age=int(p.max_age), n_init=int(p.n_init),
            nn_budget=int(p.nn_budget), mc_lambda=float(p.mc_lambda),
            ema_alpha=float(p.ema_alpha), conf_thresh_high=float(p.conf_thresh_high),
            conf_thresh_low=float(p.conf_thresh_low),
            id_preservation_weight=float(p.id_preservation_weight),
            crowd_detection=int(bool(p.crowd_detection)),
            born_confirmed=int(bool(p.born_confirmed)))
        self._create(cfg)
        self.vec_cap = vec_cap

    def slots_used(self, seq: int = 0) -> int:
        """Listed tracks plus the lost buffer's (their galleries keep their slots)."""
        c = self.counters(seq)
        return c["n_tracks"] + c["n_lost"]

    # ---- one entry of the per-sequence parameter table (_SeqTable)
    _SEQ_STRUCT = N.BxSsSeqParams

    @staticmethod
    def _seq_struct(p: SsParams):
        return N.BxSsSeqParams(
            min_conf=float(p.min_conf), max_cos_dist=float(p.max_cos_dist),
            max_iou_dist=float(p.max_iou_dist), max_age=int(p.max_age), n_init=int(p.n_init),
            nn_budget=int(p.nn_budget), mc_lambda=float(p.mc_lambda),
            ema_alpha=float(p.ema_alpha), conf_thresh_high=float(p.conf_thresh_high),
            conf_thresh_low=float(p.conf_thresh_low),
            id_preservation_weight=float(p.id_preservation_weight),
            crowd_detection=int(bool(p.crowd_detection)),
            born_confirmed=int(bool(p.born_confirmed)))

    @staticmethod
    def _seq_params_of(o) -> SsParams:
        return SsParams(
            min_conf=o.min_conf, max_cos_dist=o.max_cos_dist, max_iou_dist=o.max_iou_dist,
            max_age=o.max_age, n_init=o.n_init, nn_budget=o.nn_budget, mc_lambda=o.mc_lambda,
            ema_alpha=o.ema_alpha, conf_thresh_high=o.conf_thresh_high,
            conf_thresh_low=o.conf_thresh_low, id_preservation_weight=o.id_preservation_weight,
            crowd_detection=bool(o.crowd_detection), born_confirmed=bool(o.born_confirmed))

    def grown(self, track_cap: int, det_cap: int) -> "SsEngine":
        """A new engine with larger capacities holding this one's state (bx_ss_copy_state)."""
        e = SsEngine(self.n_seq, track_cap, det_cap, self.emb_dim, self.vec_cap, self.params)
        N.check(self._L.bx_ss_copy_state(e._h, self._h), "bx_ss_copy_state")
        return e

    def step(self, dets, det_off, embs, warps, out, out_count, seq0: int = 0,
             nseq: int | None = None, stream=None):
        """One frame for sequences [seq0, seq0+nseq) from device tensors (see bx_ss_step):
        dets [sumN, 6] f64, det_off [S+1] i32, embs [sumN, F] f64, out [sumN, 10] f64."""
        nseq, stream = self._range(seq0, nseq, stream)
        N.check(self._L.bx_ss_step(self._h, seq0, nseq, _ptr(dets), _ptr(det_off), _ptr(embs),
                                   _ptr(warps), _ptr(out), _ptr(out_count), stream), "bx_ss_step")

    def update_host(self, seq: int, dets: np.ndarray, embs: np.ndarray,
                    warp: np.ndarray | None = None) -> np.ndarray:
        d = np.ascontiguousarray(dets, dtype=np.float64).reshape(-1, 6)
        n = d.shape[0]
        e = np.ascontiguousarray(embs, dtype=np.float64).reshape(n, -1) if n else None
        if n and e.shape[1] != self.emb_dim:
            raise ValueError(f"embedding dim {e.shape[1]} != engine emb_dim {self.emb_dim}")
        w = None if warp is None else np.ascontiguousarray(warp, np.float64).reshape(6)
        out = np.empty((max(n, 1), 10), np.float64)
        m = C.c_int(0)
        N.check(self._L.bx_ss_update_host(
            self._h, seq, d.ctypes.data if n else None, n, e.ctypes.data if n else None,
            None if w is None else w.ctypes.data, out.ctypes.data, C.byref(m), None),
            "bx_ss_update_host")
        return out[: m.value].copy()

    def counters(self, seq: int = 0) -> dict:
        fc, nid, nt, nl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        N.check(self._L.bx_ss_counters_host(self._h, seq, C.byref(fc), C.byref(nid), C.byref(nt),
                                            C.byref(nl)), "counters")
        return {"frame_count": fc.value, "next_id": nid.value, "n_tracks": nt.value,
                "n_lost": nl.value}

    def tracks(self, seq: int = 0) -> dict:
        cap = self.track_cap
        ids = np.zeros(cap, np.int32)
        st = np.zeros(cap, np.int32)
        mean = np.zeros((cap, 8))
        cov = np.zeros((cap, 8, 8))
        n = C.c_int()
        N.check(self._L.bx_ss_tracks_host(self._h, seq, cap, ids.ctypes.data, st.ctypes.data,
                                          mean.ctypes.data, cov.ctypes.data, C.byref(n)),
                "tracks")
        k = min(n.value, cap)
        return {"id": ids[:k], "state": st[:k], "mean": mean[:k], "covariance": cov[:k]}

    def state_set(self, seq: int, ids, mean=None, covariance=None) -> None:
        """Write Track.mean [n,8] / Track.covariance [n,8,8] of live tracks by id."""
        n, ids, m, c = _state_arrays(ids, mean, covariance, 8, 64)
        N.check(self._L.bx_ss_state_set_host(self._h, seq, n, ids.ctypes.data, _p(m), _p(c)),
                "state_set")

    def track_attrs(self, seq: int = 0) -> dict:
        """Per track in list order: id, quality_score, conf, _max_age, len(features)."""
        cap = self.track_cap
        ids, mx, nf = (np.zeros(cap, np.int32) for _ in range(3))
        q, cf = np.zeros(cap), np.zeros(cap)
        n = C.c_int()
        N.check(self._L.bx_ss_track_attrs_host(self._h, seq, cap, ids.ctypes.data, q.ctypes.data,
                                               cf.ctypes.data, mx.ctypes.data, nf.ctypes.data,
                                               C.byref(n)), "track_attrs")
        k = min(n.value, cap)
        return {"id": ids[:k], "quality": q[:k], "conf": cf[:k], "max_age": mx[:k],
                "n_features": nf[:k]}

    def track_attrs_set(self, seq: int, ids, quality=None, conf=None, max_age=None) -> None:
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        q = None if quality is None else np.ascontiguousarray(quality, np.float64).reshape(-1)
        c = None if conf is None else np.ascontiguousarray(conf, np.float64).reshape(-1)
        m = None if max_age is None else np.ascontiguousarray(max_age, np.int32).reshape(-1)
        N.check(self._L.bx_ss_track_attrs_set_host(self._h, seq, ids.size, ids.ctypes.data,
                                                   _p(q), _p(c), _p(m)), "track_attrs_set")

    def last_features(self, seq: int, ids) -> np.ndarray:
        """features[-1] of the tracks `ids` ([n, emb_dim] float64)."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        out = np.zeros((ids.size, self.emb_dim))
        if ids.size:
            N.check(self._L.bx_ss_last_feature_host(self._h, seq, ids.size, ids.ctypes.data,
                                                    out.ctypes.data), "last_features")
        return out

    def last_features_set(self, seq: int, ids, feats, normalize: bool = True) -> None:
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        f = np.ascontiguousarray(feats, np.float64).reshape(ids.size, self.emb_dim)
        N.check(self._L.bx_ss_last_feature_set_host(self._h, seq, ids.size, ids.ctypes.data,
                                                    f.ctypes.data, int(bool(normalize))),
                "last_features_set")

    def frame_stats(self, seq0: int = 0, nseq: int | None = None) -> dict:
        nseq = self.n_seq - seq0 if nseq is None else nseq
        a = (C.c_int64 * 7)()
        N.check(self._L.bx_ss_frame_stats_host(self._h, seq0, nseq, a), "frame_stats")
        return dict(zip(["dets", "tracks", "queried", "rows", "outputs", "frame", "matches"],
                        [int(x) for x in a]))

    def set_lsap_mode(self, fast: bool) -> None:
        """Solve + certify the cascade LSAPs (default) or always solve them in scipy's row order
        (bx_ss_set_lsap_mode)."""
        N.check(self._L.bx_ss_set_lsap_mode(self._h, int(bool(fast))), "bx_ss_set_lsap_mode")

    def lsap_stats(self, seq0: int = 0, nseq: int | None = None) -> dict:
        """LSAP counters since creation (bx_ss_lsap_stats_host): solves, certified unique,
        unique up to rejected pairs, ties re-solved in scipy's order, stages restarted."""
        nseq = self.n_seq - seq0 if nseq is None else nseq
        a = (C.c_int64 * 5)()
        N.check(self._L.bx_ss_lsap_stats_host(self._h, seq0, nseq, a), "lsap_stats")
        return dict(zip(["solves", "unique", "unique_up_to_rejected", "ties", "restarts"],
                        [int(x) for x in a]))


class SsTableEngine(_SeqTable, SsEngine):
    """An ``SsEngine`` with per-sequence ``SsParams`` (``_SeqTable``; include/bxstrongsort.h,
    boxmot_amd.tune.sweep_strong).  The capacities, ``emb_dim`` and ``vec_cap`` stay the
    engine's, and an entry's ``nn_budget`` may not exceed the engine's own, which sized the
    galleries.  ``max_age``, ``nn_budget`` and ``max_cos_dist`` of an entry seed the state crowd
    mode adapts, so a sequence takes an entry only at frame counter 0 (fresh or just reset):
    ``set_seq_params`` raises ``ValueError`` for a sequence that has run a frame since its last
    reset, and for an entry ``SsEngine`` would refuse; ``seq_params`` gives the three as seeded,
    not as crowd mode adapted them.  (A class of its own because SsEngine's method set is pinned
    by tests/test_engine_api_host.py.)"""

    def grown(self, track_cap: int, det_cap: int) -> "SsTableEngine":
        """As SsEngine.grown; bx_ss_copy_state carries the tracks and the sequences' adapted
        state but not the table, which is set on the new engine first: its sequences are at
        frame counter 0 then, as the call requires."""
        e = self._retable(SsTableEngine(self.n_seq, track_cap, det_cap, self.emb_dim,
                                        self.vec_cap, self.params))
        N.check(self._L.bx_ss_copy_state(e._h, self._h), "bx_ss_copy_state")
        if hasattr(self, "occ_cap"):  # (the copy carried pools, latches and settings)
            e.occ_cap = self.occ_cap
        return e

    # ---- occlusion handling on the device (bx_ss_set_occlusion_host).  Here and not on SsEngine
    # for the reason the class exists: SsEngine's method set is pinned.  An engine on which
    # neither a table nor occlusion was set launches SsEngine's kernels.
    def set_occlusion(self, seq0: int, on, threshold, nseq: int | None = None,
                      occ_cap: int = 32) -> None:
        """``handle_occlusions`` / ``occlusion_threshold`` of sequences [seq0, seq0 + nseq):
        ``on`` and ``threshold`` are scalars or one value per sequence (nseq defaults to their
        length, or to every sequence from seq0 for two scalars).  From the first call on every
        frame of this engine ends with the occlusion pass (OcclusionHandler's edits, on the
        device); it allocates ``occ_cap`` buffered tracks per sequence, fixed from then on.
        ``ValueError`` for a sequence that has run a frame since its last reset, or another
        ``occ_cap``.  ``grown()`` carries settings, pools and latches over."""
        on_a, thr_a = np.atleast_1d(np.asarray(on)), np.atleast_1d(np.asarray(threshold))
        if nseq is None:
            nseq = max(on_a.size, thr_a.size) if max(on_a.size, thr_a.size) > 1 \
                else self.n_seq - seq0
        on_a = np.ascontiguousarray(np.broadcast_to(on_a != 0, (nseq,)), np.int32)
        thr_a = np.ascontiguousarray(np.broadcast_to(thr_a, (nseq,)), np.float64)
        N.check(self._L.bx_ss_set_occlusion_host(self._h, int(seq0), int(nseq), on_a.ctypes.data,
                                                 thr_a.ctypes.data, int(occ_cap), None),
                "bx_ss_set_occlusion_host")
        self.occ_cap = int(occ_cap)

    def occlusion(self, seq: int = 0) -> dict:
        """Sequence ``seq``'s settings, the update count at which a mutual occlusion latched (0:
        none; the reference raises TypeError there) and the buffered tracks."""
        on, mf, nb, thr = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        N.check(self._L.bx_ss_occlusion_host(self._h, int(seq), C.byref(on), C.byref(thr),
                                             C.byref(mf), C.byref(nb)), "bx_ss_occlusion_host")
        return {"on": bool(on.value), "threshold": thr.value, "mutual_frame": mf.value,
                "n_buffered": nb.value}

    def occlusion_buffer(self, seq: int, id: int) -> np.ndarray:
        """The buffered features of track ``id``, oldest first ([n, emb_dim], n <= 10; n = 0
        without a buffer): OcclusionStateManager.occlusion_buffer[id]."""
        v = np.zeros((10, self.emb_dim))
        n = C.c_int()
        N.check(self._L.bx_ss_occlusion_buffer_host(self._h, int(seq), int(id), v.ctypes.data,
                                                    C.byref(n)), "bx_ss_occlusion_buffer_host")
        return v[: n.value].copy()


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    raise TypeError(type(x))


def _current_stream():
    try:
        import torch

        if torch.cuda.is_available():
            return torch.cuda.current_stream().cuda_stream
    except Exception:
        pass
    return None

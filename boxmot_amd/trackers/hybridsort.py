"""HybridSort on the MI355X engine — drop-in for boxmot.trackers.hybridsort.hybridsort.HybridSort
(reference trackers/hybridsort/hybridsort.py:350-741).

Same constructor signature and defaults (``reid_weights``, ``device``, ``half`` are accepted for
compatibility; ``det_thresh`` has no default, as in the reference), same ``update(dets, img,
embs)`` contract and output rows (ids start at 1).  The frame — the 9-state Kalman filter that
also tracks the detection score, the two appearance distances per pair (smoothed feature and
30-deep feature-bank mean) on the fp64 matrix cores, the association on asso_func + four-corner
direction consistency - score difference + appearance, the long-term-ReID correction filter, the
OCR round, the feature moving average, births and deaths — is three kernel launches.

The reference does not run as published; this follows it with the patches H1-H3 of
tests/golden/make_golden_hybridsort.py.  Like the reference, column 7 of the
output rows is a confidence, not a detection index: HybridSort reads ``cls`` and ``det_ind`` from
the unfiltered frame at an index into the kept detections, ``det_ind`` from its score column
(hybridsort.py:458,467,604).

Camera-motion compensation is the reference's ``ECC`` attribute (hybridsort.py:417, 448-451;
like there it is no constructor argument, ``tracker.ECC = True`` switches it on, and
``HybridSortPerClass`` alone takes it as a keyword): while it is true every frame starts with ``self.cmc.apply(img,
dets)`` (``boxmot_amd.ECC()`` unless another estimator is assigned; built on the first frame
that needs it), the warp is rounded to float32, the type the reference's estimator returns, and
every live track's ``camera_update`` runs under it on the device before the predict, under an
identity warp too.  Where the reference raises on a state score of exactly 0
the track is left as it was (``engine.ecc(0)["score_zero_skips"]`` counts them).

Out of scope: the ReID embeddings are an input (``embs``; the reference would run its ReID
backend) and ``use_byte=True`` (the reference's BYTE round cannot run).  Embeddings are float64
on the engine: ``embs`` is converted with ``np.asarray(embs, np.float64)``.

``HybridSort(per_class=True)`` still raises NotImplementedError; the mode is the subclass
``HybridSortPerClass`` (basetracker.py:155-201): class c is engine sequence c, all classes share the
frame counter and the class-level id counter; the class split of the frame's rows and the merge
of the classes' rows under class-global ids run on the device around the same three launches
(``HybridsortEngine.update_classes_host``, include/bxclasses.h).
"""
from __future__ import annotations

import numpy as np

from ..engine import HybridsortCmcEngine, HybridsortEngine, HybridsortParams
from ..iou import KINDS
from .basetracker import BaseTracker, CapacityGuard, ClassMapGuard, model_embs


class HybridSort(BaseTracker):
    _PER_CLASS = False  # HybridSortPerClass: the per_class mode is built
    # KalmanBoxTracker.count is a class attribute shared by every instance and reset by each
    # HybridSort constructor (hybridsort.py:115,176-177,418); output ids are count + 1: mirrored
    # here as a counter that starts at 1.
    _id_count = 1
    model = None  # a ReID backend (get_features(xyxys, img)): embeds when `embs` is missing

    def __init__(self, reid_weights, device, half, det_thresh, per_class: bool = False,
                 max_age: int = 30, min_hits: int = 3, iou_threshold: float = 0.3,
                 delta_t: int = 3, asso_func: str = "iou", inertia: float = 0.2,
                 longterm_reid_weight: float = 0, TCM_first_step_weight: float = 0,
                 use_byte: bool = False, track_cap: int = 256, det_cap: int = 256):
        if use_byte:
            raise NotImplementedError(
                "HybridSort(use_byte=True) is not built: the reference's BYTE round calls "
                "KalmanBoxTracker.update with the wrong arguments, so it defines no behaviour")
        if per_class and not self._PER_CLASS:
            raise NotImplementedError(
                "HybridSort(per_class=True) is not wired up: the per_class mode on the MI355X "
                "engine is the class HybridSortPerClass")
        super().__init__(max_age=max_age, per_class=per_class, asso_func=asso_func)
        # (HybridSortPerClass sets _nr_classes before this constructor runs, as DeepOcSortPerClass)
        self.nr_classes = int(getattr(self, "_nr_classes", self.nr_classes))
        self.max_age = max_age
        self.min_hits = min_hits
        self.iou_threshold = iou_threshold
        self.det_thresh = det_thresh
        self.delta_t = delta_t
        self.inertia = inertia
        self.use_byte = use_byte
        self.longterm_reid_weight = longterm_reid_weight
        self.TCM_first_step_weight = TCM_first_step_weight
        self.ECC = False  # a plain attribute, as in the reference: read at every update
        self._cmc = None  # the estimator, built by the first read of `cmc`
        HybridSort._id_count = 1
        # an unknown asso_func never reaches the engine: setup_decorator raises ValueError for it
        # on the first update (basetracker.py:140-147), as DeepOcSort's; "iou" only fills the field
        self._params = HybridsortParams(
            det_thresh=det_thresh, max_age=max_age, min_hits=min_hits,
            iou_threshold=iou_threshold, delta_t=delta_t,
            asso_func=asso_func if asso_func in KINDS else "iou", inertia=inertia,
            longterm_reid_weight=longterm_reid_weight,
            TCM_first_step_weight=TCM_first_step_weight)
        self._caps = (track_cap, det_cap)
        self._cap = CapacityGuard()
        self._map = ClassMapGuard()
        self._engine_ids = 1
        self._frame_latched = False
        # the embedding width is learnt from the first frame that has detections; empty frames
        # before it are counted and replayed into the engine once it exists
        self.engine = None
        self._empty_before_engine = 0

    @property
    def cmc(self):
        """The camera-motion estimator (``apply(img, dets)`` -> a 2x3 affine): ``boxmot_amd.ECC()``,
        the reference's ``get_cmc_method("ecc")()``, built on first use; assignable."""
        if self._cmc is None:
            from ..cmc import ECC

            self._cmc = ECC()
        return self._cmc

    @cmc.setter
    def cmc(self, value):
        self._cmc = value

    def _make_engine(self, emb_dim: int) -> HybridsortEngine:
        # (with ECC on: the engine that takes warps; its switches are set in _sync_ecc)
        cls = HybridsortCmcEngine if self.ECC else HybridsortEngine
        return cls(n_seq=self.nr_classes if self.per_class else 1, track_cap=self._caps[0],
                   det_cap=self._caps[1], emb_dim=emb_dim, params=self._params)

    def _warp(self, img, dets):
        """One class call's ``self.cmc.apply(img, dets)`` (hybridsort.py:448-451), rounded to
        float32 as the reference's estimator returns it."""
        w = self.cmc.apply(img, dets)
        return np.asarray(w, np.float64).reshape(2, 3).astype(np.float32).astype(np.float64)

    def _sync_ecc(self) -> bool:
        """The engine's switches follow the attribute; returns it.  The first frame with ECC on
        moves a plain engine's state into one that takes warps."""
        on = bool(self.ECC)
        if not isinstance(self.engine, HybridsortCmcEngine):
            if not on:
                return False
            old = self.engine
            has_cls = self.per_class and old.classes() is not None
            self.engine = HybridsortCmcEngine.grown(old, old.track_cap, old.det_cap,
                                                    self._map.cap if has_cls else None)
            old.close()
        if self.engine.ecc_on(0) != on:  # (the host mirror: nothing waits on the device)
            self.engine.set_ecc(0, on)
        return on

    @BaseTracker.setup_decorator
    @BaseTracker.per_class_decorator
    def update(self, dets: np.ndarray, img: np.ndarray, embs: np.ndarray = None) -> np.ndarray:
        self.check_inputs(dets, img, embs)
        n = int(dets.shape[0])
        embs = model_embs(self, dets, img, embs)
        if n and embs is None:
            raise ValueError("HybridSort on the MI355X engine needs `embs`: ReID inference is "
                             "outside the association path")
        e = np.asarray(embs, np.float64).reshape(n, -1) if n else None
        if self.engine is None:
            if e is None:
                # nothing to learn the embedding width from yet: an empty frame on an empty
                # tracker only advances the frame counter; replayed below
                self.frame_count += 1
                self._empty_before_engine += 1
                if self.ECC:  # (the estimator keeps state: it sees every frame)
                    for _ in range(self.nr_classes if self.per_class else 1):
                        self.cmc.apply(img, dets)
                return np.empty((0, 8))
            self.engine = self._make_engine(e.shape[1])
            for _ in range(self._empty_before_engine):
                if self.per_class:
                    self.engine.update_classes_host(0, self.nr_classes, np.empty((0, 6), np.float32),
                                                    None, HybridSort._id_count)
                else:
                    self.engine.update_host(0, np.empty((0, 6), np.float32))
            self._empty_before_engine = 0
        if not self._frame_latched and self._first_frame_processed:
            # the engine's centroid frame size follows BaseTracker's first-frame latch
            for q in range(self.engine.n_seq):
                self.engine.set_frame_size(q, self.w, self.h)
            self._frame_latched = True
        self.frame_count += 1
        if self.per_class:
            # class c runs as engine sequence c (its births are at most its detections), one
            # native call; the class-level id counter goes in and comes back
            C = self.nr_classes
            self.engine = self._cap.fit(self.engine, ClassMapGuard.class_counts(dets, C), n)
            self.engine = self._map.fit(self.engine, C, n)
            warps = None
            if self._sync_ecc():
                # one CMC call per class call, on that class's rows (basetracker.py:175-189 ->
                # hybridsort.py:448-449), as DeepOcSortPerClass
                d = np.asarray(dets, np.float32).reshape(-1, 6)
                warps = np.stack([self._warp(img, d[d[:, 5] == c]) for c in range(C)])
            out, HybridSort._id_count = self.engine.update_classes_host(
                0, C, dets, e, HybridSort._id_count, *([warps] if warps is not None else []))
            return out if out.shape[0] else np.empty((0, 8))
        self.engine = self._cap.fit(self.engine, {0: n}, n)
        warp = self._warp(img, dets) if self._sync_ecc() else None
        if self._engine_ids != HybridSort._id_count:
            self.engine.set_id_count(0, HybridSort._id_count)
        out = self.engine.update_host(0, dets, e, *([warp] if warp is not None else []))
        self._engine_ids = HybridSort._id_count = self.engine.counters(0)["id_count"]
        return out if out.shape[0] else np.empty((0, 8))

    @property
    def active_tracks(self):
        """Track list snapshot: id, Kalman state (x [9], P [9, 9]), smoothed feature and the
        number of features pushed into the bank, per track (per_class: the list of the class that
        ran last, as the reference's swap leaves it)."""
        return self._seq_tracks(self.nr_classes - 1 if self.per_class else 0)

    def _seq_tracks(self, q):
        if self.engine is None:
            return []
        snap = self.engine.tracks(q)
        ids = snap["id"]
        if self.per_class and ids.shape[0]:  # the class-global ids the rows carry
            ids = self.engine.classes().id_map(0, q)[ids - 1]
        return [{"id": int(ids[k]), "x": snap["x"][k], "P": snap["P"][k],
                 "emb": snap["emb"][k], "bank_count": int(snap["bank_count"][k])}
                for k in range(ids.shape[0])]

    def _class_active_lists(self):
        # class c is engine sequence c
        return [self._seq_tracks(c) for c in range(self.nr_classes)]


class HybridSortPerClass(HybridSort):
    """HybridSort with per_class=True (see the module docstring): the reference's constructor
    arguments without ``per_class``, plus ``nr_classes`` (BaseTracker's 80; fewer classes keep the
    engine, one sequence per class, small).  Shares HybridSort's class-level id counter."""

    _PER_CLASS = True

    def __init__(self, reid_weights, device, half, det_thresh, nr_classes: int = 80, **kwargs):
        kwargs.pop("per_class", None)
        ecc = bool(kwargs.pop("ECC", False))
        self._nr_classes = int(nr_classes)
        super().__init__(reid_weights, device, half, det_thresh, per_class=True, **kwargs)
        self.ECC = ecc

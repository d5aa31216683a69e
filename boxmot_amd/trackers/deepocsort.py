"""DeepOCSort on the MI355X engine — drop-in for boxmot.trackers.deepocsort.deepocsort.DeepOcSort
(reference trackers/deepocsort/deepocsort.py:238-498).

Same constructor signature and defaults (``reid_weights``, ``device``, ``half`` are accepted for
compatibility), same ``update(dets, img, embs)`` contract and output rows (ids start at 1).  The
frame — CMC affine correction of every track, XYSR Kalman predict/update with ORU, the appearance
contraction on the fp64 matrix cores, the association on asso_func + direction consistency + the
adaptively weighted appearance term, the OCR round, the embedding moving average, births and
deaths — is three kernel launches.  Like the OCSort drop-in it follows the reference with the
patches P1-P5.

Out of scope and therefore required as inputs: the ReID embeddings (``embs``; the reference would
run its ReID backend when they are missing) and the camera-motion warp — ``self.cmc.apply(img,
boxes)`` must return a 2x3 affine (identity by default; the reference's sparse-optical-flow
estimator is image processing outside the association path).

Embeddings are float64 on the engine: ``embs`` is converted with ``np.asarray(embs,
np.float64)``.  With float32 ``embs`` the reference runs in mixed width — a newborn track keeps
its float32 row, so ``dets_embs @ trk_embs.T`` is a single-precision product until a track's
first update and double precision afterwards.  That is not reproduced: here the product is
always double precision over the converted values.

``DeepOcSort(per_class=True)`` still raises NotImplementedError; the mode is the subclass
``DeepOcSortPerClass`` (basetracker.py:155-201): class c is engine sequence c, all classes share the
frame counter and the class-level id counter; the class split of the frame's rows and the merge
of the classes' rows under class-global ids run on the device around the same three launches
(``DeepOcsortEngine.update_classes_host``, include/bxclasses.h).  The CMC is asked once per class
id with that class's boxes over ``det_thresh``, as the reference's class calls do.
"""
from __future__ import annotations

import numpy as np

from ..engine import DeepOcsortEngine, DeepOcsortParams
from ..iou import KINDS
from .basetracker import BaseTracker, CapacityGuard, ClassMapGuard, model_embs
from .botsort import IdentityCMC


class DeepOcSort(BaseTracker):
    _PER_CLASS = False  # DeepOcSortPerClass: the per_class mode is built
    # KalmanBoxTracker.count is a class attribute shared by every instance and set to 1 by each
    # DeepOcSort constructor (deepocsort.py:56,117-118,305): mirrored here.
    _id_count = 1
    model = None  # a ReID backend (get_features(xyxys, img)): embeds when `embs` is missing

    def __init__(self, reid_weights=None, device=None, half: bool = False,
                 per_class: bool = False, det_thresh: float = 0.3, max_age: int = 30,
                 min_hits: int = 3, iou_threshold: float = 0.3, delta_t: int = 3,
                 asso_func: str = "iou", inertia: float = 0.2, w_association_emb: float = 0.5,
                 alpha_fixed_emb: float = 0.95, aw_param: float = 0.5,
                 embedding_off: bool = False, cmc_off: bool = False, aw_off: bool = False,
                 Q_xy_scaling: float = 0.01, Q_s_scaling: float = 0.0001,
                 track_cap: int = 256, det_cap: int = 256, **kwargs):
        if per_class and not self._PER_CLASS:
            raise NotImplementedError(
                "DeepOcSort(per_class=True) is not wired up: the per_class mode on the MI355X "
                "engine is the class DeepOcSortPerClass")
        super().__init__(max_age=max_age, per_class=per_class, asso_func=asso_func)
        # (DeepOcSortPerClass sets _nr_classes before this constructor runs: the engine below, one
        # sequence per class, may be built here)
        self.nr_classes = int(getattr(self, "_nr_classes", self.nr_classes))
        self.max_age = max_age
        self.min_hits = min_hits
        self.iou_threshold = iou_threshold
        self.det_thresh = det_thresh
        self.delta_t = delta_t
        self.inertia = inertia
        self.w_association_emb = w_association_emb
        self.alpha_fixed_emb = alpha_fixed_emb
        self.aw_param = aw_param
        self.Q_xy_scaling = Q_xy_scaling
        self.Q_s_scaling = Q_s_scaling
        self.embedding_off = embedding_off
        self.cmc_off = cmc_off
        self.aw_off = aw_off
        self.cmc = IdentityCMC()
        DeepOcSort._id_count = 1
        self._params = DeepOcsortParams(
            det_thresh=det_thresh, max_age=max_age, min_hits=min_hits,
            iou_threshold=iou_threshold, delta_t=delta_t,
            asso_func=asso_func if asso_func in KINDS else "iou", inertia=inertia,
            w_association_emb=w_association_emb, alpha_fixed_emb=alpha_fixed_emb,
            aw_param=aw_param, embedding_off=embedding_off, aw_off=aw_off,
            Q_xy_scaling=Q_xy_scaling, Q_s_scaling=Q_s_scaling)
        self._caps = (track_cap, det_cap)
        self._cap = CapacityGuard()
        self._map = ClassMapGuard()
        self._engine_ids = 1
        self._frame_latched = False
        # the embedding width is learnt from the first frame that has detections; empty frames
        # before it are counted and replayed into the engine once it exists
        self.engine = self._make_engine(0) if embedding_off else None
        self._empty_before_engine = 0

    def _make_engine(self, emb_dim: int) -> DeepOcsortEngine:
        return DeepOcsortEngine(n_seq=self.nr_classes if self.per_class else 1, track_cap=self._caps[0], det_cap=self._caps[1],
                                emb_dim=emb_dim, params=self._params)

    @BaseTracker.setup_decorator
    @BaseTracker.per_class_decorator
    def update(self, dets: np.ndarray, img: np.ndarray, embs: np.ndarray = None) -> np.ndarray:
        self.check_inputs(dets, img, embs)
        n = int(dets.shape[0])
        embs = model_embs(self, dets, img, embs, not self.embedding_off)
        if not self.embedding_off and n and embs is None:
            raise ValueError("DeepOcSort(embedding_off=False) on the MI355X engine needs `embs`: "
                             "ReID inference is outside the association path")
        e = None
        if not self.embedding_off and n:
            e = np.asarray(embs, np.float64).reshape(n, -1)
        if self.engine is None:
            if e is None:
                # nothing to learn the embedding width from yet.  An empty frame on an empty
                # tracker only advances the frame counter (and calls the CMC, which may keep
                # state): it is replayed below when the first embeddings arrive
                self.frame_count += 1
                self._empty_before_engine += 1
                if not self.cmc_off:
                    for _ in range(self.nr_classes if self.per_class else 1):  # one per class call
                        self.cmc.apply(img, np.empty((0, 4)))
                return np.empty((0, 8)) if self.per_class else np.array([])
            self.engine = self._make_engine(e.shape[1])
            for _ in range(self._empty_before_engine):
                if self.per_class:
                    self.engine.update_classes_host(0, self.nr_classes, np.empty((0, 6), np.float32),
                                                    None, DeepOcSort._id_count)
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
            return self._update_classes(dets, img, e, n)
        self.engine = self._cap.fit(self.engine, {0: n}, n)
        warp = None
        if not self.cmc_off:
            # deepocsort.py:353: the boxes of the detections over det_thresh
            d = np.asarray(dets, np.float32).reshape(-1, 6)
            boxes = d[d[:, 4] > self.det_thresh][:, :4].astype(np.float64)
            warp = np.asarray(self.cmc.apply(img, boxes), np.float64).reshape(2, 3)
            warp = None if np.array_equal(warp, np.eye(2, 3)) else warp
        if self._engine_ids != DeepOcSort._id_count:
            self.engine.set_id_count(0, DeepOcSort._id_count)
        out = self.engine.update_host(0, dets, e, warp)
        self._engine_ids = DeepOcSort._id_count = self.engine.counters(0)["id_count"]
        return out if out.shape[0] else np.array([])

    def _update_classes(self, dets, img, e, n):
        """The per_class=True frame: class c runs as engine sequence c (its births are at most its
        detections), one native call; the class-level id counter goes in and comes back."""
        C = self.nr_classes
        self.engine = self._cap.fit(self.engine, ClassMapGuard.class_counts(dets, C), n)
        self.engine = self._map.fit(self.engine, C, n)
        warps = None
        if not self.cmc_off:
            # one CMC call per class id, on the boxes of that class's detections over det_thresh
            # (basetracker.py:175-189 -> deepocsort.py:353)
            d = np.asarray(dets, np.float32).reshape(-1, 6)
            warps = np.empty((C, 2, 3), np.float64)
            for c in range(C):
                cd = d[d[:, 5] == c]
                boxes = cd[cd[:, 4] > self.det_thresh][:, :4].astype(np.float64)
                warps[c] = np.asarray(self.cmc.apply(img, boxes), np.float64).reshape(2, 3)
            warps = None if np.array_equal(warps, np.broadcast_to(np.eye(2, 3), warps.shape)) \
                else warps
        out, DeepOcSort._id_count = self.engine.update_classes_host(
            0, C, dets, e, DeepOcSort._id_count, warps)
        return out if out.shape[0] else np.empty((0, 8))

    @property
    def active_tracks(self):
        """Track list snapshot: id, XYSR Kalman state (x [7], P [7, 7]) and, unless
        embedding_off, the embedding per track (per_class: the list of the class that ran last,
        as the reference's swap leaves it)."""
        return self._seq_tracks(self.nr_classes - 1 if self.per_class else 0)

    def _seq_tracks(self, q):
        if self.engine is None:
            return []
        snap = self.engine.tracks(q)
        ids = snap["id"]
        if self.per_class and ids.shape[0]:  # the class-global ids the rows carry
            ids = self.engine.classes().id_map(0, q)[ids - 1]
        emb = snap.get("emb")
        return [{"id": int(ids[k]), "x": snap["x"][k], "P": snap["P"][k],
                 **({} if emb is None else {"emb": emb[k]})} for k in range(ids.shape[0])]

    def _class_active_lists(self):
        # class c is engine sequence c
        return [self._seq_tracks(c) for c in range(self.nr_classes)]


class DeepOcSortPerClass(DeepOcSort):
    """DeepOcSort with per_class=True (see the module docstring): the reference's constructor
    arguments without ``per_class``, plus ``nr_classes`` (BaseTracker's 80; fewer classes keep the
    engine, one sequence per class, small).  Shares DeepOcSort's class-level id counter."""

    _PER_CLASS = True

    def __init__(self, reid_weights=None, device=None, half: bool = False, nr_classes: int = 80,
                 **kwargs):
        kwargs.pop("per_class", None)
        self._nr_classes = int(nr_classes)
        super().__init__(reid_weights, device, half, per_class=True, **kwargs)

"""Hyper-parameter sweeps on the batched engine: K configurations x S sequences as ONE engine.

Reference stage replaced (``boxmot/engine/evolve.py``): its objective function runs the tracker
over all sequences with one configuration and evaluates, once per trial.  Here the K
configurations of a sweep run together: a table engine (``engine._SeqTable``) of K*S sequences is
built, engine sequence ``k*S + s`` is sequence ``s`` under configuration ``k``
(``set_seq_params``), and every frame index is one K*S-wide launch fed from device memory, the K*S
sequences reading each sequence's detections and embeddings from ONE copy
(``engine.SharedSequenceFeeder``, include/bxfeed.h).  The search strategy (which configurations
to try) stays with the caller; ``grid`` builds the cartesian product of a search space.

One driver, ``_run_sweep``, runs every sweep: the refusals that need no engine, the sequences and
their frame tables, every config resolved as ``run_sequences`` resolves it, the engine, the
feeder, the frame loop (``_drive``) and the report (``_report``).  What a tracker family adds is a
``_Spec`` in ``_SPECS``: its trackers, its own refusals, how its engine is built and stepped,
whether embeddings, frame sizes and warps apply, and the feeder's format.  The public sweeps are
signatures and documentation over it: ``sweep`` (OCSort; DESIGN.md 2.18 is the contract),
``sweep_reid`` (DeepOCSort, HybridSort; 2.20), ``sweep_bot`` (ByteTrack, BoT-SORT; 2.22),
``sweep_boost`` (BoostTrack, whose variants differ in constructor flags only; 2.23) and
``sweep_strong`` (StrongSort; 2.24), whose spec carries hooks of its own: float64 detections and
10-column rows from the feeder, and an occlusion post-process that stays on the host, per sweep,
unless ``occlusion="device"`` asks for the engine's own pass (2.26).

``sweep_gsi`` runs any of the five with GSI between tracking and scoring, on the
feeder's result slots in device memory (``postprocessing.gsi_device``, include/bxgsi.h).
"""
from __future__ import annotations

import dataclasses
import itertools
from pathlib import Path

import numpy as np

SUPPORTED = ("ocsort",)
SUPPORTED_REID = ("deepocsort", "hybridsort")  # sweep_reid's trackers
SUPPORTED_BOT = ("bytetrack", "botsort")       # sweep_bot's trackers
SUPPORTED_BOOST = ("boosttrack",)              # sweep_boost's tracker
SUPPORTED_STRONG = ("strongsort",)             # sweep_strong's tracker
_CAPS = ("track_cap", "det_cap")


def grid(space: dict) -> list:
    """The cartesian product of ``space`` (name -> list of values; names are OcSort's constructor
    arguments) as a list of dicts, the last name varying fastest."""
    names = list(space)
    return [dict(zip(names, v)) for v in itertools.product(*[list(space[n]) for n in names])]


SCORES = ("host", "device")


def _check(tracker_type: str, configs, sequences=None, gt=None, exp_dir=None, score="host",
           keep_results=True, supported=SUPPORTED, what="tune.sweep") -> list:
    """The refusals of ``sweep`` (and, with its own trackers, ``sweep_reid``) that need no
    engine."""
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {score!r}")
    if score == "device" and gt is None:
        raise ValueError('score="device" scores against gt: give gt')
    if not keep_results:
        if gt is None:
            raise ValueError("keep_results=False without gt would return nothing")
        if exp_dir is not None:
            raise ValueError("keep_results=False: exp_dir needs the rows on the host")
        if score == "host":
            raise ValueError('keep_results=False: score="host" needs the rows on the host; '
                             'use score="device"')
    if tracker_type not in supported:
        raise NotImplementedError(
            f"{what} drives {', '.join(supported)} only (the engine with per-sequence "
            f"parameters), not {tracker_type}")
    configs = [dict(c) for c in configs]
    if not configs:
        raise ValueError(f"{what} needs at least one config")
    for k, c in enumerate(configs):
        if "per_class" in c:
            raise NotImplementedError(f"config {k}: per_class is not available in a sweep")
    for cap in _CAPS:
        if len({repr(c.get(cap)) for c in configs}) > 1:
            raise ValueError(f"{cap} sizes the engine's memory: it must be absent from every "
                             f"config or equal in all of them")
    if score == "device" and sequences is not None and list(gt) != list(sequences):
        raise ValueError('score="device" reads the engine\'s sequences in place: gt must name '
                         'the same sequences in the same order')
    return configs


def _resolve_reid(tracker_type: str, F: int, cfg: dict, more=()):
    """(params, track_cap, det_cap, and the attributes ``more`` names) of one config, resolved as
    run_sequences resolves its tracker_kwargs: through ``motio._batched_engine`` itself, on a
    one-sequence engine."""
    from . import motio

    eng = motio._batched_engine(tracker_type, 1, F, cfg)[0]
    try:
        return (eng.params, eng.track_cap, eng.det_cap, *[getattr(eng, a) for a in more])
    finally:
        eng.close()


def _resolve(cfg: dict):
    """``_resolve_reid`` for OCSort: (OcsortParams, track_cap, det_cap)."""
    return _resolve_reid("ocsort", 0, cfg)


@dataclasses.dataclass(frozen=True)
class _Spec:
    """What one public sweep adds to ``_run_sweep``.  ``extra`` names the keyword arguments beyond
    the driver's own; they reach ``check``, ``engine`` and ``drive``, which hold their defaults."""

    name: str                  # the public sweep, as _check names it in its refusals
    supported: tuple           # its trackers
    engine: object             # (E, tracker_type, n_seq, F, resolved, **extra) -> (engine, feed_emb):
    #                            the table engine, E the engine module, and the embedding width fed
    step: object               # (eng, tracker_type, feed_emb, run, warp): one run of a frame index
    check: object = None       # its own refusals: (tracker_type, configs, warps, score,
    #                            keep_results, **extra)
    embeddings: bool = True    # the sequences' embedding width F matters (else F = 0)
    frame_sizes: bool = False  # the public sweep takes frame_sizes
    warps: bool = True         # ... and warps
    feeder_kw: dict = dataclasses.field(default_factory=dict)  # SharedSequenceFeeder's format
    resolve_more: tuple = ()   # further attributes of the resolved one-sequence engine
    seq_check: object = None   # refusals that need the sequences: (seqs, widths, dets)
    drive: object = None       # in _drive's place: (eng, feed, step, tail, resolved, names, fids,
    #                            tables, **extra) -> (rows, summaries), tail = _drive's arguments
    extra: tuple = ()          # the names of those keyword arguments

    @property
    def keywords(self) -> set:
        """The keyword arguments the sweep accepts: the public sweep's, and ``extra``."""
        return {"exp_dir", "gt", "benchmark", "seq_lengths", "frame_ids", "score", "keep_results",
                *(["frame_sizes"] if self.frame_sizes else []),
                *(["warps"] if self.warps else []), *self.extra}


def _run_sweep(spec: _Spec, tracker_type, sequences, configs, post=None, *, exp_dir, gt, benchmark,
               seq_lengths, frame_ids, score, keep_results, frame_sizes=None, warps=None,
               **extra) -> list:
    """Every public sweep; ``post``: None, or ``sweep_gsi``'s (interval, tau).  The refusals come
    in this order: ``_check`` and the family's own, the return for no sequences, the sequences'
    embedding widths, the configs as they resolve, and then the engine is built."""
    configs = _check(tracker_type, configs, sequences, gt, exp_dir, score, keep_results,
                     supported=spec.supported, what=f"tune.{spec.name}")
    if spec.check is not None:
        spec.check(tracker_type, configs, warps, score, keep_results, **extra)
    from . import engine as E  # (looked up when the sweep runs: tests replace its classes)
    from . import motio

    names = list(sequences)
    seqs = [s if isinstance(s, motio.BinSequence) else motio.BinSequence(s)
            for s in sequences.values()]
    S, K = len(seqs), len(configs)
    if not S:
        return [{"config": c, "results": {} if keep_results else None, "summary": None}
                for c in configs]
    widths = sorted({int(s.emb_dim) for s in seqs}) if spec.embeddings else [0]
    dets = [np.asarray(s.dets).astype(np.float32) for s in seqs]
    if spec.seq_check is not None:
        spec.seq_check(seqs, widths, dets)
    if len(widths) > 1:
        raise ValueError(f"the sequences' embedding widths differ ({widths}): one engine has one "
                         "emb_dim")
    F = widths[0]
    fids, tables = _frame_tables(names, seqs, frame_ids)
    table = None
    if warps is not None:  # [T, S, 6] as run_sequences builds it, then every config's copy
        table = motio._flow_warps(names, seqs, fids, F, warps, None, None).repeat(1, K, 1)
    more = {"more": spec.resolve_more} if spec.resolve_more else {}
    resolved = [_resolve_reid(tracker_type, F, c, **more) for c in configs]
    eng, feed_emb = spec.engine(E, tracker_type, K * S, F, resolved, **extra)
    feed = None
    try:
        for k in range(K):
            eng.set_seq_params(k * S, [resolved[k][0]] * S)
            for q, nm in enumerate(names):
                if frame_sizes and nm in frame_sizes:
                    eng.set_frame_size(k * S + q, *frame_sizes[nm])
        none = [None] * ((K - 1) * S)
        feed = E.SharedSequenceFeeder(dets + none, [s.embs if feed_emb else None for s in seqs]
                                      + none, tables * K, feed_emb, source=list(range(S)) * K,
                                      **spec.feeder_kw)

        def step(t, run):
            q0, ns = run[:2]
            spec.step(eng, tracker_type, feed_emb, run,
                      None if table is None else table[t, q0: q0 + ns])

        tail = (K, gt, benchmark, seq_lengths, score, keep_results, post)
        if spec.drive is None:
            rows, summaries = _drive(eng, feed, step, *tail)
        else:
            rows, summaries = spec.drive(eng, feed, step, tail, resolved, names, fids, tables,
                                         **extra)
    finally:
        if feed is not None:
            feed.close()
        eng.close()
    return _report(configs, names, rows, summaries, exp_dir, gt, benchmark, seq_lengths, post)


def sweep(tracker_type: str, sequences: dict, configs, *, exp_dir=None, gt: dict | None = None,
          benchmark: str = "MOT17", seq_lengths: dict | None = None,
          frame_ids: dict | None = None, frame_sizes: dict | None = None,
          score: str = "host", keep_results: bool = True) -> list:
    """Run every config of ``configs`` over every sequence in one batched engine.

    sequences / frame_ids / frame_sizes: as in ``motio.run_sequences``.  configs: K dicts of
    tracker kwargs, each meaning what ``run_sequences("ocsort", ..., tracker_kwargs=cfg)`` makes
    of it (an empty dict is create_tracker's YAML defaults, a non-empty one goes through the
    drop-in's constructor as an ``evolve_param_dict`` does).  ``track_cap`` / ``det_cap`` must be
    absent or equal across configs (``ValueError``), ``per_class`` and trackers other than ocsort
    raise ``NotImplementedError``; all three before any engine is built.

    Returns one entry per config: ``{"config": cfg, "results": {name: [n, 9] float64 MOT rows},
    "summary": mot_summary of the config or None without gt}``.  With ``exp_dir`` the rows are
    also written to ``exp_dir/<k as 4 digits>/<name>.txt``, byte-identical to run_sequences'
    files.  With ``gt`` (name -> gt rows or file, ``seq_lengths`` / ``benchmark`` as in
    ``evaluate_mot``) every config is scored: one evaluator handle, one run per config, because
    a run's COMBINED record is formed on the device over all the sequences of the run.

    ``score="device"`` scores all K configs in ONE evaluator run of K groups, straight from the
    feeder's result buffers in device memory (``SequenceFeeder.results_device``,
    ``MotEvaluator.set_gt`` / ``run_device``): the rows are neither copied to the host nor
    bucketed there, and the summaries are bit-identical to ``score="host"``'s.  It needs ``gt``
    to name the sequences in ``sequences``' order.  ``keep_results=False`` (with
    ``score="device"`` and gt, without ``exp_dir``) skips the copy of the rows altogether:
    ``"results"`` is None.  Combinations that cannot work raise ``ValueError`` before any engine
    is built.

    The detections are uploaded and held once per sequence, not once per config.  A nonzero
    engine or feeder status raises ``RuntimeError``.
    """
    return _run_sweep(_SPECS["sweep"], tracker_type, sequences, configs, exp_dir=exp_dir, gt=gt,
                      benchmark=benchmark, seq_lengths=seq_lengths, frame_ids=frame_ids,
                      frame_sizes=frame_sizes, score=score, keep_results=keep_results)


def _ocsort_engine(E, tracker_type, n_seq, F, resolved):
    p, tc, dc = resolved[0]
    return E.OcsortTableEngine(n_seq=n_seq, track_cap=tc, det_cap=dc, params=p), 0


def _ocsort_step(eng, tracker_type, feed_emb, run, warp):
    q0, ns, _, pd, po, _, pout, pcnt = run
    eng.step(pd, po, pout, pcnt, seq0=q0, nseq=ns)


def _frame_tables(names, seqs, frame_ids) -> tuple:
    """Per sequence the frame ids it iterates and its feeder table ``(row_start, row_cnt,
    frame_id)``."""
    fids = [np.asarray(frame_ids[nm]) if frame_ids and nm in frame_ids else s.frame_ids
            for nm, s in zip(names, seqs)]
    tables = []
    for s, f in zip(seqs, fids):
        start, cnt = np.zeros(len(f), np.int64), np.zeros(len(f), np.int64)
        for i, x in enumerate(f):
            j = s._index.get(int(x))
            if j is not None:
                start[i], cnt[i] = s.offsets[j], s.offsets[j + 1] - s.offsets[j]
        tables.append((start, cnt, np.asarray(f, np.int64)))
    return fids, tables


def _drive(eng, feed, step, K: int, gt, benchmark, seq_lengths, score, keep_results,
           post=None, after=None) -> tuple:
    """The frame loop both sweeps share: per frame index one gather, ``step(t, run)`` for each of
    its runs and one append; then the status checks, the device-side scores and the one copy of
    the rows.  Returns (rows per engine sequence or None, summaries per config or None).

    ``post`` (``sweep_gsi``'s (interval, tau)): the feeder's slots go through ``gsi_device`` once;
    its three tensors are what the device scores and what comes back as the rows.
    ``after``: called once after the frame loop, before any check (a flow's own errors)."""
    for t in range(feed.n_frames):
        runs = feed.schedule[t]
        if not runs:
            continue
        feed.gather(t)
        for run in runs:
            step(t, run)
        feed.append(t)
    if after is not None:
        after()
    if eng.status() != 0:
        raise RuntimeError(f"engine status {eng.status()} (capacity overflow)")
    summaries = None
    if post is not None:
        from .postprocessing import gsi_device

        if feed.status() != 0:
            raise RuntimeError(f"feeder status {feed.status()} (result buffer overflow)")
        res, base, n, _ = feed.results_device
        post = gsi_device(res, base, n, feed.n_seq, *post)
    if score == "device":
        if feed.status() != 0:
            raise RuntimeError(f"feeder status {feed.status()} (result buffer overflow)")
        summaries = _score_device(gt, feed, K, benchmark, seq_lengths, post)
    if not keep_results:
        return None, summaries
    if post is None:
        return feed.results(), summaries
    out, b, c = (x.cpu().numpy() for x in post)
    return [out[b[q]: b[q] + c[q]] for q in range(feed.n_seq)], summaries


def _gsi_host_rows(rows: list, post) -> list:
    """``sweep_gsi``'s post-stage for rows that were formed on the host (a StrongSort sweep with
    handle_occlusions): every engine sequence's rows as one slot of one ``gsi_device`` call."""
    import torch

    from .postprocessing import gsi_device

    n = np.array([r.shape[0] for r in rows], np.int64)
    base = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate([r.reshape(-1, 9) for r in rows]), np.float64)
    out, b, c = (x.cpu().numpy() for x in gsi_device(
        torch.from_numpy(flat).cuda(), torch.from_numpy(base).cuda(), torch.from_numpy(n).cuda(),
        None, *post))
    return [out[b[q]: b[q] + c[q]] for q in range(len(rows))]


def _report(configs, names, rows, summaries, exp_dir, gt, benchmark, seq_lengths,
            post=None) -> list:
    """One entry per config from the rows of engine sequences ``k*S + s``: the files under
    ``exp_dir``, and the host-side scores when the device did not score.  With ``post`` the rows
    are ``gsi_device``'s and the files are what ``postprocessing.gsi`` leaves: space-separated
    ``%d`` rows, and an empty file for a sequence without rows."""
    from . import motio
    from .postprocessing import MOT_FMT

    S = len(names)
    out = []
    for k, cfg in enumerate(configs):
        if rows is None:
            out.append({"config": cfg, "results": None, "summary": summaries[k]})
            continue
        res = {nm: rows[k * S + q].copy() for q, nm in enumerate(names)}
        if exp_dir is not None:
            for nm, r in res.items():
                p = Path(exp_dir) / f"{k:04d}" / f"{nm}.txt"
                if post is None or not r.size:
                    motio.write_mot_results(p, r if r.size else np.empty((0, 0)))
                else:
                    p.parent.mkdir(parents=True, exist_ok=True)
                    np.savetxt(p, r, fmt=MOT_FMT)
        out.append({"config": cfg, "results": res, "summary": None})
    if summaries is not None:
        for o, summary in zip(out, summaries):
            o["summary"] = summary
    elif gt is not None:
        for o, summary in zip(out, _score(gt, [o["results"] for o in out], benchmark,
                                          seq_lengths)):
            o["summary"] = summary
    return out


def _check_reid(tracker_type: str, configs, warps, score, keep_results) -> None:
    """The refusals of ``sweep_reid`` beyond ``_check``'s that need no engine and no device."""
    from . import motio

    if len({bool(c.get("embedding_off", False)) for c in configs}) > 1:
        raise ValueError("embedding_off decides the engine's embedding width and launches: it "
                         "must be the same in every config")
    for k, c in enumerate(configs):
        if tracker_type == "hybridsort" and c.get("use_byte"):
            raise NotImplementedError(
                f"config {k}: HybridSort(use_byte=True) is not built: the reference's BYTE round "
                "calls KalmanBoxTracker.update with the wrong arguments, so it defines no "
                "behaviour")
        if warps is not None:  # (cmc_off / use_ecc against warps)
            # hybridsort: one config with ECC=True takes the warps; the others run uncompensated
            # in the same engine (their switches are off).  None: run_sequences' refusal
            hyb = tracker_type == "hybridsort" and any(x.get("ECC") for x in configs)
            motio._check_warp_args(tracker_type, dict(c, ECC=True) if hyb else c, 0, warps, None,
                                   None)


def sweep_reid(tracker_type: str, sequences: dict, configs, *, exp_dir=None,
               gt: dict | None = None, benchmark: str = "MOT17", seq_lengths: dict | None = None,
               frame_ids: dict | None = None, frame_sizes: dict | None = None,
               score: str = "host", keep_results: bool = True, warps=None) -> list:
    """``sweep`` for the appearance trackers ``"deepocsort"`` and ``"hybridsort"``: every config of
    ``configs`` over every sequence in one ``DeepOcsortTableEngine`` / ``HybridsortTableEngine``
    of K*S sequences, engine sequence ``k*S + s`` being sequence ``s`` under config ``k``.

    Arguments, return value, scoring and ``keep_results`` as in ``sweep``; each config means what
    ``run_sequences(tracker_type, ..., tracker_kwargs=cfg, resident=True)`` makes of it, and the
    files under ``exp_dir/<k as 4 digits>/`` are byte-identical to that run's.  The sequences are
    fed by one ``SharedSequenceFeeder`` with ``source[k*S + s] = s``: detections and embeddings
    are uploaded and held once per sequence, not once per config.

    ``warps`` (deepocsort, and hybridsort when at least one config sets ``ECC=True``: configs
    without it run uncompensated in the same engine): what ``run_sequences(warps=...)`` takes, a
    ``cmc.WarpTable`` over
    these sequences or a mapping name -> ``[n_frames, 6]``; rounded to float32 as there, and every
    config's copy of a sequence gets that sequence's warp (the ``[T, K*S, 6]`` table is built once
    on the device).  ``cmc.sof_warp_table(images, stepped, sof=SOF(...))`` returns such a table:
    with it the sweep runs the reference's default DeepOCSort, whose camera-motion estimator is
    sparse optical flow.

    Raised before any engine is built: ``NotImplementedError`` for another tracker, ``per_class``
    in a config or HybridSort's ``use_byte=True``; ``ValueError`` for caps or ``embedding_off``
    that differ across configs, ``warps`` with hybridsort when no config sets ``ECC=True`` or with
    a config that switches the
    camera-motion compensation off (``cmc_off`` / ``use_ecc``), sequences whose embedding widths
    differ, and the ``score`` / ``keep_results`` combinations ``sweep`` refuses.
    """
    return _run_sweep(_SPECS["sweep_reid"], tracker_type, sequences, configs, exp_dir=exp_dir,
                      gt=gt, benchmark=benchmark, seq_lengths=seq_lengths, frame_ids=frame_ids,
                      frame_sizes=frame_sizes, score=score, keep_results=keep_results,
                      warps=warps)


def _reid_engine(E, tracker_type, n_seq, F, resolved):
    p, tc, dc = resolved[0]
    cls = E.DeepOcsortTableEngine if tracker_type == "deepocsort" else E.HybridsortTableEngine
    if tracker_type == "hybridsort" and any(getattr(r[0], "ECC", False) for r in resolved):
        cls = E.HybridsortCmcTableEngine  # (a config switches the camera update on)
    eng = cls(n_seq=n_seq, track_cap=tc, det_cap=dc, emb_dim=F or 1, params=p)
    return eng, F if eng.emb_dim else 0


def _reid_step(eng, tracker_type, feed_emb, run, warp):
    from . import motio

    q0, ns, _, pd, po, pe, pout, pcnt = run
    motio._step(eng, tracker_type, pd, po, pe, pout, pcnt, q0, ns, warp)


def _emb_step(eng, tracker_type, feed_emb, run, warp):
    """The step of the engines that take (embeddings or None, warps or None): bx_engine's,
    BoostTrack's and StrongSort's."""
    q0, ns, _, pd, po, pe, pout, pcnt = run
    eng.step(pd, po, pe if feed_emb else None, warp, pout, pcnt, seq0=q0, nseq=ns)


def _check_bot(tracker_type: str, configs, warps, score, keep_results) -> None:
    """The refusals of ``sweep_bot`` beyond ``_check``'s that need no engine and no device."""
    from . import motio

    if len({bool(c.get("with_reid", True)) for c in configs}) > 1:
        raise ValueError("with_reid decides the engine's embedding width and launches: it must "
                         "be absent from every config or equal in all of them")
    if warps is not None:
        for c in configs:  # (bytetrack against warps)
            motio._check_warp_args(tracker_type, c, 0, warps, None, None)


def sweep_bot(tracker_type: str, sequences: dict, configs, *, exp_dir=None,
              gt: dict | None = None, benchmark: str = "MOT17", seq_lengths: dict | None = None,
              frame_ids: dict | None = None, score: str = "host", keep_results: bool = True,
              warps=None) -> list:
    """``sweep`` for ``"bytetrack"`` and ``"botsort"``: every config of ``configs`` over every
    sequence in one ``engine.TableEngine`` of K*S sequences, engine sequence ``k*S + s`` being
    sequence ``s`` under config ``k``.

    Arguments, return value, scoring and ``keep_results`` as in ``sweep``; each config means what
    ``run_sequences(tracker_type, ..., tracker_kwargs=cfg)`` makes of it, and the files under
    ``exp_dir/<k as 4 digits>/`` are byte-identical to that run's.  The sequences are fed by one
    ``SharedSequenceFeeder`` with ``source[k*S + s] = s``: detections and (BoT-SORT with ReID)
    float64 embeddings are uploaded and held once per sequence, not once per config.

    ``warps`` (botsort only): what ``run_sequences(warps=...)`` takes, a ``cmc.WarpTable`` over
    these sequences (``cmc.warp_table`` / ``cmc.sof_warp_table`` return one) or a mapping name ->
    ``[n_frames, 6]``; rounded to float32 as there, and every config's copy of a sequence gets
    that sequence's warp.

    Raised before any engine is built: ``NotImplementedError`` for another tracker or
    ``per_class`` in a config; ``ValueError`` for caps or ``with_reid`` that differ across
    configs, ``warps`` with bytetrack, sequences whose embedding widths differ, and the ``score``
    / ``keep_results`` combinations ``sweep`` refuses.
    """
    return _run_sweep(_SPECS["sweep_bot"], tracker_type, sequences, configs, exp_dir=exp_dir,
                      gt=gt, benchmark=benchmark, seq_lengths=seq_lengths, frame_ids=frame_ids,
                      score=score, keep_results=keep_results, warps=warps)


def _bot_engine(E, tracker_type, n_seq, F, resolved):
    p, tc, dc = resolved[0]
    feed_emb = F if tracker_type == "botsort" and p.with_reid else 0
    return E.TableEngine(tracker_type, n_seq=n_seq, track_cap=tc, det_cap=dc, emb_dim=feed_emb,
                         emb_f64=True, params=p), feed_emb


def _boost_reid(cfg: dict) -> bool:
    """with_reid as run_sequences("boosttrack", tracker_kwargs=cfg) resolves it: the YAML default
    (on) for an empty cfg, else the constructor's (off) under cfg."""
    return bool(cfg.get("with_reid", False)) if cfg else True


def _check_boost(tracker_type: str, configs, warps, score, keep_results) -> None:
    """The refusals of ``sweep_boost`` beyond ``_check``'s that need no engine and no device."""
    from . import motio

    if len({_boost_reid(c) for c in configs}) > 1:
        raise ValueError("with_reid decides the engine's embedding width and launches: it must "
                         "resolve to the same value in every config")
    if warps is not None:
        for c in configs:  # (use_ecc=False against warps)
            motio._check_warp_args(tracker_type, c, 0, warps, None, None)


def sweep_boost(sequences: dict, configs, *, exp_dir=None, gt: dict | None = None,
                benchmark: str = "MOT17", seq_lengths: dict | None = None,
                frame_ids: dict | None = None, score: str = "host", keep_results: bool = True,
                warps=None) -> list:
    """``sweep`` for BoostTrack: every config of ``configs`` over every sequence in one
    ``engine.BoostTableEngine`` of K*S sequences, engine sequence ``k*S + s`` being sequence ``s``
    under config ``k``.  The variants of the BoostTrack paper (BoostTrack, BoostTrack+,
    BoostTrack++) are configs: they differ in ``use_rich_s``, ``use_sb``, ``use_vt``,
    ``use_dlo_boost``, ``use_duo_boost`` and ``s_sim_corr`` only.

    Arguments, return value, scoring and ``keep_results`` as in ``sweep``; each config means what
    ``run_sequences("boosttrack", ..., tracker_kwargs=cfg)`` makes of it (an empty dict is the
    YAML's BoostTrack++ with ReID, a non-empty one goes through the drop-in's constructor), and
    the files under ``exp_dir/<k as 4 digits>/`` are byte-identical to that run's.  The sequences
    are fed by one ``SharedSequenceFeeder`` with ``source[k*S + s] = s``: detections and (with
    ReID) float64 embeddings are uploaded and held once per sequence, not once per config.

    ``warps``: what ``run_sequences(warps=...)`` takes, a ``cmc.WarpTable`` over these sequences
    (``cmc.warp_table`` / ``cmc.sof_warp_table`` return one) or a mapping name ->
    ``[n_frames, 6]``; rounded to float32 as there, and every config's copy of a sequence gets
    that sequence's warp.

    Raised before any engine is built: ``NotImplementedError`` for ``per_class`` in a config;
    ``ValueError`` for caps or ``with_reid`` that differ across configs, ``warps`` with a config
    that switches ``use_ecc`` off, sequences whose embedding widths differ, and the ``score`` /
    ``gt`` / ``keep_results`` combinations ``sweep`` refuses.
    """
    return _run_sweep(_SPECS["sweep_boost"], "boosttrack", sequences, configs, exp_dir=exp_dir,
                      gt=gt, benchmark=benchmark, seq_lengths=seq_lengths, frame_ids=frame_ids,
                      score=score, keep_results=keep_results, warps=warps)


def _boost_engine(E, tracker_type, n_seq, F, resolved):
    params = [r[0] for r in resolved]
    if len({bool(p.with_reid) for p in params}) > 1:  # (what _check_boost's reading missed)
        raise ValueError("with_reid resolves differently across the configs: "
                         f"{[bool(p.with_reid) for p in params]}")
    feed_emb = F if params[0].with_reid else 0
    return E.BoostTableEngine(n_seq=n_seq, track_cap=resolved[0][1], det_cap=resolved[0][2],
                              emb_dim=feed_emb, params=params[0]), feed_emb


def _strong_occ(cfg: dict) -> bool:
    """handle_occlusions as run_sequences("strongsort", tracker_kwargs=cfg) resolves it: on, the
    reference's default, unless cfg switches it off."""
    return bool(cfg.get("handle_occlusions", True))


def _check_strong(tracker_type: str, configs, warps, score, keep_results,
                  occlusion="host") -> None:
    """The refusals of ``sweep_strong`` beyond ``_check``'s that need no engine and no device."""
    from . import motio

    motio.check_occlusion(tracker_type, occlusion)
    if len({repr(c.get("vec_cap")) for c in configs}) > 1:
        raise ValueError("vec_cap sizes the engine's memory: it must be absent from every config "
                         "or equal in all of them")
    occ = set() if occlusion == "device" else {_strong_occ(c) for c in configs}
    if len(occ) > 1:
        raise ValueError("handle_occlusions is a setting of the sweep, not of a config: it must "
                         "resolve to the same value in every config")
    if True in occ and score == "device":
        raise ValueError('score="device" reads rows appended on the device; with '
                         "handle_occlusions the rows are edited on the host: use "
                         'score="host", or handle_occlusions=False in every config')
    if True in occ and not keep_results:
        raise ValueError("keep_results=False needs the rows on the device; with "
                         "handle_occlusions they are formed on the host")
    if warps is not None:
        for c in configs:  # (cmc_off / use_ecc=False against warps)
            motio._check_warp_args(tracker_type, c, 0, warps, None, None)


def sweep_strong(sequences: dict, configs, *, exp_dir=None, gt: dict | None = None,
                 benchmark: str = "MOT17", seq_lengths: dict | None = None,
                 frame_ids: dict | None = None, score: str = "host", keep_results: bool = True,
                 warps=None) -> list:
    """``sweep`` for StrongSort: every config of ``configs`` over every sequence in one
    ``engine.SsTableEngine`` of K*S sequences, engine sequence ``k*S + s`` being sequence ``s``
    under config ``k``.

    Arguments, return value, scoring and ``keep_results`` as in ``sweep``; each config means what
    ``run_sequences("strongsort", ..., tracker_kwargs=cfg)`` makes of it, and the files under
    ``exp_dir/<k as 4 digits>/`` are byte-identical to that run's with the same ``warps``.  The
    sequences are fed by one ``SharedSequenceFeeder`` with ``source[k*S + s] = s`` in its float64 /
    10-column mode: detections (held as float32, which ``BinSequence``'s values are widened from
    exactly as ``run_sequences`` widens them) and float64 embeddings are uploaded and held once
    per sequence, not once per config.  The engine's own ``nn_budget``, which sizes the galleries,
    is the largest of the configs'.

    ``handle_occlusions`` is a setting of the sweep: it must resolve to the same value in every
    config.  Off, the rows are appended on the device and ``score="device"`` is available.  On
    (the reference's default, and what an empty config means) the feeder still gathers and the
    one engine still steps, but after each frame index the runs' rows come back to the host, an
    ``OcclusionHandler`` per engine sequence (with its config's ``occlusion_threshold``) edits
    tracks and rows as in ``run_sequences``, and the host formatter makes the MOT rows;
    ``score="device"`` and ``keep_results=False`` are refused then.  The handler's ``TypeError``
    on mutual occlusion propagates.

    ``sweep_strong_device`` is this sweep with the occlusion handling in the engine instead
    (its signature is this one's plus ``occlusion``; this one's is pinned).

    ``warps``: what ``run_sequences(warps=...)`` takes; every config's copy of a sequence gets that
    sequence's warp.

    Raised before any engine is built: ``NotImplementedError`` for ``per_class`` in a config;
    ``ValueError`` for ``track_cap``, ``det_cap`` or ``vec_cap`` that differ across configs, mixed
    ``handle_occlusions``, ``warps`` with a config that switches the camera-motion compensation
    off, sequences whose embedding widths differ or whose detections are not float32 values (the
    feeder holds float32, ``run_sequences`` feeds StrongSort float64: pack such a sequence from
    detections rounded to float32, e.g. ``dets.astype(np.float32)``), and the ``score`` / ``gt`` /
    ``keep_results`` combinations ``sweep`` refuses.
    """
    return _run_sweep(_SPECS["sweep_strong"], "strongsort", sequences, configs, exp_dir=exp_dir,
                      gt=gt, benchmark=benchmark, seq_lengths=seq_lengths, frame_ids=frame_ids,
                      score=score, keep_results=keep_results, warps=warps)


def sweep_strong_device(sequences: dict, configs, *, exp_dir=None, gt: dict | None = None,
                        benchmark: str = "MOT17", seq_lengths: dict | None = None,
                        frame_ids: dict | None = None, score: str = "host",
                        keep_results: bool = True, warps=None,
                        occlusion: str = "device") -> list:
    """``sweep_strong`` with an ``occlusion`` argument (``sweep_strong`` itself keeps its
    signature).  ``"host"`` is ``sweep_strong``, refusals included.  ``"device"``: the engine's
    occlusion pass (``SsTableEngine.set_occlusion``) ends every frame, and no
    ``OcclusionHandler`` is built; each engine sequence gets its config's ``handle_occlusions``
    and ``occlusion_threshold``, so configs may differ in ``handle_occlusions``, the rows are
    appended on the device, ``score="device"`` and ``keep_results=False`` are accepted, and the
    files are byte-identical to the host flow's.  A mutual occlusion raises the reference's
    ``TypeError`` after the frame loop, naming the sequence and its update count, before anything
    is scored or written; a full buffer pool is a ``RuntimeError`` naming ``occ_cap``.
    ``sweep_gsi("strongsort", ..., occlusion="device")`` passes the argument through."""
    return _run_sweep(_SPECS["sweep_strong"], "strongsort", sequences, configs, exp_dir=exp_dir,
                      gt=gt, benchmark=benchmark, seq_lengths=seq_lengths, frame_ids=frame_ids,
                      score=score, keep_results=keep_results, warps=warps, occlusion=occlusion)


def _strong_seq_check(seqs, widths, dets) -> None:
    if len(widths) > 1 or not widths[0]:
        raise ValueError(f"StrongSort needs embeddings of one width in every sequence (got "
                         f"{widths}): one engine has one emb_dim")
    for s, d in zip(seqs, dets):
        if not np.array_equal(d.astype(np.float64), np.asarray(s.dets)):
            raise ValueError(f"{s.path}: detections that are not float32 values cannot be "
                             "held once as float32 (run_sequences feeds them as float64): "
                             "pack the sequence from detections rounded to float32")


def _strong_engine(E, tracker_type, n_seq, F, resolved, occlusion="host"):
    """``resolved``: per config (SsParams, track_cap, det_cap, vec_cap, occlusion_threshold or
    None).  The engine's own nn_budget, which sizes the galleries, is the configs' largest."""
    params = [r[0] for r in resolved]
    if len({r[1:4] for r in resolved}) > 1 or (
            occlusion != "device" and len({r[4] is None for r in resolved}) > 1):
        raise ValueError("the configs resolve to different capacities or handle_occlusions: "
                         f"{[r[1:] for r in resolved]}")
    base = dataclasses.replace(params[0], nn_budget=max(int(p.nn_budget) for p in params))
    return E.SsTableEngine(n_seq=n_seq, track_cap=resolved[0][1], det_cap=resolved[0][2],
                           emb_dim=F, vec_cap=resolved[0][3], params=base), F


def _strong_drive(eng, feed, step, tail, resolved, names, fids, tables, occlusion="host"):
    """StrongSort's frame loop.  Without handle_occlusions, or with the engine's own occlusion
    pass (each engine sequence with its config's settings), ``_drive``; else ``_drive_occlusion``
    with each config's threshold, and ``sweep_gsi``'s post-stage on its host rows."""
    from . import motio

    S, K, post = len(names), tail[0], tail[-1]
    occ_thr = [r[4] for r in resolved]
    after = None
    if occlusion == "device" and any(t is not None for t in occ_thr):
        for k in range(K):
            eng.set_occlusion(k * S, occ_thr[k] is not None,
                              0.3 if occ_thr[k] is None else occ_thr[k], nseq=S)
        after = lambda: motio.raise_device_occlusion(eng, names)  # noqa: E731
    if occlusion == "device" or occ_thr[0] is None:
        return _drive(eng, feed, step, *tail, after)
    rows = _drive_occlusion(eng, feed, step, fids * K, [tb[1] for tb in tables] * K,
                            [t for t in occ_thr for _ in range(S)])
    return (rows if post is None else _gsi_host_rows(rows, post)), None


def _drive_occlusion(eng, feed, step, fids, feed_cnt, thresholds) -> list:
    """``_drive`` for a StrongSort sweep with handle_occlusions: per frame index one gather and
    the steps of its runs, then the runs' out / out_count back on the host, the occlusion
    post-process of every stepped sequence (with its update count, as run_sequences calls it)
    and the host formatter.  ``feed_cnt[q][t]``: detections of engine sequence q at frame index
    t.  Returns each engine sequence's MOT rows [n, 9]."""
    import torch

    from . import motio
    from .occlusion import OcclusionHandler

    occ = [OcclusionHandler(eng, q, thr) for q, thr in enumerate(thresholds)]
    nupd = [0] * feed.n_seq
    results = [[] for _ in range(feed.n_seq)]
    dev = torch.device("cuda")
    for t in range(feed.n_frames):
        runs = feed.schedule[t]
        if not runs:
            continue
        feed.gather(t)
        outs = []
        for run in runs:  # the rows go to tensors of this frame index, which the host reads
            out = torch.empty((run[2], 10), dtype=torch.float64, device=dev)
            cnt = torch.empty(run[1], dtype=torch.int32, device=dev)
            step(t, (*run[:6], out, cnt))
            outs.append((out, cnt))
        # every run is stepped before a handler edits the engine: a handler touches its own
        # sequence alone, and the next frame index is stepped after all of them
        for (q0, ns, *_), (out, cnt) in zip(runs, outs):
            o, c = out.cpu().numpy(), cnt.cpu().numpy()
            r0 = 0
            for q in range(q0, q0 + ns):
                rows = o[r0: r0 + c[q - q0]]
                r0 += int(feed_cnt[q][t])  # (the sequence's detections: its det_off step)
                nupd[q] += 1
                rows = occ[q](nupd[q], rows)
                if rows.shape[0]:
                    results[q].append(motio.convert_to_mot_format(rows, int(fids[q][t])))
    if eng.status() != 0:
        raise RuntimeError(f"engine status {eng.status()} (capacity overflow)")
    return [np.vstack(r) if r else np.empty((0, 9)) for r in results]


GSI_MAX_INTERVAL = 22
# tracker -> the public sweep sweep_gsi runs for it (its keyword arguments, its implementation)
GSI_DISPATCH = {"ocsort": "sweep", "deepocsort": "sweep_reid", "hybridsort": "sweep_reid",
                "bytetrack": "sweep_bot", "botsort": "sweep_bot", "boosttrack": "sweep_boost",
                "strongsort": "sweep_strong"}


def sweep_gsi(tracker_type: str, sequences: dict, configs, *, interval: int = 20,
              tau: float = 10, **sweep_kwargs) -> list:
    """The sweep of ``tracker_type`` with GSI (``postprocessing.gsi``: tracklet interpolation and
    Gaussian smoothing, the reference's ``val.py --gsi``) applied to every config's rows before
    they are scored, returned or written: the flow track -> GSI -> evaluate, per config, in one
    engine, one ``gsi_device`` call and one evaluator run.

    ``tracker_type`` chooses the sweep (``GSI_DISPATCH``): ocsort -> ``sweep``; deepocsort,
    hybridsort -> ``sweep_reid``; bytetrack, botsort -> ``sweep_bot``; boosttrack ->
    ``sweep_boost``; strongsort -> ``sweep_strong``.  ``sweep_kwargs`` are that sweep's own keyword
    arguments (``exp_dir``, ``gt``, ``score``, ``keep_results``, ``warps``, ...), with its meaning
    and its refusals, raised before any engine is built.

    Per config ``k``, ``results[name]`` is ``[n, 9]`` float64 with whole-number values, ids
    ascending and frames ascending within an id: what ``np.loadtxt`` reads from the file
    ``postprocessing.gsi`` leaves.  With ``exp_dir``, ``exp_dir/<k as 4 digits>/<name>.txt`` is
    byte-identical to what the plain sweep writes there followed by ``gsi(exp_dir/<k as 4
    digits>, interval, tau)``: space-separated ``%d`` rows, and a sequence without rows keeps its
    empty file.  ``gsi`` globs ``MOT*.txt`` only; ``sweep_gsi`` treats EVERY sequence, whatever
    its name.  ``score="host"`` evaluates those arrays; ``score="device"`` runs ``gsi_device`` on
    the feeder's result slots and scores its tensors in one evaluator run of K groups, with
    ``keep_results=False`` without copying a row to the host; the summaries are bit-identical.
    A ``LinAlgError`` of the smoothing propagates.

    ``interval`` must not exceed 22 (``ValueError``): the reference computes an inserted row's
    frame as ``prev + (cur - prev) * (i / (cur - prev))`` in float64, which is a whole number for
    every gap up to 21 (every ``prev`` in 1..3999 checked) but not from a gap of 22 on (first at
    i = 15); ``%d`` truncates such a frame to the one before it, the id then stands twice in a
    frame, and the evaluator refuses the rows.
    """
    if tracker_type not in GSI_DISPATCH:
        raise NotImplementedError(
            f"tune.sweep_gsi drives {', '.join(GSI_DISPATCH)} (the trackers with a sweep), not "
            f"{tracker_type}")
    if int(interval) > GSI_MAX_INTERVAL:
        raise ValueError(
            f"interval must not exceed {GSI_MAX_INTERVAL}, got {interval}: from a gap of 22 "
            "frames on, the reference's prev + (cur - prev) * (i / (cur - prev)) is not a whole "
            "number for every inserted frame, so after %d an id can stand twice in a frame, "
            "which the evaluator refuses")
    spec = _SPECS[GSI_DISPATCH[tracker_type]]
    for k in sweep_kwargs:
        if k not in spec.keywords:
            raise TypeError(f"tune.{spec.name}() got an unexpected keyword argument {k!r}")
    # the public sweep's defaults under the caller's keywords
    return _run_sweep(spec, tracker_type, sequences, configs, (int(interval), float(tau)),
                      **{**_PUBLIC[spec.name].__kwdefaults__, **sweep_kwargs})


_SPECS = {s.name: s for s in (
    _Spec("sweep", SUPPORTED, _ocsort_engine, _ocsort_step, embeddings=False, frame_sizes=True,
          warps=False),
    _Spec("sweep_reid", SUPPORTED_REID, _reid_engine, _reid_step, _check_reid, frame_sizes=True),
    _Spec("sweep_bot", SUPPORTED_BOT, _bot_engine, _emb_step, _check_bot),
    _Spec("sweep_boost", SUPPORTED_BOOST, _boost_engine, _emb_step, _check_boost),
    _Spec("sweep_strong", SUPPORTED_STRONG, _strong_engine, _emb_step, _check_strong,
          feeder_kw=dict(det_f64=True, out_cols=10),
          resolve_more=("vec_cap", "occlusion_threshold"), seq_check=_strong_seq_check,
          drive=_strong_drive, extra=("occlusion",)),
)}
_PUBLIC = {"sweep": sweep, "sweep_reid": sweep_reid, "sweep_bot": sweep_bot,
           "sweep_boost": sweep_boost, "sweep_strong": sweep_strong}


def _score(gt: dict, results: list, benchmark: str, seq_lengths) -> list:
    """mot_summary of every config's results, as ``evaluate_mot(gt, results_k)`` gives it: the
    gt is parsed once, and one evaluator handle runs once per config."""
    from . import evaluation as E

    if benchmark not in E.BENCHMARKS:
        raise ValueError(f"benchmark must be one of {sorted(E.BENCHMARKS)}, got {benchmark!r}")
    if "COMBINED" in gt:
        raise ValueError("a sequence cannot be called COMBINED")
    names, frames, gts, _ = E.prepare_inputs(gt, results[0], seq_lengths)
    parsed = dict(zip(names, gts))
    summaries = []
    ev = E.MotEvaluator()
    try:
        for res in results:
            trs = E.prepare_inputs(parsed, res, seq_lengths)[3]
            rec = ev.run(frames, gts, trs, E.BENCHMARKS[benchmark])
            full = {n: E._unpack(rec[k], E.METRICS) for k, n in enumerate(names)}
            full["COMBINED"] = E._unpack(rec[len(names)], E.METRICS)
            summaries.append(E.mot_summary(full))
    finally:
        ev.close()
    return summaries


def _score_device(gt: dict, feed, n_groups: int, benchmark: str, seq_lengths,
                  post=None) -> list:
    """mot_summary of every config from the feeder's device-resident rows: the gt is bucketed
    and uploaded once, and ONE evaluator run of ``n_groups`` groups forms every COMBINED.
    ``post``: None, or ``gsi_device``'s three tensors, scored in place of the feeder's slots."""
    from . import evaluation as E

    if benchmark not in E.BENCHMARKS:
        raise ValueError(f"benchmark must be one of {sorted(E.BENCHMARKS)}, got {benchmark!r}")
    if "COMBINED" in gt:
        raise ValueError("a sequence cannot be called COMBINED")
    names, frames, gts, _ = E.prepare_inputs(gt, {}, seq_lengths)
    res, base, n = feed.results_device[:3] if post is None else post
    ev = E.MotEvaluator()
    try:
        ev.set_gt(frames, gts)
        rec = ev.run_device(res, base, n, n_groups, E.BENCHMARKS[benchmark], row_stride=9)
    finally:
        ev.close()
    summaries = []
    for r in rec:
        full = {nm: E._unpack(r[k], E.METRICS) for k, nm in enumerate(names)}
        full["COMBINED"] = E._unpack(r[len(names)], E.METRICS)
        summaries.append(E.mot_summary(full))
    return summaries

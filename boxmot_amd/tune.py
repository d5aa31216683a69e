"""Hyper-parameter sweeps on the batched engine: K configurations x S sequences as ONE engine.

Reference stage replaced (``boxmot/engine/evolve.py``): its objective function runs the tracker
over all sequences with one configuration and evaluates, once per trial.  Here the K
configurations of a sweep run together: an ``OcsortTableEngine`` of K*S sequences is built, engine
sequence ``k*S + s`` is sequence ``s`` under configuration ``k`` (``set_seq_params``,
include/bxocsort.h), and every frame index is one K*S-wide launch fed from device memory
(``engine.SequenceFeeder``, include/bxfeed.h).  The search strategy (which configurations to try)
stays with the caller; ``grid`` builds the cartesian product of a search space.

Three engines have per-sequence parameters: OCSort (``sweep``; DESIGN.md 2.18 is the contract) and
the two appearance trackers of its family, DeepOCSort and HybridSort (``sweep_reid``; DESIGN.md
2.20), whose K*S sequences read each sequence's detections and embeddings from ONE copy in device
memory (``engine.SharedSequenceFeeder``).  ByteTrack and BoT-SORT, which share ``bx_engine``, have
them too (``sweep_bot``), fed the same way, and so has BoostTrack
(``sweep_boost``), whose variants differ in constructor flags only.  StrongSort
(``sweep_strong``) completes the set: its feeder gathers float64 detections and
10-column rows, and its occlusion post-process stays on the host, per sweep, unless
``occlusion="device"`` asks for the engine's own pass.

``sweep_gsi`` runs any of the five with GSI between tracking and scoring, on the
feeder's result slots in device memory (``postprocessing.gsi_device``, include/bxgsi.h).
"""
from __future__ import annotations

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


def _resolve(cfg: dict):
    """(OcsortParams, track_cap, det_cap) of one config, resolved as run_sequences resolves its
    tracker_kwargs: through ``motio._batched_engine`` itself, on a one-sequence engine."""
    from . import motio

    eng = motio._batched_engine("ocsort", 1, 0, cfg)[0]
    try:
        return eng.params, eng.track_cap, eng.det_cap
    finally:
        eng.close()


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

    The detections are uploaded once per (config, sequence): K copies of a few MB for MOT-sized
    inputs.  A nonzero engine or feeder status raises ``RuntimeError``.
    """
    return _sweep(tracker_type, sequences, configs, None, exp_dir=exp_dir, gt=gt,
                  benchmark=benchmark, seq_lengths=seq_lengths, frame_ids=frame_ids,
                  frame_sizes=frame_sizes, score=score, keep_results=keep_results)


def _sweep(tracker_type, sequences, configs, post, *, exp_dir, gt, benchmark, seq_lengths,
           frame_ids, frame_sizes, score, keep_results) -> list:
    """``sweep``; ``post``: None, or ``sweep_gsi``'s (interval, tau)."""
    configs = _check(tracker_type, configs, sequences, gt, exp_dir, score, keep_results)
    from . import motio
    from .engine import OcsortTableEngine, SequenceFeeder

    names = list(sequences)
    seqs = [s if isinstance(s, motio.BinSequence) else motio.BinSequence(s)
            for s in sequences.values()]
    S, K = len(seqs), len(configs)
    if not S:
        return [{"config": c, "results": {} if keep_results else None, "summary": None}
                for c in configs]
    resolved = [_resolve(c) for c in configs]
    params = [r[0] for r in resolved]
    eng = OcsortTableEngine(n_seq=K * S, track_cap=resolved[0][1], det_cap=resolved[0][2],
                       params=params[0])
    feed = None
    try:
        fids, tables = _frame_tables(names, seqs, frame_ids)
        dets = [np.asarray(s.dets).astype(np.float32) for s in seqs]
        for k in range(K):
            eng.set_seq_params(k * S, [params[k]] * S)
            for q, nm in enumerate(names):
                if frame_sizes and nm in frame_sizes:
                    eng.set_frame_size(k * S + q, *frame_sizes[nm])
        feed = SequenceFeeder(dets * K, [None] * (K * S), tables * K, 0)

        def step(t, run):
            q0, ns, _, pd, po, _, pout, pcnt = run
            eng.step(pd, po, pout, pcnt, seq0=q0, nseq=ns)

        rows, summaries = _drive(eng, feed, step, K, gt, benchmark, seq_lengths, score,
                                 keep_results, post)
    finally:
        if feed is not None:
            feed.close()
        eng.close()
    return _report(configs, names, rows, summaries, exp_dir, gt, benchmark, seq_lengths, post)


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


def _check_reid(tracker_type: str, configs, sequences, gt, exp_dir, score, keep_results,
                warps) -> list:
    """The refusals of ``sweep_reid`` that need no engine and no device."""
    from . import motio

    configs = _check(tracker_type, configs, sequences, gt, exp_dir, score, keep_results,
                     supported=SUPPORTED_REID, what="tune.sweep_reid")
    if len({bool(c.get("embedding_off", False)) for c in configs}) > 1:
        raise ValueError("embedding_off decides the engine's embedding width and launches: it "
                         "must be the same in every config")
    for k, c in enumerate(configs):
        if tracker_type == "hybridsort" and c.get("use_byte"):
            raise NotImplementedError(
                f"config {k}: HybridSort(use_byte=True) is not built: the reference's BYTE round "
                "calls KalmanBoxTracker.update with the wrong arguments, so it defines no "
                "behaviour")
        if warps is not None:  # (hybridsort, cmc_off / use_ecc against warps)
            motio._check_warp_args(tracker_type, c, 0, warps, None, None)
    return configs


def _resolve_reid(tracker_type: str, F: int, cfg: dict):
    """(params, track_cap, det_cap) of one config, resolved as run_sequences resolves its
    tracker_kwargs: through ``motio._batched_engine`` itself, on a one-sequence engine."""
    from . import motio

    eng = motio._batched_engine(tracker_type, 1, F, cfg)[0]
    try:
        return eng.params, eng.track_cap, eng.det_cap
    finally:
        eng.close()


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

    ``warps`` (deepocsort only): what ``run_sequences(warps=...)`` takes, a ``cmc.WarpTable`` over
    these sequences or a mapping name -> ``[n_frames, 6]``; rounded to float32 as there, and every
    config's copy of a sequence gets that sequence's warp (the ``[T, K*S, 6]`` table is built once
    on the device).  ``cmc.sof_warp_table(images, stepped, sof=SOF(...))`` returns such a table:
    with it the sweep runs the reference's default DeepOCSort, whose camera-motion estimator is
    sparse optical flow.

    Raised before any engine is built: ``NotImplementedError`` for another tracker, ``per_class``
    in a config or HybridSort's ``use_byte=True``; ``ValueError`` for caps or ``embedding_off``
    that differ across configs, ``warps`` with hybridsort or with a config that switches the
    camera-motion compensation off (``cmc_off`` / ``use_ecc``), sequences whose embedding widths
    differ, and the ``score`` / ``keep_results`` combinations ``sweep`` refuses.
    """
    return _sweep_reid(tracker_type, sequences, configs, None, exp_dir=exp_dir, gt=gt,
                       benchmark=benchmark, seq_lengths=seq_lengths, frame_ids=frame_ids,
                       frame_sizes=frame_sizes, score=score, keep_results=keep_results,
                       warps=warps)


def _sweep_reid(tracker_type, sequences, configs, post, *, exp_dir, gt, benchmark, seq_lengths,
                frame_ids, frame_sizes, score, keep_results, warps) -> list:
    """``sweep_reid``; ``post``: None, or ``sweep_gsi``'s (interval, tau)."""
    configs = _check_reid(tracker_type, configs, sequences, gt, exp_dir, score, keep_results,
                          warps)
    from . import motio
    from . import engine as E

    names = list(sequences)
    seqs = [s if isinstance(s, motio.BinSequence) else motio.BinSequence(s)
            for s in sequences.values()]
    S, K = len(seqs), len(configs)
    if not S:
        return [{"config": c, "results": {} if keep_results else None, "summary": None}
                for c in configs]
    widths = sorted({int(s.emb_dim) for s in seqs})
    if len(widths) > 1:
        raise ValueError(f"the sequences' embedding widths differ ({widths}): one engine has one "
                         "emb_dim")
    F = widths[0]
    fids, tables = _frame_tables(names, seqs, frame_ids)
    table = None
    if warps is not None:  # [T, S, 6] as run_sequences builds it, then every config's copy
        table = motio._flow_warps(names, seqs, fids, F, warps, None, None).repeat(1, K, 1)
    resolved = [_resolve_reid(tracker_type, F, c) for c in configs]
    params = [r[0] for r in resolved]
    cls = E.DeepOcsortTableEngine if tracker_type == "deepocsort" else E.HybridsortTableEngine
    eng = cls(n_seq=K * S, track_cap=resolved[0][1], det_cap=resolved[0][2], emb_dim=F or 1,
              params=params[0])
    feed = None
    try:
        feed_emb = F if eng.emb_dim else 0
        dets = [np.asarray(s.dets).astype(np.float32) for s in seqs]
        embs = [s.embs if feed_emb else None for s in seqs]
        for k in range(K):
            eng.set_seq_params(k * S, [params[k]] * S)
            for q, nm in enumerate(names):
                if frame_sizes and nm in frame_sizes:
                    eng.set_frame_size(k * S + q, *frame_sizes[nm])
        none = [None] * ((K - 1) * S)
        feed = E.SharedSequenceFeeder(dets + none, embs + none, tables * K, feed_emb,
                                      source=list(range(S)) * K)

        def step(t, run):
            q0, ns, _, pd, po, pe, pout, pcnt = run
            motio._step(eng, tracker_type, pd, po, pe, pout, pcnt, q0, ns,
                        None if table is None else table[t, q0: q0 + ns])

        rows, summaries = _drive(eng, feed, step, K, gt, benchmark, seq_lengths, score,
                                 keep_results, post)
    finally:
        if feed is not None:
            feed.close()
        eng.close()
    return _report(configs, names, rows, summaries, exp_dir, gt, benchmark, seq_lengths, post)


def _check_bot(tracker_type: str, configs, sequences, gt, exp_dir, score, keep_results,
               warps) -> list:
    """The refusals of ``sweep_bot`` that need no engine and no device."""
    from . import motio

    configs = _check(tracker_type, configs, sequences, gt, exp_dir, score, keep_results,
                     supported=SUPPORTED_BOT, what="tune.sweep_bot")
    if len({bool(c.get("with_reid", True)) for c in configs}) > 1:
        raise ValueError("with_reid decides the engine's embedding width and launches: it must "
                         "be absent from every config or equal in all of them")
    if warps is not None:
        for c in configs:  # (bytetrack against warps)
            motio._check_warp_args(tracker_type, c, 0, warps, None, None)
    return configs


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
    return _sweep_bot(tracker_type, sequences, configs, None, exp_dir=exp_dir, gt=gt,
                      benchmark=benchmark, seq_lengths=seq_lengths, frame_ids=frame_ids,
                      score=score, keep_results=keep_results, warps=warps)


def _sweep_bot(tracker_type, sequences, configs, post, *, exp_dir, gt, benchmark, seq_lengths,
               frame_ids, score, keep_results, warps) -> list:
    """``sweep_bot``; ``post``: None, or ``sweep_gsi``'s (interval, tau)."""
    configs = _check_bot(tracker_type, configs, sequences, gt, exp_dir, score, keep_results,
                         warps)
    from . import motio
    from . import engine as E

    names = list(sequences)
    seqs = [s if isinstance(s, motio.BinSequence) else motio.BinSequence(s)
            for s in sequences.values()]
    S, K = len(seqs), len(configs)
    if not S:
        return [{"config": c, "results": {} if keep_results else None, "summary": None}
                for c in configs]
    widths = sorted({int(s.emb_dim) for s in seqs})
    if len(widths) > 1:
        raise ValueError(f"the sequences' embedding widths differ ({widths}): one engine has one "
                         "emb_dim")
    F = widths[0]
    fids, tables = _frame_tables(names, seqs, frame_ids)
    table = None
    if warps is not None:  # [T, S, 6] as run_sequences builds it, then every config's copy
        table = motio._flow_warps(names, seqs, fids, F, warps, None, None).repeat(1, K, 1)
    resolved = [_resolve_reid(tracker_type, F, c) for c in configs]
    params = [r[0] for r in resolved]
    reid = tracker_type == "botsort" and bool(params[0].with_reid)
    feed_emb = F if reid else 0
    eng = E.TableEngine(tracker_type, n_seq=K * S, track_cap=resolved[0][1],
                        det_cap=resolved[0][2], emb_dim=feed_emb, emb_f64=True, params=params[0])
    feed = None
    try:
        dets = [np.asarray(s.dets).astype(np.float32) for s in seqs]
        embs = [s.embs if feed_emb else None for s in seqs]
        for k in range(K):
            eng.set_seq_params(k * S, [params[k]] * S)
        none = [None] * ((K - 1) * S)
        feed = E.SharedSequenceFeeder(dets + none, embs + none, tables * K, feed_emb,
                                      source=list(range(S)) * K)

        def step(t, run):
            q0, ns, _, pd, po, pe, pout, pcnt = run
            eng.step(pd, po, pe if feed_emb else None,
                     None if table is None else table[t, q0: q0 + ns], pout, pcnt,
                     seq0=q0, nseq=ns)

        rows, summaries = _drive(eng, feed, step, K, gt, benchmark, seq_lengths, score,
                                 keep_results, post)
    finally:
        if feed is not None:
            feed.close()
        eng.close()
    return _report(configs, names, rows, summaries, exp_dir, gt, benchmark, seq_lengths, post)


def _boost_reid(cfg: dict) -> bool:
    """with_reid as run_sequences("boosttrack", tracker_kwargs=cfg) resolves it: the YAML default
    (on) for an empty cfg, else the constructor's (off) under cfg."""
    return bool(cfg.get("with_reid", False)) if cfg else True


def _check_boost(configs, sequences, gt, exp_dir, score, keep_results, warps) -> list:
    """The refusals of ``sweep_boost`` that need no engine and no device."""
    from . import motio

    configs = _check("boosttrack", configs, sequences, gt, exp_dir, score, keep_results,
                     supported=SUPPORTED_BOOST, what="tune.sweep_boost")
    if len({_boost_reid(c) for c in configs}) > 1:
        raise ValueError("with_reid decides the engine's embedding width and launches: it must "
                         "resolve to the same value in every config")
    if warps is not None:
        for c in configs:  # (use_ecc=False against warps)
            motio._check_warp_args("boosttrack", c, 0, warps, None, None)
    return configs


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
    return _sweep_boost(sequences, configs, None, exp_dir=exp_dir, gt=gt, benchmark=benchmark,
                        seq_lengths=seq_lengths, frame_ids=frame_ids, score=score,
                        keep_results=keep_results, warps=warps)


def _sweep_boost(sequences, configs, post, *, exp_dir, gt, benchmark, seq_lengths, frame_ids,
                 score, keep_results, warps) -> list:
    """``sweep_boost``; ``post``: None, or ``sweep_gsi``'s (interval, tau)."""
    configs = _check_boost(configs, sequences, gt, exp_dir, score, keep_results, warps)
    from . import motio
    from . import engine as E

    names = list(sequences)
    seqs = [s if isinstance(s, motio.BinSequence) else motio.BinSequence(s)
            for s in sequences.values()]
    S, K = len(seqs), len(configs)
    if not S:
        return [{"config": c, "results": {} if keep_results else None, "summary": None}
                for c in configs]
    widths = sorted({int(s.emb_dim) for s in seqs})
    if len(widths) > 1:
        raise ValueError(f"the sequences' embedding widths differ ({widths}): one engine has one "
                         "emb_dim")
    F = widths[0]
    fids, tables = _frame_tables(names, seqs, frame_ids)
    table = None
    if warps is not None:  # [T, S, 6] as run_sequences builds it, then every config's copy
        table = motio._flow_warps(names, seqs, fids, F, warps, None, None).repeat(1, K, 1)
    resolved = [_resolve_reid("boosttrack", F, c) for c in configs]
    params = [r[0] for r in resolved]
    if len({bool(p.with_reid) for p in params}) > 1:  # (what _check_boost's reading missed)
        raise ValueError("with_reid resolves differently across the configs: "
                         f"{[bool(p.with_reid) for p in params]}")
    feed_emb = F if params[0].with_reid else 0
    eng = E.BoostTableEngine(n_seq=K * S, track_cap=resolved[0][1], det_cap=resolved[0][2],
                             emb_dim=feed_emb, params=params[0])
    feed = None
    try:
        dets = [np.asarray(s.dets).astype(np.float32) for s in seqs]
        embs = [s.embs if feed_emb else None for s in seqs]
        for k in range(K):
            eng.set_seq_params(k * S, [params[k]] * S)
        none = [None] * ((K - 1) * S)
        feed = E.SharedSequenceFeeder(dets + none, embs + none, tables * K, feed_emb,
                                      source=list(range(S)) * K)

        def step(t, run):
            q0, ns, _, pd, po, pe, pout, pcnt = run
            eng.step(pd, po, pe if feed_emb else None,
                     None if table is None else table[t, q0: q0 + ns], pout, pcnt,
                     seq0=q0, nseq=ns)

        rows, summaries = _drive(eng, feed, step, K, gt, benchmark, seq_lengths, score,
                                 keep_results, post)
    finally:
        if feed is not None:
            feed.close()
        eng.close()
    return _report(configs, names, rows, summaries, exp_dir, gt, benchmark, seq_lengths, post)


def _strong_occ(cfg: dict) -> bool:
    """handle_occlusions as run_sequences("strongsort", tracker_kwargs=cfg) resolves it: on, the
    reference's default, unless cfg switches it off."""
    return bool(cfg.get("handle_occlusions", True))


def _check_strong(configs, sequences, gt, exp_dir, score, keep_results, warps,
                  occlusion="host") -> list:
    """The refusals of ``sweep_strong`` that need no engine and no device."""
    from . import motio

    motio.check_occlusion("strongsort", occlusion)
    configs = _check("strongsort", configs, sequences, gt, exp_dir, score, keep_results,
                     supported=SUPPORTED_STRONG, what="tune.sweep_strong")
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
            motio._check_warp_args("strongsort", c, 0, warps, None, None)
    return configs


def _resolve_strong(F: int, cfg: dict):
    """(SsParams, track_cap, det_cap, vec_cap, occlusion_threshold or None) of one config,
    resolved as run_sequences resolves its tracker_kwargs: through ``motio._batched_engine``
    itself, on a one-sequence engine."""
    from . import motio

    eng = motio._batched_engine("strongsort", 1, F, cfg)[0]
    try:
        return eng.params, eng.track_cap, eng.det_cap, eng.vec_cap, eng.occlusion_threshold
    finally:
        eng.close()


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
    return _sweep_strong(sequences, configs, None, exp_dir=exp_dir, gt=gt, benchmark=benchmark,
                         seq_lengths=seq_lengths, frame_ids=frame_ids, score=score,
                         keep_results=keep_results, warps=warps)


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
    return _sweep_strong(sequences, configs, None, exp_dir=exp_dir, gt=gt, benchmark=benchmark,
                         seq_lengths=seq_lengths, frame_ids=frame_ids, score=score,
                         keep_results=keep_results, warps=warps, occlusion=occlusion)


def _sweep_strong(sequences, configs, post, *, exp_dir, gt, benchmark, seq_lengths, frame_ids,
                  score, keep_results, warps, occlusion="host") -> list:
    """``sweep_strong``; ``post``: None, or ``sweep_gsi``'s (interval, tau)."""
    configs = _check_strong(configs, sequences, gt, exp_dir, score, keep_results, warps,
                            occlusion)
    import dataclasses

    from . import motio
    from . import engine as E

    names = list(sequences)
    seqs = [s if isinstance(s, motio.BinSequence) else motio.BinSequence(s)
            for s in sequences.values()]
    S, K = len(seqs), len(configs)
    if not S:
        return [{"config": c, "results": {} if keep_results else None, "summary": None}
                for c in configs]
    widths = sorted({int(s.emb_dim) for s in seqs})
    if len(widths) > 1 or not widths[0]:
        raise ValueError(f"StrongSort needs embeddings of one width in every sequence (got "
                         f"{widths}): one engine has one emb_dim")
    F = widths[0]
    dets = [np.asarray(s.dets).astype(np.float32) for s in seqs]
    for s, d in zip(seqs, dets):  # (before any engine is built)
        if not np.array_equal(d.astype(np.float64), np.asarray(s.dets)):
            raise ValueError(f"{s.path}: detections that are not float32 values cannot be "
                             "held once as float32 (run_sequences feeds them as float64): "
                             "pack the sequence from detections rounded to float32")
    fids, tables = _frame_tables(names, seqs, frame_ids)
    table = None
    if warps is not None:  # [T, S, 6] as run_sequences builds it, then every config's copy
        table = motio._flow_warps(names, seqs, fids, F, warps, None, None).repeat(1, K, 1)
    resolved = [_resolve_strong(F, c) for c in configs]
    params = [r[0] for r in resolved]
    occ_thr = [r[4] for r in resolved]
    device = occlusion == "device"
    if len({r[1:4] for r in resolved}) > 1 or (
            not device and len({t is None for t in occ_thr}) > 1):
        raise ValueError("the configs resolve to different capacities or handle_occlusions: "
                         f"{[r[1:] for r in resolved]}")
    base = dataclasses.replace(params[0], nn_budget=max(int(p.nn_budget) for p in params))
    eng = E.SsTableEngine(n_seq=K * S, track_cap=resolved[0][1], det_cap=resolved[0][2],
                          emb_dim=F, vec_cap=resolved[0][3], params=base)
    feed = None
    try:
        embs = [s.embs for s in seqs]
        for k in range(K):
            eng.set_seq_params(k * S, [params[k]] * S)
        after = None
        if device and any(t is not None for t in occ_thr):
            for k in range(K):
                eng.set_occlusion(k * S, occ_thr[k] is not None,
                                  0.3 if occ_thr[k] is None else occ_thr[k], nseq=S)
            after = lambda: motio.raise_device_occlusion(eng, names)  # noqa: E731
        none = [None] * ((K - 1) * S)
        feed = E.SharedSequenceFeeder(dets + none, embs + none, tables * K, F,
                                      source=list(range(S)) * K, det_f64=True, out_cols=10)

        def step(t, run, out=None, cnt=None):
            q0, ns, _, pd, po, pe, pout, pcnt = run
            eng.step(pd, po, pe, None if table is None else table[t, q0: q0 + ns],
                     pout if out is None else out, pcnt if cnt is None else cnt,
                     seq0=q0, nseq=ns)

        if device or occ_thr[0] is None:
            rows, summaries = _drive(eng, feed, step, K, gt, benchmark, seq_lengths, score,
                                     keep_results, post, after)
        else:
            rows, summaries = _drive_occlusion(eng, feed, step, fids * K,
                                               [tb[1] for tb in tables] * K,
                                               [t for t in occ_thr for _ in range(S)]), None
            if post is not None:
                rows = _gsi_host_rows(rows, post)
    finally:
        if feed is not None:
            feed.close()
        eng.close()
    return _report(configs, names, rows, summaries, exp_dir, gt, benchmark, seq_lengths, post)


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
            step(t, run, out, cnt)
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
    name = GSI_DISPATCH[tracker_type]
    # the public sweep's defaults under the caller's keywords; one it does not have is the
    # implementation's TypeError
    kw = {**globals()[name].__kwdefaults__, **sweep_kwargs}
    head = () if name in ("sweep_boost", "sweep_strong") else (tracker_type,)  # (one tracker)
    return globals()["_" + name](*head, sequences, configs, (int(interval), float(tau)), **kw)


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

#!/usr/bin/env python
"""Time a sweep scored after GSI in two ways, K ocsort configs on the two scenes of
tests/tune_data.py:

  (a) tune.sweep_gsi(score="device", keep_results=False): track, GSI and evaluation without a
      result row on the host;
  (b) the flow without it: tune.sweep(keep_results=True), then gsi_batch and the "%d" truncation
      per config, then evaluate_mot per config.

The two alternate, REPEATS times after one warm-up of each; wall time around work that ends in a
device synchronise.  The summaries of the two flows are compared.  Prints one JSON line with the
median and the fastest of each and the kernel launches of the GSI stage (counted from the row
counts: pack or keys, the bitonic passes, scan, fill, the smoothing kernels, finalise).
Recorded in DESIGN.md 2.25; nothing gates on it.
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def bitonic_passes(rows: int) -> int:
    p = 1
    while p < max(rows, 1):
        p <<= 1
    lg = p.bit_length() - 1
    return lg * (lg + 1) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--interval", type=int, default=20)
    ap.add_argument("--tau", type=float, default=10)
    a = ap.parse_args()

    import torch

    from boxmot_amd import evaluate_mot, mot_summary, motio, tune
    from boxmot_amd.postprocessing import gsi_batch
    from tests import tune_data as TD

    names = [f"MOT17-{s:02d}" for s in range(TD.S)]
    gt = {nm: TD.synthetic_gt(s) for s, nm in enumerate(names)}
    space = dict(det_thresh=[0.3, 0.4, 0.5, 0.6], max_age=[2, 30], asso_func=["iou", "giou"])
    configs = tune.grid(space)[: a.configs]
    with tempfile.TemporaryDirectory() as d:
        packed = {nm: motio.pack_arrays(TD.packed_rows(TD.scene_frames(s)), None,
                                        Path(d) / f"{nm}.bxmot") for s, nm in enumerate(names)}

        def flow_a():
            res = tune.sweep_gsi("ocsort", packed, configs, interval=a.interval, tau=a.tau, gt=gt,
                                 score="device", keep_results=False)
            return [r["summary"] for r in res]

        rows_in, rows_out = [], []

        def flow_b():
            res = tune.sweep("ocsort", packed, configs)
            out = []
            rows_in.clear(), rows_out.clear()
            for r in res:
                arrs = gsi_batch([r["results"][nm] for nm in names], a.interval, a.tau)
                rows_in.append(sum(r["results"][nm].shape[0] for nm in names))
                rows_out.append(sum(x.shape[0] for x in arrs))
                out.append(mot_summary(evaluate_mot(
                    gt, {nm: np.trunc(x) + 0.0 for nm, x in zip(names, arrs)})))
            return out

        sa, sb = flow_a(), flow_b()  # warm-up: the library, the allocator, every shape
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(a.repeats):
            for flow, ts in ((flow_a, ta), (flow_b, tb)):
                t0 = time.perf_counter()
                flow()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
    # the GSI stage's kernels: (a) one call over all K * S slots, (b) one gsi_batch per config;
    # 2 stands for the smoothing kernels (LDS and blocked; the blocked one only if a tracklet
    # exceeds 176 rows, which these scenes never reach, so it is 1 here)
    launches_a = 1 + bitonic_passes(sum(rows_in)) + 1 + 1 + 1 + 1
    launches_b = sum(1 + bitonic_passes(r) + 1 + 1 + 1 for r in rows_in)
    print(json.dumps(dict(
        configs=len(configs), sequences=len(names), repeats=a.repeats,
        rows_in=int(sum(rows_in)), rows_out=int(sum(rows_out)), same_summaries=sa == sb,
        a_sweep_gsi_device_s=dict(median=float(np.median(ta)), min=float(min(ta))),
        b_sweep_gsi_batch_evaluate_s=dict(median=float(np.median(tb)), min=float(min(tb))),
        gsi_stage_launches=dict(a=launches_a, b=launches_b),
        evaluator_runs=dict(a=1, b=len(configs)))))


if __name__ == "__main__":
    main()

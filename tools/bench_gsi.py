#!/usr/bin/env python
"""Time the GSI post-processing on one workload: FILES result files x TRACKS tracklets x FRAMES
frames each (seeded random walks, one short gap per tracklet).

  python tools/bench_gsi.py                      # gsi_batch on the GPU (device events + wall)
  python tools/bench_gsi.py --reference DIR      # the reference's per-file loop on the CPU
                                                 # (DIR holds its `boxmot` package), PROCS processes

Prints one JSON line.  Recorded in DESIGN.md; nothing gates on it.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def make_file(seed, tracks, frames):
    rng = np.random.default_rng(seed)
    rows = []
    for ident in range(1, tracks + 1):
        f = np.arange(1, frames + 1)
        a = int(rng.integers(2, frames - 8))
        f = np.delete(f, np.arange(a, a + 5))
        box = np.array([800.0, 400.0, 60.0, 120.0]) + np.cumsum(rng.normal(0, 2, (len(f), 4)), 0)
        rows.append(np.concatenate([f[:, None].astype(float), np.full((len(f), 1), float(ident)),
                                    box, np.full((len(f), 1), 0.9), np.zeros((len(f), 1))], 1))
    return np.concatenate(rows)


def _ref_file(args):
    ref_dir, seed, tracks, frames, interval, tau = args
    sys.path.insert(0, str(Path(ref_dir) / "tests" / "golden"))
    from make_golden import install_shim

    install_shim()
    from boxmot.postprocessing.gsi import gaussian_smooth, linear_interpolation

    a = make_file(seed, tracks, frames)
    t0 = time.perf_counter()
    gaussian_smooth(linear_interpolation(a, interval), tau)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--interval", type=int, default=20)
    ap.add_argument("--tau", type=float, default=10)
    ap.add_argument("--reference", action="store_true",
                    help="time the reference's two functions per file on the CPU (through the "
                         "shim of tests/golden/make_golden.py)")
    ap.add_argument("--procs", type=int, default=16)
    a = ap.parse_args()
    res = dict(files=a.files, tracks=a.tracks, frames=a.frames)
    if a.reference:
        from concurrent.futures import ProcessPoolExecutor

        repo = Path(__file__).resolve().parents[1]
        jobs = [(repo, s, a.tracks, a.frames, a.interval, a.tau) for s in range(a.files)]
        t0 = time.perf_counter()
        with ProcessPoolExecutor(max_workers=min(a.procs, 16)) as ex:
            per = list(ex.map(_ref_file, jobs))
        res.update(mode="reference_cpu", procs=min(a.procs, 16),
                   wall_s=time.perf_counter() - t0, cpu_s_sum=float(np.sum(per)))
    else:
        import torch

        from boxmot_amd.postprocessing import gsi_batch

        arrays = [make_file(s, a.tracks, a.frames) for s in range(a.files)]
        gsi_batch(arrays[:2], a.interval, a.tau)  # load the library, warm the allocator
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = gsi_batch(arrays, a.interval, a.tau)
        e1.record()
        torch.cuda.synchronize()
        res.update(mode="gsi_batch_gpu", wall_s=time.perf_counter() - t0,
                   event_ms=e0.elapsed_time(e1), rows_out=int(sum(o.shape[0] for o in out)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

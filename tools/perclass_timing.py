#!/usr/bin/env python
"""HybridSort step time and stage shares on the batched engine, and the cost of the class split +
id merge of ``step_classes`` for HybridSort and DeepOCSort.

The scene and the method of tools/deepoc_timing.py: 1024 sequences x 64 objects x F = 128
(float64 embeddings), 40 warm-up frames, then 60 timed frames staged in HBM first; the timed
window is device events around the 60 steps (one synchronise at its end).  Every figure is taken
``--repeats`` times, each on a fresh engine over the same frames, and printed as median [min,
max].  Lines:
  <tracker> step           ms/step
  <tracker> step_classes   the same detections, every class 0, one class: split + merge on top
  HybridSort's three stages from separate, untimed passes with bx_hybrid_probe on one stage at a
  time, as deepoc_timing.py does for DeepOCSort
Recorded in DESIGN.md 2.11 / 2.12, not gated: none of these has an earlier value to compare with.

Usage: python tools/perclass_timing.py [--seqs 1024] [--objs 64] [--dim 128] [--layout crowded]
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def spread(v):
    return f"{statistics.median(v):.3f} [{min(v):.3f}, {max(v):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=1024)
    ap.add_argument("--objs", type=int, default=64)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layout", default="grid")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("perclass_timing needs a HIP device: no timing is taken without one")
    from boxmot_amd.engine import (DeepOcsortEngine, DeepOcsortParams, HybridsortEngine,
                                   HybridsortParams)
    from boxmot_amd.synth import TorchSceneBatch

    S, NF = a.seqs, a.warmup + a.steps
    cap = 1 << max(5, (2 * a.objs - 1).bit_length())  # slots for every object, with room
    scene = TorchSceneBatch(S, a.objs, emb_dim=a.dim, seed=5, conf_lo=0.31, layout=a.layout)
    frames = []
    for t in range(1, NF + 1):
        d, off, e = scene.frame(t)
        d = d.clone()
        d[:, 5] = 0.0  # one class
        frames.append((d, off, e.double().contiguous()))
    rows = max(int(f[0].shape[0]) for f in frames)
    out = torch.zeros((rows, 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(S, dtype=torch.int32, device="cuda")

    def timed(step):
        for f in frames[: a.warmup]:
            step(f)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for f in frames[a.warmup:]:
            step(f)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def hybrid():
        return HybridsortEngine(S, cap, a.objs, a.dim, HybridsortParams())

    res = {}
    for name, make, plain, classes in [
        ("hybridsort", hybrid, lambda g, f: g.step(f[0], f[1], f[2], out, cnt),
         lambda g, f: g.step_classes(f[0], f[1], f[2], out, cnt, 1)),
        ("deepocsort", lambda: DeepOcsortEngine(S, cap, a.objs, a.dim, DeepOcsortParams()),
         lambda g, f: g.step(f[0], f[1], f[2], None, out, cnt),
         lambda g, f: g.step_classes(f[0], f[1], f[2], None, out, cnt, 1)),
    ]:
        for mode, fn in (("step", plain), ("step_classes", classes)):
            ms = []
            for _ in range(a.repeats):
                eng = make()
                ms.append(timed(lambda f: fn(eng, f)))
                assert eng.status() == 0
                eng.close()
            res[name, mode] = ms
            print(f"{name} {mode:12s} {S} seq x {a.objs} obj x F={a.dim} ({a.layout}): "
                  f"{spread(ms)} ms/step")
        d = [c - p for c, p in zip(res[name, "step_classes"], res[name, "step"])]
        base = statistics.median(res[name, "step"])
        print(f"  split + merge (C = 1): {spread(d)} ms/step "
              f"({100 * statistics.median(d) / base:+.1f}% of the step)")

    base = statistics.median(res["hybridsort", "step"])
    for stage in HybridsortEngine.STAGES:  # untimed passes: one probed stage each
        v = []
        for _ in range(a.repeats):
            eng = hybrid()
            for k, f in enumerate(frames):
                if k == a.warmup:
                    torch.cuda.synchronize()
                    eng.probe(stage)
                eng.step(f[0], f[1], f[2], out, cnt)
            tot, n = eng.probe_read()
            v.append(tot / max(n, 1))
            eng.close()
        print(f"  hybridsort {stage:8s} {spread(v)} ms/step "
              f"({100 * statistics.median(v) / base:.0f}% of the step)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""DeepOCSort step time on the batched engine, beside OCSort on the same detections.

1024 sequences x 64 objects x F = 128 (float64 embeddings), 40 warm-up frames, then 60 timed
frames: the frames are staged in HBM first, the timed window is device events around the 60
steps (one synchronise at its end).  The three kernels' shares come from a separate, untimed
pass over the same frames with bx_deepoc_probe on one stage at a time.  The OCSort line (motion
only, same detections, same det_thresh) is the baseline the gap is read against.  Recorded in
DESIGN.md 2.9, not gated.

Usage: python tools/deepoc_timing.py [--seqs 1024] [--objs 64] [--dim 128] [--layout crowded]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

PEAK_F64_MFMA = 78.6e12  # FLOP/s, MI355X fp64 matrix peak (MI355X_MICROARCH.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=1024)
    ap.add_argument("--objs", type=int, default=64)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--layout", default="grid")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("deepoc_timing needs a HIP device: no timing is taken without one")
    from boxmot_amd.engine import (DeepOcsortEngine, DeepOcsortParams, OcsortEngine,
                                   OcsortParams)
    from boxmot_amd.synth import TorchSceneBatch

    S, NF = a.seqs, a.warmup + a.steps
    cap = 1 << max(5, (2 * a.objs - 1).bit_length())  # slots for every object, with room
    scene = TorchSceneBatch(S, a.objs, emb_dim=a.dim, seed=5, conf_lo=0.31, layout=a.layout)
    frames = []
    for t in range(1, NF + 1):
        d, off, e = scene.frame(t)
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

    def deepoc():
        return DeepOcsortEngine(S, cap, a.objs, a.dim, DeepOcsortParams())

    eng = deepoc()
    ms = timed(lambda f: eng.step(f[0], f[1], f[2], None, out, cnt))
    assert eng.status() == 0
    stats = eng.frame_stats()
    eng.close()
    print(f"deepocsort {S} seq x {a.objs} obj x F={a.dim} ({a.layout}): {ms:.3f} ms/step "
          f"({stats['tracks'] / S:.1f} tracks/seq at the end)")

    shares, flops = {}, 0.0
    for stage in DeepOcsortEngine.STAGES:  # untimed passes: one probed stage each
        eng = deepoc()
        pairs = 0
        for k, f in enumerate(frames):
            if k == a.warmup:
                torch.cuda.synchronize()
                eng.probe(stage)
            if k >= a.warmup and stage == "embcost":
                nt = eng.frame_stats()["tracks"]  # (synchronises: this pass is not timed)
                pairs += int(f[0].shape[0]) * nt / S
            eng.step(f[0], f[1], f[2], None, out, cnt)
        tot, n = eng.probe_read()
        shares[stage] = tot / max(n, 1)
        if stage == "embcost":
            flops = 2.0 * a.dim * pairs / a.steps  # useful FLOP per step (mean tracks per seq)
        eng.close()
    for stage, v in shares.items():
        print(f"  {stage:8s} {v:.3f} ms/step ({100 * v / ms:.0f}% of the step)")
    if shares["embcost"] > 0:
        rate = flops / (shares["embcost"] * 1e-3)
        print(f"  embcost  {rate / 1e12:.2f} TFLOP/s useful = {100 * rate / PEAK_F64_MFMA:.1f}% of "
              f"the fp64 MFMA peak ({PEAK_F64_MFMA / 1e12:.1f} TFLOP/s)")

    oc = OcsortEngine(S, cap, a.objs, OcsortParams(det_thresh=0.3, inertia=0.2))
    ms_oc = timed(lambda f: oc.step(f[0], f[1], out, cnt))
    assert oc.status() == 0
    oc.close()
    print(f"ocsort     same detections, motion only: {ms_oc:.3f} ms/step "
          f"(deepocsort / ocsort = {ms / ms_oc:.2f}x; frame kernel alone "
          f"{shares['frame'] / ms_oc:.2f}x)")


if __name__ == "__main__":
    main()

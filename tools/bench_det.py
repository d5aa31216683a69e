#!/usr/bin/env python
"""Times the detector front end (boxmot_amd/det.py) on the device against what a user of plain
torch has without it.  Device events around every call, warm-up first, medians reported.

  letterbox    B frames of 1080 x 1920 into (800, 1440), float32 and float16; the bytes it must
               move (frames read once, output written once) over the time give its share of the
               HBM rate.  Baseline: torch.nn.functional.interpolate + pad + normalise (not
               bit-comparable; timed only).
  postprocess  pred [B, 23625, 6] with about `cands` candidates per image at conf 0.01.
               Baseline: the plain-torch restatement (sort, IoU matrix, the Python keep loop with
               one host synchronisation per kept box), which is what stands in for
               torchvision.ops.batched_nms where torchvision does not exist.

Prints one JSON line per measurement.  Run kernel by kernel under a tracer for the split between
filter, sort, matrix and sweep: the kernels are named det_*_kernel.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

HBM_PEAK = 8.0e12  # bytes per second (spec)


def timed(fn, warmup, reps):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def synth_pred(B, A, cands, seed):
    """[B, A, 6] on the device: `cands` rows per image score above 0.01, as clusters of about
    five overlapping boxes around random centres in an 800 x 1440 input."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    pred = torch.zeros(B, A, 6, device="cuda")
    pred[..., 0] = torch.rand(B, A, generator=g, device="cuda") * 1440
    pred[..., 1] = torch.rand(B, A, generator=g, device="cuda") * 800
    pred[..., 2] = 20 + torch.rand(B, A, generator=g, device="cuda") * 80
    pred[..., 3] = 40 + torch.rand(B, A, generator=g, device="cuda") * 160
    pred[..., 4] = torch.rand(B, A, generator=g, device="cuda") * 0.009
    pred[..., 5] = 1.0
    n_obj = max(1, cands // 5)
    idx = torch.rand(B, A, generator=g, device="cuda").argsort(1)[:, :cands]
    centre = idx[:, :n_obj].repeat(1, (cands + n_obj - 1) // n_obj)[:, :cands]
    rows = torch.gather(pred, 1, centre[..., None].expand(-1, -1, 6)).clone()
    rows[..., :4] += torch.randn(B, cands, 4, generator=g, device="cuda") * 3
    rows[..., 4] = 0.02 + torch.rand(B, cands, generator=g, device="cuda") * 0.97
    pred.scatter_(1, idx[..., None].expand(-1, -1, 6), rows)
    return pred


def torch_postprocess(pred, conf, iou_thr, ratio):
    """The plain-torch restatement a user writes without torchvision: per image a sort, an IoU
    matrix, and the greedy loop on the host."""
    import torch

    out = []
    for p in pred:
        s = p[:, 4] * p[:, 5]
        p = p[s >= conf]
        s = s[s >= conf]
        order = s.argsort(descending=True)
        p, s = p[order], s[order]
        b = torch.stack([p[:, 0] - p[:, 2] / 2, p[:, 1] - p[:, 3] / 2, p[:, 0] + p[:, 2] / 2,
                         p[:, 1] + p[:, 3] / 2], 1)
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        lt, rb = torch.max(b[:, None, :2], b[None, :, :2]), torch.min(b[:, None, 2:], b[None, :, 2:])
        inter = (rb - lt).clamp(min=0).prod(2)
        over = inter / (area[:, None] + area[None] - inter) > iou_thr
        removed = torch.zeros(len(b), dtype=torch.bool, device=b.device)
        keep = []
        for i in range(len(b)):
            if removed[i]:  # (one host synchronisation per candidate)
                continue
            keep.append(i)
            removed |= over[i]
        k = torch.tensor(keep, dtype=torch.long, device=b.device)
        out.append(torch.cat([b[k] / ratio, s[k, None], torch.zeros_like(s[k, None])], 1))
    return out


def torch_letterbox(frames, size, r, rh, rw, half, mean, std):
    import torch
    import torch.nn.functional as F

    x = frames.permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=(rh, rw), mode="bilinear", align_corners=False)
    x = F.pad(x, (0, size[1] - rw, 0, size[0] - rh), value=114.0).flip(1) / 255.0
    x = (x - mean) / std
    return x.half() if half else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--cands", type=int, nargs="+", default=[200, 3000])
    ap.add_argument("--anchors", type=int, default=23625)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--base-reps", type=int, default=3)
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()

    import torch

    from boxmot_amd import det

    assert torch.cuda.is_available(), "bench_det needs a HIP device"
    size, H, W = (800, 1440), 1080, 1920
    r, rh, rw = det.letterbox_geometry(H, W, size)
    mean = torch.tensor(det.YOLOX_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(det.YOLOX_STD, device="cuda").view(1, 3, 1, 1)
    for B in a.batches:
        frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda")
        for half in (False, True):
            out = torch.empty((B, 3) + size, device="cuda",
                              dtype=torch.float16 if half else torch.float32)
            med, lo, hi = timed(lambda: det.letterbox(frames, size, half=half, out=out),
                                a.warmup, a.reps)
            nbytes = frames.numel() + out.numel() * out.element_size()
            rec = dict(what="letterbox", B=B, dtype="float16" if half else "float32", ms=med,
                       ms_min=lo, ms_max=hi, bytes=nbytes, tb_per_s=nbytes / med / 1e9,
                       hbm_share=nbytes / (med * 1e-3) / HBM_PEAK)
            if not a.skip_baseline:
                base = timed(lambda: torch_letterbox(frames, size, r, rh, rw, half, mean, std),
                             a.warmup, a.reps)[0]
                rec.update(torch_ms=base, ratio=base / med)
            print(json.dumps(rec), flush=True)
        del frames
        for cands in a.cands:
            pred = synth_pred(B, a.anchors, cands, seed=B * 100003 + cands)
            ratio = torch.full((B,), r, device="cuda")
            outs = det.postprocess(pred, ratio=ratio)
            off = outs[1].cpu()
            fn = lambda: det.postprocess(pred, ratio=ratio, out=outs)  # noqa: E731
            med, lo, hi = timed(fn, a.warmup, a.reps)
            rec = dict(what="postprocess", B=B, A=a.anchors, cands=cands,
                       kept_per_image=float(off[-1]) / B, ms=med, ms_min=lo, ms_max=hi)
            if not a.skip_baseline:
                base = timed(lambda: torch_postprocess(pred, 0.01, 0.7, r), 1, a.base_reps)[0]
                rec.update(torch_ms=base, ratio=base / med)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

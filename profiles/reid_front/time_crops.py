"""Times bx_reid_crops with device events against its two references (neither is the code under
test): the store floor (output bytes over the HBM bandwidth) and what a user can write today, a
loop of torch.nn.functional.interpolate per box on the same device (not bit-compatible).

Workload: 64 frames of 1080x1920 with 128 boxes each (8192 crops, pedestrian-sized, seeded), into
256x128, float32 and fp16; warm, median of 20.  Needs a HIP device; prints one JSON line per
case and, with --out, writes them to a file.

    python profiles/reid_front/time_crops.py [--out FILE] [--loop-boxes 1024]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from boxmot_amd import reid  # noqa: E402

HBM_MEASURED = 6.29e12  # bytes/s, float4 copy on the MI355X (8.0e12 is the specification)
HBM_SPEC = 8.0e12
F, H, W, PER_FRAME = 64, 1080, 1920, 128
SIZE = (256, 128)


def workload(seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    frames = torch.randint(0, 256, (F, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    rng = np.random.default_rng(seed)
    n = F * PER_FRAME
    w = rng.uniform(40.0, 160.0, n)            # pedestrian-sized: 40..160 wide, 2..3 times as tall
    h = w * rng.uniform(2.0, 3.0, n)
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)  # (boxes at the border overhang it)
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
    frame_of = np.repeat(np.arange(F, dtype=np.int32), PER_FRAME)
    return frames, torch.from_numpy(boxes).cuda(), torch.from_numpy(frame_of).cuda(), boxes


def median_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def interpolate_loop(frames, boxes_host, frame_of_host, out, mean, std, k):
    """The reference's get_crops with the resize moved to the device: per box a slice, a permute,
    one F.interpolate and a write into the batch; the normalisation once at the end."""
    for i in range(k):
        x1, y1, x2, y2 = np.rint(boxes_host[i]).astype(int)
        x1, y1, x2, y2 = max(0, x1), max(0, y1), min(W, x2), min(H, y2)
        crop = frames[frame_of_host[i], y1:y2, x1:x2].permute(2, 0, 1)[None].to(out.dtype)
        out[i] = torch.nn.functional.interpolate(crop, size=SIZE, mode="bilinear",
                                                 align_corners=False)[0].flip(0)
    o = out[:k]
    o /= 255.0
    o -= mean
    o /= std


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--loop-boxes", type=int, default=1024,
                    help="boxes the interpolate loop is timed on (its time is per box)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    frames, boxes, frame_of, boxes_host = workload()
    fo_host = frame_of.cpu().numpy()
    ok = np.array([x2 > x1 and y2 > y1 for x1, y1, x2, y2 in
                   (np.clip(np.rint(b), 0, [W, H, W, H]) for b in boxes_host)])
    assert ok.all(), "the workload has no empty crop"
    n = boxes.shape[0]
    lines = []
    for half in (False, True):
        dtype = torch.float16 if half else torch.float32
        out = torch.empty((n, 3, *SIZE), dtype=dtype, device="cuda")
        codes = torch.empty(n, dtype=torch.int32, device="cuda")
        med, lo, hi = median_ms(lambda: reid.crop_batch(frames, boxes, frame_of, SIZE, half,
                                                        out=out, codes=codes))
        assert not codes.any().item()
        nbytes = out.numel() * out.element_size()
        floor = nbytes / HBM_MEASURED * 1e3
        k = min(args.loop_boxes, n)
        mean = torch.tensor(reid.IMAGENET_MEAN, device="cuda", dtype=dtype).view(1, 3, 1, 1)
        std = torch.tensor(reid.IMAGENET_STD, device="cuda", dtype=dtype).view(1, 3, 1, 1)
        loop, _, _ = median_ms(lambda: interpolate_loop(frames, boxes_host, fo_host, out, mean,
                                                        std, k), reps=5, warm=1)
        loop_all = loop * n / k
        lines.append({
            "case": "fp16" if half else "float32", "crops": n, "out_bytes": nbytes,
            "kernel_ms_median": round(med, 4), "kernel_ms_min": round(lo, 4),
            "kernel_ms_max": round(hi, 4), "achieved_TBps": round(nbytes / med / 1e9, 3),
            "store_floor_ms_at_6.29TBps": round(floor, 4),
            "fraction_of_floor": round(floor / med, 3),
            "store_floor_ms_at_8.0TBps_spec": round(nbytes / HBM_SPEC * 1e3, 4),
            "interpolate_loop_boxes_timed": k, "interpolate_loop_ms_scaled_to_all": round(loop_all, 1),
            "speedup_over_loop": round(loop_all / med, 1)})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()

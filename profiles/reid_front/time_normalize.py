"""Times bx_reid_normalize with device events: 8192 float32 rows, for a width that takes the
wave-parallel sum (512 = 128 * 4) and for widths that take one sequential walk per wave (1280,
2051).  Warm, median of 20; one JSON line per width.

    python profiles/reid_front/time_normalize.py [--out FILE]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from time_crops import median_ms  # noqa: E402

from boxmot_amd import reid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    n, lines = 8192, []
    for F in (512, 1280, 2051):
        x = torch.randn(n, F, device="cuda")
        out = torch.empty_like(x)
        med, lo, hi = median_ms(lambda: reid.normalize_features(x, out=out))
        lines.append({"rows": n, "F": F, "wave_parallel_sum": F == 512,
                      "kernel_ms_median": round(med, 4), "kernel_ms_min": round(lo, 4),
                      "kernel_ms_max": round(hi, 4),
                      "bytes_moved": 2 * x.numel() * 4,
                      "achieved_TBps": round(2 * x.numel() * 4 / med / 1e9, 3)})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        Path(args.out).write_text("".join(json.dumps(v) + "\n" for v in lines))


if __name__ == "__main__":
    main()

"""The crop launch alone, for a counter run: the timing workload of time_crops.py, one warm-up
and three launches each of the float32 and the fp16 kernel, nothing else on the device.

    rocprofv3 --pmc COUNTER... --output-format csv -d DIR -o run -- \
        python profiles/reid_front/pmc_crops.py
    python profiles/reid_front/pmc_report.py DIR...

(counters in a run of their own: no tracing in the same run)
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from time_crops import SIZE, workload  # noqa: E402

from boxmot_amd import reid  # noqa: E402


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    frames, boxes, frame_of, _ = workload()
    n = boxes.shape[0]
    for half in (False, True):
        out = torch.empty((n, 3, *SIZE), dtype=torch.float16 if half else torch.float32,
                          device="cuda")
        for _ in range(4):
            reid.crop_batch(frames, boxes, frame_of, SIZE, half, out=out)
        torch.cuda.synchronize()
        del out
    print("done")


if __name__ == "__main__":
    main()

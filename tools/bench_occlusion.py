"""Time per frame index of ``motio.run_sequences("strongsort", ...)`` with StrongSort's occlusion
handling on the host (an ``OcclusionHandler`` per sequence) and on the device (the engine's
occlusion pass), over a synthetic ``corner`` set of S sequences.

    python tools/bench_occlusion.py --seqs 16 --objects 24 --frames 40 --runs 5

One warm-up run per mode (library load, allocator, first launches), then ``--runs`` timed runs
each, interleaved host/device so drift hits both; the wall time of a whole run, files included,
divided by the frame indices.  Prints the median and the min-max spread per mode and one JSON
line.  A run that raises the reference's TypeError (a mutual occlusion in the scene) is reported
and ends the benchmark."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seqs", type=int, default=16)
    ap.add_argument("--objects", type=int, default=24)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--emb-dim", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    os.environ["GITHUB_ACTIONS"] = "true"  # tracks born Confirmed, as the fixtures
    os.environ.pop("GITHUB_JOB", None)
    import torch

    from boxmot_amd import motio
    from boxmot_amd.synth import SyntheticScene

    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        seqs = {}
        for s in range(a.seqs):
            # one scene for every sequence: the corner layout of the occlusion fixtures, whose
            # seed 42 runs 80 frames without a mutual occlusion (other seeds raise early)
            sc = SyntheticScene(n_obj=a.objects, seed=42, layout="corner", emb_dim=a.emb_dim,
                                emb_dtype=np.float64, conf_lo=0.3, p_det=0.8,
                                corner=((30, 0.9), (55, 0.9), (95, 0.9), (160, 0.9)))
            rows, embs = [], []
            for t in range(1, a.frames + 1):
                d, e, _ = sc.frame(t)
                rows.append(np.concatenate([np.full((d.shape[0], 1), t), d], 1))
                embs.append(e)
            seqs[f"c{s:03d}"] = motio.pack_arrays(
                np.concatenate(rows).astype(np.float32).astype(np.float64), np.concatenate(embs),
                tmp / f"c{s:03d}.bxmot")
        kw = dict(occlusion_threshold=a.threshold)

        def run(mode, k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            motio.run_sequences("strongsort", seqs, tmp / f"{mode}{k}", tracker_kwargs=kw,
                                occlusion=mode)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.frames * 1e3

        times = {"host": [], "device": []}
        try:
            for mode in times:
                run(mode, "w")
            for k in range(a.runs):
                for mode in times:
                    times[mode].append(run(mode, k))
        except TypeError as e:
            print(f"the scene holds a mutual occlusion ({e}); choose other sizes or a threshold")
            return 1
        same = all((tmp / "host0" / f"{nm}.txt").read_bytes() ==
                   (tmp / "device0" / f"{nm}.txt").read_bytes() for nm in seqs)
    out = {"seqs": a.seqs, "objects": a.objects, "frames": a.frames, "emb_dim": a.emb_dim,
           "runs": a.runs, "files_identical": same}
    for mode, ts in times.items():
        out[f"{mode}_ms_per_frame_index"] = round(statistics.median(ts), 4)
        out[f"{mode}_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
        print(f"{mode:6s}: median {statistics.median(ts):8.3f} ms per frame index "
              f"(min {min(ts):.3f}, max {max(ts):.3f}, {a.runs} runs)")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

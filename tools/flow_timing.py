#!/usr/bin/env python
"""Wall time of DeepOcSort (or, with --tracker hybridsort, HybridSort) over many sequences, three
ways:

  dropins    one fresh single-sequence drop-in per sequence, one after the other
  default    motio.run_sequences(tracker, ...): one batched engine, frames assembled on the host
  resident   the same with resident=True: the sequences and the result rows stay in device memory

Every way reads the same packed sequences and writes the same MOT files (checked byte for byte).

    python tools/flow_timing.py --seqs 256 --frames 200 --objects 44 --emb-dim 64
    python tools/flow_timing.py --tracker hybridsort
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--objects", type=int, default=44)  # p_det 0.9: about 40 detections a frame
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-dropins", action="store_true")
    ap.add_argument("--tracker", default="deepocsort", choices=["deepocsort", "hybridsort"])
    a = ap.parse_args()
    import torch

    from boxmot_amd import DeepOcSort, HybridSort, motio
    from boxmot_amd.synth import SyntheticScene

    img = np.zeros((1080, 1920, 3), np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        packed, dets_total = {}, 0
        for k in range(a.seqs):
            sc = SyntheticScene(n_obj=a.objects, seed=7000 + k, emb_dim=a.emb_dim,
                                emb_dtype="float64", p_det=0.9, conf_lo=0.31,
                                layout="crowded" if k % 2 else "grid")
            d7, em = [], []
            for t in range(1, a.frames + 1):
                d, e, _ = sc.frame(t)
                d7.append(np.concatenate([np.full((d.shape[0], 1), t), d], 1))
                em.append(e)
            d7 = np.concatenate(d7)
            dets_total += d7.shape[0]
            packed[f"S{k:04d}"] = motio.pack_arrays(d7, np.concatenate(em), tmp / f"{k}.bxmot")

        def flow(resident, out):
            motio.run_sequences(a.tracker, packed, out, resident=resident)

        def dropins(out):
            for nm, p in packed.items():
                seq = motio.BinSequence(p)
                # (run_sequences gives HybridSort, whose det_thresh has no default, 0.3)
                tr = DeepOcSort() if a.tracker == "deepocsort" else HybridSort(None, None, False,
                                                                               0.3)
                rows = []
                for fid in seq.frame_ids:
                    d, e = seq.frame(fid)
                    o = np.asarray(tr.update(d, img, e), np.float64).reshape(-1, 8)
                    if o.shape[0]:
                        rows.append(motio.convert_to_mot_format(o, int(fid)))
                motio.write_mot_results(out / f"{nm}.txt",
                                        np.vstack(rows) if rows else np.empty((0, 0)))

        def timed(fn, tag, repeats, warm=1):
            best = []
            for r in range(repeats + warm):  # the first run warms up (module load, allocator)
                out = tmp / f"{tag}_{r}"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(out)
                torch.cuda.synchronize()
                best.append(time.perf_counter() - t0)
            return sorted(best[warm:]), tmp / f"{tag}_{repeats + warm - 1}"

        res = {"tracker": a.tracker, "seqs": a.seqs, "frames": a.frames, "emb_dim": a.emb_dim,
               "detections_per_frame": dets_total / (a.seqs * a.frames)}
        t_def, d_def = timed(lambda o: flow(False, o), "default", a.repeats)
        t_res, d_res = timed(lambda o: flow(True, o), "resident", a.repeats)
        res["default_s"], res["resident_s"] = t_def, t_res
        same = all((d_def / f"{nm}.txt").read_bytes() == (d_res / f"{nm}.txt").read_bytes()
                   for nm in packed)
        if not a.skip_dropins:
            t_one, d_one = timed(dropins, "dropins", 1, warm=0)  # (after the flows: warm)
            res["dropins_s"] = t_one
            same = same and all((d_def / f"{nm}.txt").read_bytes() ==
                                (d_one / f"{nm}.txt").read_bytes() for nm in packed)
        res["files_identical"] = same
        print(json.dumps(res))
        return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

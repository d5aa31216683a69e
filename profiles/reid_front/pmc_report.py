"""Per-launch counter values of the crop kernels from rocprofv3 --pmc CSV directories: a counter's
rows of one dispatch (one per instance) are summed, the launches after the warm-up averaged.

    python profiles/reid_front/pmc_report.py DIR [DIR...]
"""
import collections
import csv
import glob
import sys


def main():
    acc = collections.defaultdict(lambda: collections.defaultdict(lambda: collections.defaultdict(float)))
    for d in sys.argv[1:]:
        for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                k = r["Kernel_Name"]
                if "reid_crops_kernel" not in k:
                    continue
                kind = "fp16" if ("DF16_" in k or "_Float16" in k) else "float32"
                acc[kind][r["Counter_Name"]][(d, r["Dispatch_Id"])] += float(r["Counter_Value"])
    for kind in sorted(acc):
        print(f"reid_crops_kernel {kind}")
        for c in sorted(acc[kind]):
            per = acc[kind][c]
            ids = sorted(per, key=lambda t: (t[0], int(t[1])))
            vals = [per[i] for i in ids][1:] or [per[i] for i in ids]  # (drop the warm-up)
            print(f"   {c:28s} {sum(vals) / len(vals):18.1f}   launches {len(vals)}")


if __name__ == "__main__":
    main()

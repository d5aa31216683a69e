"""bench.py's command line: a plain run (no probes, no roofline, no CPU baseline) with
`--dump-outputs`, and the size cap of the dump."""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_script", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_float64_and_seeded_sample(tmp_path, monkeypatch):
    """Arrays are written as float64; past the byte cap each keeps a seeded sample of its rows,
    in order and the same from call to call, and the files together stay under the cap."""
    bench = load_bench()
    rows = np.arange(4000 * 8, dtype=np.float64).reshape(4000, 8)
    counts = np.arange(50, dtype=np.int32)
    bench.dump_outputs(tmp_path / "a", {"out_rows": rows, "out_counts": counts})
    got = np.load(tmp_path / "a" / "out_rows.npy")
    assert got.dtype == np.float64 and np.array_equal(got, rows)
    got_c = np.load(tmp_path / "a" / "out_counts.npy")
    assert got_c.dtype == np.float64 and np.array_equal(got_c, counts)

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 * 1000)
    for d in ("b", "c"):
        bench.dump_outputs(tmp_path / d, {"out_rows": rows, "out_counts": counts}, "_rank1")
    b = np.load(tmp_path / "b" / "out_rows_rank1.npy")
    assert 0 < b.shape[0] < rows.shape[0] and b.shape[1] == 8
    assert np.all(np.diff(b[:, 0]) > 0)  # rows of the input, in their order
    assert np.array_equal(b, rows[(b[:, 0] / 8).astype(int)])
    assert np.array_equal(b, np.load(tmp_path / "c" / "out_rows_rank1.npy"))
    assert sum(f.stat().st_size for f in (tmp_path / "b").iterdir()) <= 64 * 1000


@pytest.mark.gpu
def test_plain_run_dumps_last_timed_step(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 2 --dump-outputs DIR` on four BoT-SORT sequences:
    the line carries the headline fields and neither roofline nor CPU baseline, and the dumped
    rows and counts equal, bitwise, the last timed frame's outputs of the same workload driven
    in this process."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from tests.test_bench_workload import drive_bench

    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "2", "--seqs", "4", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64"
    assert line["roofline"] is None and line["cpu_baseline"] is None
    # 4 sequences advance one frame per step
    assert line["value"] == pytest.approx(4 * 1e3 / line["ms_per_step"], rel=1e-3)
    first, last = line["config"]["timed_frames"]
    assert last - first + 1 == 3

    rows = np.load(tmp_path / "out" / "out_rows.npy")
    counts = np.load(tmp_path / "out" / "out_counts.npy")
    assert rows.dtype == np.float64 and counts.dtype == np.float64
    assert rows.shape == (int(counts.sum()), 8) and counts.shape == (4,)

    eng, frames, outs = drive_bench(torch, "botsort", 4, last, warmup=2)
    out, cnt = outs[last - 1]
    off = frames[last - 1][1].cpu().numpy()
    cnt_h, out_h = cnt.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(counts, cnt_h)
    want = np.concatenate([out_h[off[s]: off[s] + cnt_h[s]] for s in range(4)], 0)
    assert np.array_equal(rows, want)

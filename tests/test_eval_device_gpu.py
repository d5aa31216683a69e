"""MOT evaluation of tracker rows that lie in device memory (MotEvaluator.set_gt / run_device,
bx_eval_run_device) against the host-row path (MotEvaluator.run, bx_eval_run_host), which
tests/test_eval_gpu.py pins to the numpy/scipy restatement.  The device path buckets, relabels and
orders the rows itself, so on the same rows in the same order every record must be the host
path's bit for bit: no tolerance anywhere in this file."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from boxmot_amd import evaluate_mot, evaluate_mot_device, evaluation  # noqa: E402
from test_eval_gpu import assert_identical, make_sequence  # noqa: E402

pytestmark = pytest.mark.gpu

BM = evaluation.BENCHMARKS


def same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_buffers(trs, stride=9, gap=5):
    """(rows, base, n) CUDA tensors of the sequences' rows in one buffer: sequence q's rows, then
    `gap` rows of NaN (0xFF bytes, as the feeder leaves unused rows) before the next base."""
    import torch

    total = sum(len(t) + gap for t in trs) + gap
    rows = np.frombuffer(b"\xff" * (total * stride * 8), np.float64).reshape(total, stride).copy()
    base, n, at = [], [], gap
    for t in trs:
        rows[at: at + len(t)] = t[:, :stride]
        base.append(at), n.append(len(t))
        at += len(t) + gap
    assert np.isnan(rows[0, 0])
    return (torch.from_numpy(rows).cuda(), torch.tensor(base, dtype=torch.int64).cuda(),
            torch.tensor(n, dtype=torch.int64).cuda())


def host_run(ev, frames, gts, trs, benchmark="MOT17"):
    return ev.run(frames, gts, [np.ascontiguousarray(t[:, :6]) for t in trs], BM[benchmark])


def device_run(ev, trs, n_groups=1, benchmark="MOT17", stride=9):
    return ev.run_device(*device_buffers(trs, stride), n_groups, BM[benchmark], row_stride=stride)


@pytest.fixture(scope="module")
def batch():
    """The 3 sequences x (40, 33, 27) frames x about 24 objects of test_eval_gpu."""
    gts, trs = [], []
    for k, (n, T) in enumerate(((24, 40), (20, 33), (28, 27))):
        g, t = make_sequence(10 + k, n, T)
        gts.append(g), trs.append(t)
    return np.array([40, 33, 27], np.int32), gts, trs


@pytest.fixture(scope="module")
def ev(batch):
    e = evaluation.MotEvaluator()
    e.set_gt(batch[0], batch[1])
    yield e
    e.close()


@pytest.fixture(scope="module")
def host_records(batch):
    """The host path's records of the batch, computed once and never changed."""
    e = evaluation.MotEvaluator()
    out = {bm: host_run(e, *batch, benchmark=bm) for bm in ("MOT17", "MOT20")}
    e.close()
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("stride", [9, 6])
@pytest.mark.parametrize("benchmark", ["MOT17", "MOT20"])
def test_one_group_equals_host_rows(batch, ev, host_records, benchmark, stride):
    got = device_run(ev, batch[2], 1, benchmark, stride)
    assert got.shape == (1, 4, evaluation.RECORD)
    same(got[0], host_records[benchmark])
    assert got[0, 3, evaluation.COUNT_AT] > 0  # (COMBINED Dets: something was scored)


def test_row_order_is_the_sources(batch, ev):
    rng = np.random.default_rng(77)
    trs = [t[rng.permutation(len(t))] for t in batch[2]]
    h = evaluation.MotEvaluator()
    want = host_run(h, batch[0], batch[1], trs)
    h.close()
    a, b = device_run(ev, trs), device_run(ev, trs)
    same(a[0], want)
    same(a, b)


def test_ids_negative_zero_and_large(batch, ev):
    trs = [t.copy() for t in batch[2]]
    ids = np.unique(trs[1][:, 1])
    new = dict(zip(ids, ids))
    new[ids[0]], new[ids[1]], new[ids[2]] = -3.0, 0.0, float(2 ** 40)
    trs[1][:, 1] = [new[i] for i in trs[1][:, 1]]
    have = set(trs[1][:, 1])
    assert {-3.0, 0.0, float(2 ** 40)} < have and any(100 < i < 9000 for i in have) and 9005.0 in have
    h = evaluation.MotEvaluator()
    want = host_run(h, batch[0], batch[1], trs)
    h.close()
    same(device_run(ev, trs)[0], want)


def test_groups_each_with_its_combined(batch, ev):
    frames, gts, _ = batch
    groups = []
    for k, p_keep in enumerate((0.9, 0.7, 0.5)):
        groups.append([make_sequence(10 + s, n, T, p_keep=p_keep, swaps=1 + k)[1]
                       for s, (n, T) in enumerate(((24, 40), (20, 33), (28, 27)))])
    groups[1][2] = np.empty((0, 9))                  # one sequence of group 1 without rows
    groups[2] = [np.empty((0, 9)) for _ in range(3)]  # group 2 without any
    got = device_run(ev, [t for g in groups for t in g], n_groups=3)
    assert got.shape == (3, 4, evaluation.RECORD)
    h = evaluation.MotEvaluator()
    for k in range(3):
        same(got[k], host_run(h, frames, gts, groups[k]))
    h.close()
    assert got[0].tobytes() != got[1].tobytes() and got[2, 3, evaluation.COUNT_AT] == 0


def test_row_counts_around_wave_and_block_sizes():
    g, t = make_sequence(21, 14, 30)
    big_g, big_t = make_sequence(22, 60, 45, n_fp=4)
    counts = [0, 1, 63, 64, 65, 255, 256, 257]
    assert len(t) >= 257 and len(big_t) > 2048  # (past one stride of the count's workgroups)
    frames = np.array([30] * len(counts) + [45], np.int32)
    gts = [g] * len(counts) + [big_g]
    trs = [t[:c] for c in counts] + [big_t]
    h = evaluation.MotEvaluator()
    want = host_run(h, frames, gts, trs)
    h.set_gt(frames, gts)
    same(device_run(h, trs)[0], want)
    h.close()


def test_frames_of_64_and_65_boxes():
    g, t = make_sequence(3, 70, 12, p_gt=1.0, p_keep=0.97, n_fp=6, n_fp_ids=10, swaps=3,
                         special=False)
    keep = np.ones(len(t), bool)
    for f, c in ((1, 64), (2, 65)):
        at = np.flatnonzero(t[:, 0] == f)
        assert len(at) >= c
        keep[at[c:]] = False
    t = t[keep]
    assert np.sum(t[:, 0] == 1) == 64 and np.sum(t[:, 0] == 2) == 65
    frames = np.array([12], np.int32)
    h = evaluation.MotEvaluator()
    want = host_run(h, frames, [g], [t])
    h.set_gt(frames, [g])
    same(device_run(h, [t])[0], want)
    h.close()


def test_id_capacity_exact_and_one_over():
    frames = np.array([10], np.int32)
    g, t8 = make_sequence(31, 6, 10, p_gt=1.0, p_keep=1.0, n_fp=2, n_fp_ids=2, swaps=1,
                          special=False)
    assert len(np.unique(t8[:, 1])) == 8 and len(np.unique(g[:, 1])) <= 8
    t9 = np.vstack([t8, [[10, 7777, 5.0, 5.0, 40.0, 80.0, 0.5, -1, -1]]])
    h = evaluation.MotEvaluator(max_ids=8)
    h.set_gt(frames, [g])
    want = host_run(h, frames, [g], [t8])
    same(device_run(h, [t8])[0], want)
    with pytest.raises(ValueError, match="capacity"):
        host_run(h, frames, [g], [t9])
    with pytest.raises(ValueError, match="capacity"):
        device_run(h, [t9])
    same(device_run(h, [t8])[0], want)
    h.close()
    # the largest table the handle allows: the sort's 128 KiB of LDS
    h = evaluation.MotEvaluator(max_ids=16384)
    h.set_gt(frames, [g])
    same(device_run(h, [t8])[0], want)
    h.close()


def test_box_capacity_exact_and_one_over():
    frames = np.array([10], np.int32)
    g, t = make_sequence(32, 12, 10, p_gt=1.0, p_keep=1.0, n_fp=6, n_fp_ids=8, swaps=1,
                         special=False)
    per = np.bincount(t[:, 0].astype(int), minlength=11)
    f = int(np.argmax(per))
    assert per[f] >= 16
    keep = np.ones(len(t), bool)
    for k in range(1, 11):
        keep[np.flatnonzero(t[:, 0] == k)[16:]] = False
    t16 = t[keep]
    assert np.bincount(t16[:, 0].astype(int)).max() == 16
    t17 = np.vstack([t16, [[f, 7777, 5.0, 5.0, 40.0, 80.0, 0.5, -1, -1]]])
    h = evaluation.MotEvaluator(max_boxes=16)
    h.set_gt(frames, [g])
    want = host_run(h, frames, [g], [t16])
    same(device_run(h, [t16])[0], want)
    with pytest.raises(ValueError, match="capacity"):
        host_run(h, frames, [g], [t17])
    with pytest.raises(ValueError, match="capacity"):
        device_run(h, [t17])
    same(device_run(h, [t16])[0], want)
    h.close()


def _bad(trs, what):
    trs = [t.copy() for t in trs]
    t = trs[1]
    if what == "frame 0":
        t[5, 0] = 0
    elif what == "frame T+1":
        t[5, 0] = 34
    elif what == "frame 2.5":
        t[5, 0] = 2.5
    elif what == "id 1.5":
        t[5, 1] = 1.5
    else:  # an id twice in a frame
        at = np.flatnonzero(t[:, 0] == t[5, 0])
        t[at[1], 1] = t[at[0], 1]
    return trs


@pytest.mark.parametrize("what", ["frame 0", "frame T+1", "frame 2.5", "id 1.5", "id twice"])
def test_input_errors_are_the_host_paths(batch, host_records, what):
    frames, gts, trs = batch
    bad = _bad(trs, what)
    h = evaluation.MotEvaluator()
    h.set_gt(frames, gts)
    with pytest.raises(Exception) as host_err:
        host_run(h, frames, gts, bad)
    with pytest.raises(Exception) as dev_err:
        device_run(h, bad)
    assert type(dev_err.value) is type(host_err.value) is ValueError
    assert "sequence 1" in str(dev_err.value)
    same(device_run(h, trs)[0], host_records["MOT17"])  # the handle is as good as before
    h.close()


def test_run_device_needs_gt(batch, host_records):
    h = evaluation.MotEvaluator()
    with pytest.raises(ValueError, match="ground truth"):
        device_run(h, batch[2])
    h.set_gt(batch[0], batch[1])
    same(device_run(h, batch[2])[0], host_records["MOT17"])
    # a second set_gt replaces the first
    h.set_gt(batch[0][:1], batch[1][:1])
    got = device_run(h, batch[2][:1])
    assert got.shape == (1, 2, evaluation.RECORD)
    same(got[0, 0], host_records["MOT17"][0])
    h.close()


def test_evaluate_mot_device_matches_evaluate_mot(batch):
    names = ["A", "B", "C"]
    gt = dict(zip(names, batch[1]))
    rows, base, n = device_buffers(batch[2] + [batch[2][0][:50], batch[2][1], np.empty((0, 9))])
    got = evaluate_mot_device(gt, rows, base, n, n_groups=2, seq_lengths=dict(zip(names, (40, 33, 27))))
    assert len(got) == 2
    lengths = dict(zip(names, (40, 33, 27)))
    assert_identical(got[0], evaluate_mot(gt, dict(zip(names, batch[2])), seq_lengths=lengths))
    second = {"A": batch[2][0][:50], "B": batch[2][1], "C": np.empty((0, 9))}
    assert_identical(got[1], evaluate_mot(gt, second, seq_lengths=lengths))

"""MOT evaluation on the device against the numpy/scipy restatement (tests/mot_eval_ref.py):
integer fields equal, float fields within 1e-9 absolute (the project's pinned-capture tolerance),
two runs bit-identical.

Inputs: boxmot_amd.synth tracks as gt (some identities made distractors or zero_marked = 0 rows),
and a seeded tracker built from them — jittered boxes (generic float IoUs, so the assignments'
value-carrying pairs are unique: the restatement checks that for every preprocessing, HOTA and
CLEAR assignment, see `gaps`), drops, id swaps and false positives."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import mot_eval_ref as R  # noqa: E402
from boxmot_amd import evaluate_mot, evaluation, mot_summary  # noqa: E402
from boxmot_amd.synth import SyntheticScene  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9
MIN_GAP = 1e-7  # far above both solvers' rounding (~1e-13 at these scores)


def make_sequence(seed, n_obj, n_frames, p_gt=0.92, p_keep=0.9, n_fp=2, n_fp_ids=6, swaps=2,
                  special=True):
    """(gt [n, 9], results [m, 9]) of one synthetic sequence."""
    rng = np.random.default_rng([seed, 0xE7A1])
    scene = SyntheticScene(n_obj=n_obj, seed=seed, layout="crowded", p_det=p_gt, jitter=0.0)
    cls = np.ones(n_obj, int)
    zm = np.ones(n_obj, int)
    if special:
        k = np.arange(n_obj)
        cls[k % 11 == 3], zm[k % 11 == 3] = 8, 0     # distractors
        cls[k % 13 == 5], zm[k % 13 == 5] = 2, 0
        cls[k % 17 == 7], zm[k % 17 == 7] = 6, 0     # a distractor for MOT20 only
        zm[k % 7 == 6] = 0                           # zero_marked = 0 (class as set above)
        cls[k % 19 == 9] = 3                         # another class, marked
    tid = np.arange(n_obj) + 101
    swap_at = {int(t): rng.choice(n_obj, 2, replace=False)
               for t in rng.choice(np.arange(3, max(4, n_frames - 1)), swaps, replace=False)} \
        if swaps else {}
    gt, tr = [], []
    for t in range(1, n_frames + 1):
        if t in swap_at:
            a, b = swap_at[t]
            tid[a], tid[b] = tid[b], tid[a]
        d, _, ids = scene.frame(t)
        for row, i in zip(d, ids):
            x, y, w, h = row[0], row[1], row[2] - row[0], row[3] - row[1]
            gt.append([t, i + 1, x, y, w, h, zm[i], cls[i], 1.0])
            if rng.random() < p_keep:
                j = rng.normal(0.0, 0.03, 4) * np.array([w, h, w, h])
                tr.append([t, tid[i], x + j[0], y + j[1], w + j[2], h + j[3], 0.9, -1, -1])
        for i in rng.choice(n_fp_ids, min(n_fp, n_fp_ids), replace=False) if n_fp_ids else ():
            w = rng.uniform(30, 90)
            tr.append([t, 9000 + i, rng.uniform(0, 1800), rng.uniform(0, 900), w, 2 * w, 0.5, -1, -1])
    return np.asarray(gt, float).reshape(-1, 9), np.asarray(tr, float).reshape(-1, 9)


def both(gt, tr, benchmark="MOT17", seq_lengths=None, **kw):
    """(device result, restatement result, the restatement's assignment gaps)."""
    got = evaluate_mot(gt, tr, benchmark=benchmark, seq_lengths=seq_lengths, **kw)
    gaps = []
    want = R.evaluate_ref(*evaluation.prepare_inputs(gt, tr, seq_lengths), benchmark, gaps)
    return got, want, gaps


def assert_same(got, want, path=""):
    if isinstance(want, dict):
        assert set(got) == set(want), path
        for k in want:
            assert_same(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, np.ndarray) and want.dtype.kind == "i":
        assert got.dtype.kind == "i" and np.array_equal(got, want), (path, got, want)
    elif isinstance(want, np.ndarray):
        assert np.max(np.abs(got - want)) <= TOL, (path, got, want)
    elif isinstance(want, (int, np.integer)) and not isinstance(want, bool):
        assert isinstance(got, int) and got == want, (path, got, want)
    else:
        assert abs(got - want) <= TOL, (path, got, want)


def assert_identical(a, b):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            assert_identical(a[k], b[k])
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    else:
        assert type(a) is type(b) and np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.fixture(scope="module")
def batch():
    """3 sequences x (40, 33, 27) frames x about 24 objects."""
    gt, tr = {}, {}
    for k, (n, T) in enumerate(((24, 40), (20, 33), (28, 27))):
        gt[f"SEQ-{k}"], tr[f"SEQ-{k}"] = make_sequence(10 + k, n, T)
    return gt, tr


@pytest.mark.parametrize("benchmark", ["MOT17", "MOT20"])
def test_batch_matches_restatement(batch, benchmark):
    got, want, gaps = both(*batch, benchmark=benchmark)
    assert len(gaps) > 3000 and min(gaps) > MIN_GAP
    assert want["COMBINED"]["CLEAR"]["IDSW"] > 0 and want["COMBINED"]["CLEAR"]["Frag"] > 0
    assert want["COMBINED"]["Count"]["Dets"] < sum(len(t) for t in batch[1].values())
    assert_same(got, want)
    assert_same(got["COMBINED"], want["COMBINED"])


def test_two_runs_are_bit_identical(batch):
    assert_identical(evaluate_mot(*batch), evaluate_mot(*batch))


def test_assignments_wider_than_a_wave():
    """70 gt ids x 80 tracker ids, at least 65 boxes of each side in every one of 12 frames: every
    per-frame assignment crosses the wave's 64 lanes, the Identity problem is 150 x 150."""
    g, t = make_sequence(3, 70, 12, p_gt=1.0, p_keep=0.97, n_fp=6, n_fp_ids=10, swaps=3,
                         special=False)
    for f in range(1, 13):
        assert np.sum(g[:, 0] == f) >= 65 and np.sum(t[:, 0] == f) >= 65
    got, want, gaps = both({"WIDE": g}, {"WIDE": t})
    assert want["WIDE"]["Count"]["GT_IDs"] == 70 and want["WIDE"]["Count"]["IDs"] == 80
    assert min(gaps) > MIN_GAP
    assert_same(got, want)


def test_identity_state_past_lds():
    """GT_IDs + IDs just above the LDS-resident Identity size: the solver state lives in HBM."""
    ev = evaluation.MotEvaluator()
    lds_n = ev.capacity()["lds_n"]
    ev.close()
    g, t = make_sequence(5, lds_n // 2 + 2, 3, p_gt=1.0, p_keep=1.0, n_fp=2, n_fp_ids=4, swaps=1,
                         special=False)
    got, want, gaps = both({"BIG": g}, {"BIG": t})
    n = want["BIG"]["Count"]["GT_IDs"] + want["BIG"]["Count"]["IDs"]
    assert lds_n < n <= lds_n + 8 and min(gaps) > MIN_GAP
    assert_same(got, want)


def test_degenerate_sequences_in_a_batch(batch):
    gt, tr = dict(batch[0]), dict(batch[1])
    gt["NOTRK"], tr["NOTRK"] = gt["SEQ-1"], np.empty((0, 9))
    gt["NOGT"], tr["NOGT"] = np.empty((0, 9)), tr["SEQ-2"]
    lengths = {"NOGT": 27}
    order = ["SEQ-0", "NOTRK", "SEQ-1", "NOGT", "SEQ-2"]
    gt, tr = {k: gt[k] for k in order}, {k: tr[k] for k in order}
    got, want, _ = both(gt, tr, seq_lengths=lengths)
    assert want["NOTRK"]["CLEAR"]["MLR"] == 1.0 and want["NOGT"]["CLEAR"]["CLR_FP"] == len(tr["NOGT"])
    assert_same(got, want)
    alone = evaluate_mot(*batch)
    assert_identical(got["SEQ-2"], alone["SEQ-2"])  # a sequence's record does not depend on the batch


def test_capacity_overflow_raises(batch):
    with pytest.raises(ValueError, match="capacity"):
        evaluate_mot(*batch, max_boxes=8)
    with pytest.raises(ValueError, match="capacity"):
        evaluate_mot(*batch, max_ids=4)
    with pytest.raises(ValueError, match="capacity"):
        evaluate_mot(*batch, max_frames=30)
    with pytest.raises(ValueError):
        evaluate_mot(*batch, max_boxes=5000)


def test_summary_of_bytetrack_result_files(tmp_path):
    """run_sequences("bytetrack") on two synth sequences, then the evaluation of its files."""
    from boxmot_amd import motio

    packed, gt = {}, {}
    for k in range(2):
        scene = SyntheticScene(n_obj=12 + 4 * k, seed=40 + k, layout="crowded", p_det=0.9)
        clean = SyntheticScene(n_obj=12 + 4 * k, seed=40 + k, layout="crowded", p_det=0.9,
                               jitter=0.0)
        dets, rows = [], []
        for t in range(1, 26):
            d, _, ids = scene.frame(t)
            c, _, _ = clean.frame(t)  # (same seed: the same identities, without the box noise)
            dets.append(np.column_stack([np.full(len(d), t), d]))
            rows += [[t, i + 1, b[0], b[1], b[2] - b[0], b[3] - b[1], 1, 1, 1.0]
                     for b, i in zip(c, ids)]
        packed[f"SYN-{k}"] = motio.pack_arrays(np.concatenate(dets), None, tmp_path / f"s{k}.bxmot")
        gt[f"SYN-{k}"] = tmp_path / f"gt{k}.txt"
        np.savetxt(gt[f"SYN-{k}"], np.asarray(rows), fmt="%.17g", delimiter=",")
    motio.run_sequences("bytetrack", packed, tmp_path / "exp")
    lengths = {"SYN-0": 25, "SYN-1": 25}
    got = evaluate_mot(gt, tmp_path / "exp", seq_lengths=lengths)
    gaps = []
    want = R.evaluate_ref(*evaluation.prepare_inputs(gt, tmp_path / "exp", lengths), "MOT17", gaps)
    assert want["COMBINED"]["CLEAR"]["CLR_TP"] > 100 and min(gaps) > 0.0
    assert_same(got, want)
    s, w = mot_summary(got), mot_summary(want)
    assert set(s) == {"HOTA", "AssA", "AssRe", "MOTA", "IDSW", "IDF1", "IDs"}
    for k in s:
        assert abs(s[k] - w[k]) <= 100 * TOL if isinstance(w[k], float) else s[k] == w[k]

"""The structured cases of tests/eval_cases.py through the numpy/scipy restatement alone: it
reproduces every hand-written expectation exactly, and every preprocessing, HOTA and CLEAR
assignment of every case has its value-carrying pairs fixed (gap > MIN_GAP) — the condition under
which tests/test_eval_cases_gpu.py may compare the device with it pair for pair."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import eval_cases as EC  # noqa: E402
import mot_eval_ref as R  # noqa: E402
from test_eval_gpu import MIN_GAP  # noqa: E402


@pytest.mark.parametrize("name", EC.NAMES)
def test_restatement_reproduces_the_hand_written_numbers(name):
    c = EC.case(name)
    want, gaps = EC.reference(name)
    assert set(want) == set(c.gt) | {"COMBINED"}
    EC.assert_expected(want, c.expect)
    assert len(gaps) > 0 and min(gaps) > MIN_GAP


def test_every_case_of_the_issue_is_there():
    for n in ("frame_kinds", "thresholds", "degenerate_boxes", "post_compaction_empty_MOT17",
              "post_compaction_empty_MOT20", "wide_frames_512", "wide_frames_1024", "counts_frames",
              "counts_seqs_1", "counts_seqs_65", "counts_seqs_257"):
        assert n in EC.NAMES
    assert len(set(EC.NAMES)) == len(EC.NAMES)


def test_inputs_are_small_integers():
    """What makes every IoU one correctly rounded division of exact integers."""
    for name in EC.NAMES:
        if name == "thresholds_exact":  # (its widths are the thresholds themselves)
            continue
        c = EC.case(name)
        for d in (c.gt, c.tr):
            for a in d.values():
                assert np.array_equal(a[:, :6], np.round(a[:, :6])) and np.abs(a[:, :6]).max() <= 2 ** 20


def test_frame_kinds_schedule():
    """40 frames, every ordered pair of kinds, and the four runs the expectations are worked
    out on."""
    kinds = [k[0] for k in EC.FRAME_KINDS]
    assert len(kinds) == 40
    assert {a + b for a, b in zip(kinds, kinds[1:])} == {a + b for a in "BGTN" for b in "BGTN"}
    s = " ".join(EC.FRAME_KINDS)
    for run in ("B0 T B0", "B0 G B0", "B0 T B1", "B1 G B0"):
        assert run in s
    assert (kinds.count("B"), kinds.count("G"), kinds.count("T"), kinds.count("N")) == (15, 9, 9, 7)


def test_threshold_ious_sit_where_the_case_says():
    """fl(w / 2000) against the alphas: within an ulp at 100 k, 5e-4 away at 100 k -+ 1."""
    c = EC.case("thresholds")
    g, t = c.gt["S"], c.tr["S"]
    w = t[(t[:, 1] == 1), 4]
    assert len(w) == 57 and np.array_equal(w.reshape(19, 3), 100 * np.arange(1, 20)[:, None] + [-1, 0, 1])
    iou = R.iou_xywh(g[g[:, 1] == 1][:, 2:6], t[t[:, 1] == 1][:, 2:6]).diagonal().reshape(19, 3)
    assert np.array_equal(iou, w.reshape(19, 3) / 2000.0)
    assert np.all(np.abs(iou[:, 1] - R.ALPHAS) <= R.EPS / 2)
    assert np.all(iou[:, 1] >= R.ALPHAS - R.EPS)  # (equality is a TP)
    assert np.all(iou[:, 0] < R.ALPHAS - 4e-4) and np.all(iou[:, 2] > R.ALPHAS + 4e-4)


def test_exact_threshold_ious_are_the_widths():
    """thresholds_exact: the IoU of frame t is its tracker width bit for bit, and the widths are
    alpha - eps itself, then the double just below it."""
    c = EC.case("thresholds_exact")
    iou = R.iou_xywh(c.gt["S"][:, 2:6], c.tr["S"][:, 2:6]).diagonal()
    w = np.array(EC.threshold_widths())
    assert len(w) == 32 and iou.tobytes() == w.tobytes()
    thr = R.ALPHAS - R.EPS
    assert np.array_equal(w[:17], thr[list(EC.THR_EXACT_AT)])
    below = thr[list(EC.THR_BELOW_AT)]
    assert np.all(w[17:] < below) and np.array_equal(np.nextafter(w[17:], 1.0), below)


def test_wide_frames_cross_the_capacities():
    a, b = EC.case("wide_frames_512"), EC.case("wide_frames_1024")
    per = lambda r: np.bincount(r[:, 0].astype(int))[1:].tolist()  # noqa: E731
    assert per(a.gt["A"]) == [257, 320, 1] and per(a.tr["A"]) == [257, 300, 1]
    assert per(b.gt["B"]) == [1024] and per(b.tr["B"]) == [1024] and b.max_boxes == 1024
    ious = np.unique(R.iou_xywh(b.gt["B"][:6, 2:6], b.tr["B"][:6, 2:6]).diagonal())
    assert ious.tolist() == [160 / 240, 180 / 220, 1.0]

"""The structured cases of tests/eval_cases.py on the device: evaluate_mot against the numpy/scipy
restatement (integer fields equal, float fields within test_eval_gpu's TOL, the 19-vectors and
COMBINED included), the hand-written integers of every case directly on the device result (a
restatement that drifted together with the kernels would still be caught), and the same rows
through MotEvaluator.set_gt / run_device, bit-identical to the host-row entry.
tests/test_eval_cases_host.py holds what makes the comparison meaningful: the restatement alone
meets the expectations, and every assignment's value-carrying pairs are fixed."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import eval_cases as EC  # noqa: E402
from boxmot_amd import evaluate_mot, evaluation  # noqa: E402
from test_eval_device_gpu import device_run, host_run, same  # noqa: E402
from test_eval_gpu import MIN_GAP, assert_same  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", EC.NAMES)
def test_host_rows_match_restatement_and_hand_numbers(name):
    c = EC.case(name)
    want, gaps = EC.reference(name)
    assert min(gaps) > MIN_GAP
    got = evaluate_mot(c.gt, c.tr, benchmark=c.benchmark, seq_lengths=c.lengths,
                       max_boxes=c.max_boxes)
    EC.assert_expected(got, c.expect)
    assert_same(got, want)
    assert_same(got["COMBINED"], want["COMBINED"])


@pytest.mark.parametrize("name", EC.NAMES)
def test_device_rows_equal_host_rows(name):
    c = EC.case(name)
    names = list(c.gt)
    frames = np.array([c.lengths[n] for n in names], np.int32)
    gts, trs = [c.gt[n] for n in names], [c.tr[n] for n in names]
    ev = evaluation.MotEvaluator(max_boxes=c.max_boxes)
    try:
        want = host_run(ev, frames, gts, trs, c.benchmark)
        ev.set_gt(frames, gts)
        got = device_run(ev, trs, 1, c.benchmark)
    finally:
        ev.close()
    assert got.shape == (1, len(names) + 1, evaluation.RECORD)
    same(got[0], want)
    res = {n: evaluation._unpack(got[0, k], evaluation.METRICS) for k, n in enumerate(names)}
    res["COMBINED"] = evaluation._unpack(got[0, len(names)], evaluation.METRICS)
    EC.assert_expected(res, c.expect)

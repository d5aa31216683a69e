"""MOT evaluation, CPU side: the numpy/scipy restatement (tests/mot_eval_ref.py) pinned on
hand-worked cases whose numbers are written out here, and the host layer of
boxmot_amd.evaluation (parsing, input checks, mot_summary, the C ABI's symbols)."""
import ctypes
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import eval_cases as EC  # noqa: E402
import mot_eval_ref as R  # noqa: E402
from boxmot_amd import _native as N  # noqa: E402
from boxmot_amd import evaluate_mot, evaluation, mot_summary  # noqa: E402
from eval_cases import gt_row, tr_row  # noqa: E402


def ref(gt, tr, T=None, benchmark="MOT17"):
    names, frames, gts, trs = evaluation.prepare_inputs(
        {"S": np.asarray(gt, float).reshape(-1, 9)}, {"S": np.asarray(tr, float).reshape(-1, 9)},
        {"S": T} if T else None)
    return R.evaluate_ref(names, frames, gts, trs, benchmark)


def test_perfect_tracker():
    gt, tr = EC.perfect_tracker()
    res = ref(gt, tr)
    for r in (res["S"], res["COMBINED"]):
        assert r["HOTA"]["HOTA"] == 1.0 and r["CLEAR"]["MOTA"] == 1.0 and r["Identity"]["IDF1"] == 1.0
        assert r["HOTA"]["AssA"] == 1.0 and r["HOTA"]["DetA"] == 1.0 and r["HOTA"]["LocA"] == 1.0
        assert np.array_equal(r["HOTA"]["HOTA_TP_alpha"], np.full(19, 10))
        assert r["CLEAR"]["CLR_TP"] == 10 and r["CLEAR"]["IDSW"] == 0 and r["CLEAR"]["MT"] == 2
        assert r["CLEAR"]["MOTP"] == 1.0 and r["CLEAR"]["CLR_Frames"] == 5
        assert r["Count"] == {"Dets": 10, "GT_Dets": 10, "IDs": 2, "GT_IDs": 2}


def test_id_swap_midway():
    """Two gt tracks, 10 frames; the tracker's two ids swap after frame 5.  Every box is exact."""
    gt, tr = EC.id_swap_midway()
    r = ref(gt, tr)["S"]
    c = r["CLEAR"]
    assert (c["CLR_TP"], c["CLR_FN"], c["CLR_FP"], c["IDSW"], c["Frag"]) == (20, 0, 0, 2, 0)
    assert c["MOTA"] == (20 - 0 - 2) / 20 and (c["MT"], c["PT"], c["ML"]) == (2, 0, 0)
    # Identity: each gt id shares 5 frames with either tracker id; the best one-to-one map keeps
    # 5 of each gt's 10 boxes: IDFN = IDFP = 10, IDTP = 10, IDF1 = 10 / (10 + 5 + 5)
    d = r["Identity"]
    assert (d["IDTP"], d["IDFN"], d["IDFP"]) == (10, 10, 10)
    assert d["IDF1"] == 0.5 and d["IDR"] == 0.5 and d["IDP"] == 0.5
    # HOTA: all 20 boxes are TPs at every alpha (DetA = 1); the four (gt, tracker) id pairs have
    # 5 matches each against 10 + 10 - 5 boxes: AssA = 4 * 5 * (5 / 15) / 20 = 1 / 3,
    # AssRe = AssPr = 4 * 5 * (5 / 10) / 20 = 1 / 2, HOTA = sqrt(1 / 3)
    h = r["HOTA"]
    assert h["DetA"] == 1.0 and h["LocA"] == 1.0
    assert h["AssA"] == pytest.approx(1 / 3, abs=1e-15)
    assert h["AssRe"] == pytest.approx(0.5, abs=1e-15) and h["AssPr"] == pytest.approx(0.5, abs=1e-15)
    assert h["HOTA"] == pytest.approx(math.sqrt(1 / 3), abs=1e-15)


def test_track_dropped_for_three_frames():
    gt, tr = EC.track_dropped_for_three_frames()
    c = ref(gt, tr)["S"]["CLEAR"]
    assert (c["CLR_TP"], c["CLR_FN"], c["CLR_FP"], c["IDSW"], c["Frag"]) == (17, 3, 0, 0, 1)
    assert c["MOTA"] == 17 / 20 and (c["MT"], c["PT"], c["ML"]) == (1, 1, 0)  # 7 / 10 <= 0.8
    # the same with the whole frame empty (prev_t is cleared on a frame without tracker boxes)
    gt1, tr1 = EC.whole_frames_dropped()
    c = ref(gt1, tr1)["S"]["CLEAR"]
    assert (c["CLR_TP"], c["CLR_FN"], c["Frag"], c["IDSW"]) == (7, 3, 1, 0)


def test_distractor_and_zero_marked_rows():
    """Object 1 is a pedestrian, object 2 a class-8 distractor, object 3 a class-1 row with
    zero_marked = 0; the tracker reports all three."""
    gt, tr = EC.distractor_and_zero_marked_rows()
    r = ref(gt, tr)["S"]
    # the box on the distractor is removed; the one on the unmarked pedestrian stays as an FP
    assert r["Count"] == {"Dets": 8, "GT_Dets": 4, "IDs": 2, "GT_IDs": 1}
    assert (r["CLEAR"]["CLR_TP"], r["CLEAR"]["CLR_FN"], r["CLEAR"]["CLR_FP"]) == (4, 0, 4)
    assert r["CLEAR"]["MOTA"] == 0.0
    assert (r["Identity"]["IDTP"], r["Identity"]["IDFN"], r["Identity"]["IDFP"]) == (4, 0, 4)
    assert r["HOTA"]["DetA"] == 0.5 and r["HOTA"]["AssA"] == 1.0
    # class 6 is a distractor for MOT20 only
    gt6, tr6 = EC.class6_rows()
    assert ref(gt6, tr6, benchmark="MOT17")["S"]["Count"]["Dets"] == 8
    assert ref(gt6, tr6, benchmark="MOT20")["S"]["Count"]["Dets"] == 4


def test_empty_results_and_gt_free_frames(tmp_path):
    gt = [gt_row(t, i, i) for t in range(1, 4) for i in (1, 2)]
    (tmp_path / "S.txt").write_text("")
    names, frames, gts, trs = evaluation.prepare_inputs({"S": np.asarray(gt)}, tmp_path)
    assert trs[0].shape == (0, 6) and frames[0] == 3
    r = R.evaluate_ref(names, frames, gts, trs)["S"]
    assert np.array_equal(r["HOTA"]["HOTA_FN_alpha"], np.full(19, 6)) and r["HOTA"]["LocA"] == 1.0
    assert r["HOTA"]["HOTA"] == 0.0
    c = r["CLEAR"]
    assert (c["CLR_FN"], c["ML"], c["MLR"], c["MOTA"], c["CLR_Frames"]) == (6, 2, 1.0, 0.0, 0)
    assert (r["Identity"]["IDFN"], r["Identity"]["IDTP"], r["Identity"]["IDF1"]) == (6, 0, 0.0)
    # a missing file is the same sequence
    names, frames, gts, trs2 = evaluation.prepare_inputs({"S": np.asarray(gt)}, tmp_path / "none")
    assert trs2[0].shape == (0, 6)
    # frames 4 and 5 have tracker boxes and no gt: two FPs, state untouched
    gt_again, tr = EC.gt_free_frames()
    assert gt_again == gt
    r = ref(gt, tr, T=5)["S"]
    assert (r["CLEAR"]["CLR_TP"], r["CLEAR"]["CLR_FP"], r["CLEAR"]["CLR_FN"]) == (6, 2, 0)
    assert r["CLEAR"]["MOTA"] == (6 - 2) / 6 and r["CLEAR"]["CLR_Frames"] == 5
    assert np.array_equal(r["HOTA"]["HOTA_FP_alpha"], np.full(19, 2))
    assert (r["Identity"]["IDTP"], r["Identity"]["IDFP"]) == (6, 2)
    # no gt at all
    r = ref([], tr, T=5)["S"]
    assert r["CLEAR"]["CLR_FP"] == 8 and r["CLEAR"]["MLR"] == 1.0 and r["Identity"]["IDFP"] == 8
    assert np.array_equal(r["HOTA"]["HOTA_FP_alpha"], np.full(19, 8)) and r["HOTA"]["LocA"] == 1.0


def test_comma_and_space_separators_parse_alike(tmp_path):
    rows = np.array([tr_row(t, i, i) for t in range(1, 4) for i in (1, 2)])
    rows[:, 2] += 0.25
    np.savetxt(tmp_path / "c.txt", rows, fmt="%.6f", delimiter=",")
    np.savetxt(tmp_path / "s.txt", rows, fmt="%.6f", delimiter=" ")
    a = evaluation.load_mot_rows(tmp_path / "c.txt", 7)
    b = evaluation.load_mot_rows(str(tmp_path / "s.txt"), 7)
    assert a.shape == (6, 9) and np.array_equal(a, b) and np.array_equal(a, rows)
    with pytest.raises(ValueError):
        evaluation.load_mot_rows(rows[:, :5], 7)


def test_input_errors():
    gt = [gt_row(t, i, i) for t in range(1, 4) for i in (1, 2)]
    tr = [tr_row(t, i, i) for t in range(1, 4) for i in (1, 2)]
    g, r = {"S": np.asarray(gt)}, {"S": np.asarray(tr)}
    with pytest.raises(ValueError, match="twice"):
        evaluate_mot(g, {"S": np.asarray(tr + [tr_row(2, 1, 2)])})
    with pytest.raises(ValueError, match="twice"):
        evaluate_mot({"S": np.asarray(gt + [gt_row(3, 2, 1)])}, r)
    with pytest.raises(ValueError, match="outside"):
        evaluate_mot(g, {"S": np.asarray(tr + [tr_row(4, 1, 1)])})
    with pytest.raises(ValueError, match="outside"):
        evaluate_mot(g, r, seq_lengths={"S": 2})
    with pytest.raises(ValueError, match="benchmark"):
        evaluate_mot(g, r, benchmark="MOT15")
    with pytest.raises(ValueError, match="metric"):
        evaluate_mot(g, r, metrics=("HOTA", "VACE"))


def test_evaluate_mot_runs_or_fails_loudly():
    gt = [gt_row(t, i, i) for t in range(1, 4) for i in (1, 2)]
    tr = [tr_row(t, i, i) for t in range(1, 4) for i in (1, 2)]
    try:
        res = evaluate_mot({"S": np.asarray(gt)}, {"S": np.asarray(tr)})
    except N.NativeUnavailable:
        assert N.device_count() == 0  # no fallback on a machine without a HIP device
    else:
        assert res["COMBINED"]["HOTA"]["HOTA"] == 1.0


def test_mot_summary_keys_and_scaling():
    gt = [gt_row(t, i, i) for t in range(1, 11) for i in (1, 2)]
    tr = [tr_row(t, (i if t <= 5 else 3 - i), i) for t in range(1, 11) for i in (1, 2)]
    s = mot_summary(ref(gt, tr))
    assert set(s) == {"HOTA", "AssA", "AssRe", "MOTA", "IDSW", "IDF1", "IDs"}
    assert s["MOTA"] == 90.0 and s["IDF1"] == 50.0 and s["IDSW"] == 2 and s["IDs"] == 2
    assert s["AssRe"] == pytest.approx(50.0, abs=1e-12)
    assert s["HOTA"] == pytest.approx(100 * math.sqrt(1 / 3), abs=1e-12)
    assert isinstance(s["IDSW"], int) and isinstance(s["HOTA"], float)


def test_bxeval_symbols_resolve():
    lib = ctypes.CDLL(str(N.build()))
    for name in ("bx_eval_create", "bx_eval_destroy", "bx_eval_capacity", "bx_eval_run_host"):
        assert getattr(lib, name)
        assert name in N.EXPORTS and name in (N.HEADER_EVAL).read_text()
    text = N.HEADER_EVAL.read_text()
    assert f"#define BX_EVAL_NALPHA {evaluation.N_ALPHA}" in text
    assert f"BX_EVAL_NF = {evaluation.RECORD}" in text
    assert f"BX_EVAL_CLEAR = {evaluation.CLEAR_AT}" in text
    assert f"BX_EVAL_IDENTITY = {evaluation.IDENTITY_AT}" in text
    assert f"BX_EVAL_COUNT = {evaluation.COUNT_AT}" in text

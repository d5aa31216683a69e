"""The device scoring path of boxmot_amd.tune.sweep, host side, no GPU: the combinations of
``score`` / ``keep_results`` that cannot work are refused before any engine is built, and the C
entry points the path rests on are declared in the headers."""
import re

import numpy as np
import pytest

import boxmot_amd
import boxmot_amd._native as N
from boxmot_amd import motio, tune

ROOT = N.REPO
GT = {"a": np.array([[1, 1, 10.0, 10.0, 50.0, 100.0, 1, 1, 1]])}


@pytest.fixture
def no_engine(monkeypatch):
    from boxmot_amd import engine, evaluation, tracker_zoo

    def fail(*a, **k):
        pytest.fail("an engine or an evaluator was built")

    monkeypatch.setattr(motio, "_batched_engine", fail)
    monkeypatch.setattr(tracker_zoo, "create_tracker", fail)
    monkeypatch.setattr(engine, "OcsortEngine", fail)
    monkeypatch.setattr(engine, "OcsortTableEngine", fail)
    monkeypatch.setattr(engine, "SequenceFeeder", fail)
    monkeypatch.setattr(evaluation, "MotEvaluator", fail)


@pytest.mark.parametrize("kw, match", [
    (dict(gt=GT, score="gpu"), "score must be"),
    (dict(score="device"), "gt"),
    (dict(keep_results=False), "gt"),
    (dict(gt=GT, score="device", keep_results=False, exp_dir="out"), "exp_dir"),
    (dict(gt=GT, score="host", keep_results=False), 'score="host"'),
])
def test_sweep_refuses_before_any_engine(no_engine, tmp_path, kw, match):
    if "exp_dir" in kw:
        kw = dict(kw, exp_dir=tmp_path / "out")
    with pytest.raises(ValueError, match=match):
        tune.sweep("ocsort", {"a": tmp_path / "a"}, [{}], **kw)
    assert not list(tmp_path.iterdir())


def test_device_score_needs_gt_in_the_sequences_order(no_engine, tmp_path):
    with pytest.raises(ValueError, match="same order"):
        tune.sweep("ocsort", {"a": tmp_path / "a", "b": tmp_path / "b"}, [{}],
                   gt={"b": GT["a"], "a": GT["a"]}, score="device")


def test_new_symbols_are_declared():
    feed = (ROOT / "include" / "bxfeed.h").read_text()
    ev = (ROOT / "include" / "bxeval.h").read_text()
    assert re.search(r"\bint\s+bx_feed_results_device\s*\(", feed)
    assert re.search(r"\bint\s+bx_eval_set_gt_host\s*\(", ev)
    assert re.search(r"\bint\s+bx_eval_run_device\s*\(", ev)
    for name in ("bx_feed_results_device", "bx_eval_set_gt_host", "bx_eval_run_device"):
        assert name in N.EXPORTS
    assert "evaluate_mot_device" in boxmot_amd.__all__
    assert callable(boxmot_amd.evaluate_mot_device)

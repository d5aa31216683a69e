"""boxmot_amd.tune.sweep_gsi and gsi_device, host side, no GPU: the signature, the dispatch table,
the refusals before any engine is built, the five public sweeps' signatures unchanged, the new C
symbols in header and binding table, and the whole-number argument behind ``interval <= 22``."""
import inspect
import re

import numpy as np
import pytest

import boxmot_amd
import boxmot_amd._native as N
from boxmot_amd import motio, postprocessing, tune

KW = inspect.Parameter.KEYWORD_ONLY
COMMON = ["exp_dir", "gt", "benchmark", "seq_lengths", "frame_ids"]
SWEEPS = {
    "sweep": ["tracker_type", "sequences", "configs"] + COMMON
    + ["frame_sizes", "score", "keep_results"],
    "sweep_reid": ["tracker_type", "sequences", "configs"] + COMMON
    + ["frame_sizes", "score", "keep_results", "warps"],
    "sweep_bot": ["tracker_type", "sequences", "configs"] + COMMON
    + ["score", "keep_results", "warps"],
    "sweep_boost": ["sequences", "configs"] + COMMON + ["score", "keep_results", "warps"],
    "sweep_strong": ["sequences", "configs"] + COMMON + ["score", "keep_results", "warps"],
}


@pytest.fixture
def no_engine(monkeypatch):
    """Any way to an engine fails the test (the pattern of tests/test_tune_host.py)."""
    from boxmot_amd import engine, tracker_zoo

    def fail(*a, **k):
        pytest.fail("an engine was built")

    monkeypatch.setattr(motio, "_batched_engine", fail)
    monkeypatch.setattr(tracker_zoo, "create_tracker", fail)
    for name in ("OcsortTableEngine", "TableEngine", "BoostTableEngine", "SsTableEngine",
                 "DeepOcsortTableEngine", "HybridsortTableEngine", "SequenceFeeder",
                 "SharedSequenceFeeder"):
        monkeypatch.setattr(engine, name, fail)
    monkeypatch.setattr(postprocessing, "gsi_device", fail)


def test_signature():
    sig = inspect.signature(tune.sweep_gsi).parameters
    assert list(sig) == ["tracker_type", "sequences", "configs", "interval", "tau", "sweep_kwargs"]
    assert sig["interval"].kind is KW and sig["tau"].kind is KW
    assert (sig["interval"].default, sig["tau"].default) == (20, 10)
    assert sig["sweep_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert "every sequence" in tune.sweep_gsi.__doc__.lower()  # (gsi globs MOT*.txt only)


def test_gsi_device_signature_and_export():
    sig = inspect.signature(postprocessing.gsi_device).parameters
    assert list(sig) == ["rows", "base", "n", "n_seq", "interval", "tau", "row_stride", "truncate"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, 20, 10, 9, True]
    assert boxmot_amd.gsi_device is postprocessing.gsi_device
    assert "gsi_device" in boxmot_amd.__all__


@pytest.mark.parametrize("name", list(SWEEPS))
def test_public_sweeps_keep_their_signatures(name):
    sig = inspect.signature(getattr(tune, name)).parameters
    assert list(sig) == SWEEPS[name]
    first_kw = SWEEPS[name].index("exp_dir")
    assert all(sig[k].kind is KW for k in SWEEPS[name][first_kw:])
    assert all(sig[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
               for k in SWEEPS[name][:first_kw])
    assert (sig["benchmark"].default, sig["score"].default) == ("MOT17", "host")
    assert sig["keep_results"].default is True
    assert all(sig[k].default is None for k in SWEEPS[name][first_kw:]
               if k not in ("benchmark", "score", "keep_results"))


def test_dispatch_table():
    assert tune.GSI_DISPATCH == {
        "ocsort": "sweep", "deepocsort": "sweep_reid", "hybridsort": "sweep_reid",
        "bytetrack": "sweep_bot", "botsort": "sweep_bot", "boosttrack": "sweep_boost",
        "strongsort": "sweep_strong"}
    assert tune.GSI_MAX_INTERVAL == 22
    for kind, name in tune.GSI_DISPATCH.items():
        assert callable(getattr(tune, name))


@pytest.mark.parametrize("kind", list(tune.GSI_DISPATCH))
def test_dispatch_reaches_the_trackers_own_checks(no_engine, tmp_path, kind):
    """Each tracker lands in its own sweep: that sweep's _check names itself in its refusal of
    an empty config list, and its own keyword arguments are the ones accepted."""
    seqs = {"MOT17-a": tmp_path / "a"}
    with pytest.raises(ValueError, match=rf"tune\.{tune.GSI_DISPATCH[kind]} needs at least one"):
        tune.sweep_gsi(kind, seqs, [])
    with pytest.raises(TypeError, match="no_such_argument"):
        tune.sweep_gsi(kind, seqs, [{}], no_such_argument=1)
    if tune.GSI_DISPATCH[kind] in ("sweep_bot", "sweep_boost", "sweep_strong"):
        with pytest.raises(TypeError, match="frame_sizes"):
            tune.sweep_gsi(kind, seqs, [{}], frame_sizes={})
    if kind == "ocsort":
        with pytest.raises(TypeError, match="warps"):
            tune.sweep_gsi(kind, seqs, [{}], warps={})
    assert not list(tmp_path.iterdir())


def test_refusals_before_any_engine(no_engine, tmp_path):
    seqs = {"MOT17-a": tmp_path / "a"}
    gt = {"MOT17-a": np.zeros((0, 9))}
    with pytest.raises(NotImplementedError, match="tune.sweep_gsi drives ocsort.*not imprassoc"):
        tune.sweep_gsi("imprassoc", seqs, [{}])
    with pytest.raises(ValueError, match=r"interval must not exceed 22, got 23.*whole number"):
        tune.sweep_gsi("ocsort", seqs, [{}], interval=23)
    for kind in ("ocsort", "bytetrack", "deepocsort", "boosttrack", "strongsort"):
        with pytest.raises(NotImplementedError, match="config 1: per_class"):
            tune.sweep_gsi(kind, seqs, [{}, {"per_class": True}], exp_dir=tmp_path / "out")
        with pytest.raises(ValueError, match='score="device" scores against gt'):
            tune.sweep_gsi(kind, seqs, [{}], score="device")
        with pytest.raises(ValueError, match="keep_results=False: exp_dir"):
            tune.sweep_gsi(kind, seqs, [{}], gt=gt, score="device", keep_results=False,
                           exp_dir=tmp_path / "out")
    with pytest.raises(ValueError, match="handle_occlusions"):  # (sweep_strong's own refusal)
        tune.sweep_gsi("strongsort", seqs, [{}], gt=gt, score="device")
    assert not list(tmp_path.iterdir())


def test_interval_22_is_accepted_by_the_check(no_engine, tmp_path):
    """22 passes sweep_gsi's own check and is stopped by the next one."""
    with pytest.raises(ValueError, match="needs at least one config"):
        tune.sweep_gsi("ocsort", {"MOT17-a": tmp_path / "a"}, [], interval=22)


def test_inserted_frames_are_whole_up_to_a_gap_of_21():
    """The argument behind the limit: the reference's frame of an inserted row, prev + (cur - prev)
    * (i / (cur - prev)) in float64, is a whole number for every gap an interval of 22 can fill
    (gaps up to 21) and every prev in 1..3999, and is not from a gap of 22 on (first at i = 15)."""
    prev = np.arange(1.0, 4000.0)
    for gap in range(2, 22):
        for i in range(1, gap):
            f = prev + ((prev + gap) - prev) * (i / gap)
            assert np.array_equal(f, prev + i), (gap, i)
    bad = [i for i in range(1, 22) if not np.array_equal(prev + 22.0 * (i / 22), prev + i)]
    assert bad and bad[0] == 15


def test_new_symbols_in_header_and_exports():
    text = N.HEADER_GSI.read_text()
    for sym in ("bx_gsi_device_plan", "bx_gsi_device_run", "bx_gsi_device_free"):
        assert re.search(rf"^int {sym}\(", text, re.M), sym
        assert sym in N.EXPORTS and sym in N._SIGS
    for old in ("bx_gsi_plan_workspace_bytes", "bx_gsi_interpolate_plan", "bx_gsi_interpolate",
                "bx_gsi_workspace_bytes", "bx_gsi_smooth", "bx_gsi_run_host"):
        assert re.search(rf"^int {old}\(", text, re.M) and old in N.EXPORTS

"""boxmot_amd.tune and OCSort's per-sequence parameters, host side, no GPU: the grid, the sweep's
refusals before any engine is built, the new C symbols and struct layout, and the check that the
three configs of the small sweep case tell themselves apart on the CPU oracle."""
import ctypes as C
import re

import numpy as np
import pytest

import boxmot_amd
import boxmot_amd._native as N
from boxmot_amd import motio, tune
from tests import tune_data as TD

ROOT = N.REPO


def test_grid_is_the_product_in_order():
    g = tune.grid({"max_age": [10, 30], "use_byte": [False, True], "inertia": [0.1]})
    assert g == [{"max_age": 10, "use_byte": False, "inertia": 0.1},
                 {"max_age": 10, "use_byte": True, "inertia": 0.1},
                 {"max_age": 30, "use_byte": False, "inertia": 0.1},
                 {"max_age": 30, "use_byte": True, "inertia": 0.1}]
    assert tune.grid({}) == [{}] and tune.grid({"min_hits": []}) == []
    assert boxmot_amd.tune is tune and "tune" in boxmot_amd.__all__


@pytest.fixture
def no_engine(monkeypatch):
    """Any way to an engine fails the test (the pattern of tests/test_deepocsort_flow_host.py)."""
    from boxmot_amd import engine, tracker_zoo

    def fail(*a, **k):
        pytest.fail("an engine was built")

    monkeypatch.setattr(motio, "_batched_engine", fail)
    monkeypatch.setattr(tracker_zoo, "create_tracker", fail)
    monkeypatch.setattr(engine, "OcsortEngine", fail)
    monkeypatch.setattr(engine, "OcsortTableEngine", fail)
    monkeypatch.setattr(engine, "SequenceFeeder", fail)


@pytest.mark.parametrize("kind", ["bytetrack", "botsort", "boosttrack", "strongsort", "deepocsort",
                                  "hybridsort"])
def test_sweep_refuses_other_trackers(no_engine, tmp_path, kind):
    with pytest.raises(NotImplementedError, match="ocsort"):
        tune.sweep(kind, {"a": tmp_path / "a"}, [{}], exp_dir=tmp_path / "out")
    assert not list(tmp_path.iterdir())


def test_sweep_refuses_per_class_and_differing_caps(no_engine, tmp_path):
    seqs = {"a": tmp_path / "a"}
    with pytest.raises(NotImplementedError, match="per_class"):
        tune.sweep("ocsort", seqs, [{}, {"per_class": True}])
    with pytest.raises(NotImplementedError, match="per_class"):
        tune.sweep("ocsort", seqs, [{"per_class": False}])
    for cap in ("track_cap", "det_cap"):
        with pytest.raises(ValueError, match=cap):
            tune.sweep("ocsort", seqs, [{cap: 32}, {cap: 64}])
        with pytest.raises(ValueError, match=cap):
            tune.sweep("ocsort", seqs, [{}, {cap: 32}])
    with pytest.raises(ValueError, match="at least one config"):
        tune.sweep("ocsort", seqs, [])
    assert not list(tmp_path.iterdir())


def test_resident_refusal_of_run_sequences_is_unchanged():
    assert motio.RESIDENT_TRACKERS == ("deepocsort", "hybridsort")


def test_new_symbols_and_struct_layout():
    """As tests/test_native_abi.py checks the others: declared in the header, bound with the
    header's argument lists, exported by the library; and the ctypes struct has the header's
    fields in the header's order, with C's layout (six doubles, five int32, padded to 72)."""
    text = (ROOT / "include" / "bxocsort.h").read_text()
    for name in ("bx_ocsort_set_seq_params_host", "bx_ocsort_seq_params_host"):
        assert re.search(rf"^int {name}\(", text, re.M) and name in N.EXPORTS and name in N._SIGS
    assert N._SIGS["bx_ocsort_set_seq_params_host"] == (
        [C.c_void_p, C.c_int, C.c_int, C.POINTER(N.BxOcsortSeqParams), C.c_void_p], C.c_int)
    assert N._SIGS["bx_ocsort_seq_params_host"] == (
        [C.c_void_p, C.c_int, C.POINTER(N.BxOcsortSeqParams)], C.c_int)
    m = re.search(r"typedef struct \{([^}]*)\} bx_ocsort_seq_params;", text)
    fields = []
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", m.group(1)):
        fields += [(n.strip(), C.c_double if ctype == "double" else C.c_int32)
                   for n in names.split(",")]
    assert fields == list(N.BxOcsortSeqParams._fields_)
    assert [f[0] for f in fields] == ["min_conf", "det_thresh", "asso_threshold", "inertia",
                                      "q_xy_scaling", "q_s_scaling", "max_age", "min_hits",
                                      "delta_t", "use_byte", "asso_kind"]
    assert C.sizeof(N.BxOcsortSeqParams) == 72
    assert [getattr(N.BxOcsortSeqParams, f[0]).offset for f in fields] == \
        [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64]
    # the per-sequence fields are the config's fields that size no memory
    cfg = [f[0] for f in N.BxOcsortConfig._fields_]
    assert set(cfg) - {f[0] for f in fields} == {"n_seq", "track_cap", "det_cap", "frame_w",
                                                 "frame_h"}
    lib = C.CDLL(str(N.build()))
    for name in ("bx_ocsort_set_seq_params_host", "bx_ocsort_seq_params_host"):
        assert getattr(lib, name)


def test_setter_refuses_a_null_engine():
    N.build()
    lib = N.load()
    assert lib.bx_ocsort_set_seq_params_host(None, 0, 1, None, None) == 1
    assert lib.bx_ocsort_seq_params_host(None, 0, C.byref(N.BxOcsortSeqParams())) == 1


def test_configs_resolve_as_run_sequences_resolves_them():
    a, b, c = (TD.resolved(x) for x in TD.CONFIGS)
    assert (a["det_thresh"], a["inertia"], a["use_byte"], a["asso_func"]) == (0.6, 0.1, False, "iou")
    assert (b["use_byte"], b["min_hits"], b["max_age"], b["delta_t"]) == (True, 1, 2, 1)
    assert (c["asso_func"], c["det_thresh"], c["inertia"], c["asso_threshold"]) == \
        ("giou", 0.4, 0.3, 0.2)


@pytest.fixture(scope="module")
def oracle_rows():
    """Per config and sequence the C oracle's rows [n, 9] (frame first), frame by frame as
    tests/test_oracle.py drives it; a frame without detections is not an update."""
    from oracle import pyoracle as po

    out = []
    for cfg in TD.CONFIGS:
        per_seq = []
        for s in range(TD.S):
            tr = po.OracleTracker("ocsort", **TD.resolved(cfg))
            rows = [np.empty((0, 9))]
            for t, d in enumerate(TD.scene_frames(s), 1):
                if d.shape[0]:
                    o = tr.update(d, None)
                    rows.append(np.column_stack([np.full(o.shape[0], float(t)), o]))
            per_seq.append(np.concatenate(rows))
        out.append(per_seq)
    return out


def test_the_scenes_exercise_what_the_configs_change():
    for s in range(TD.S):
        frames = TD.scene_frames(s)
        conf = np.concatenate([d[:, 4] for d in frames])
        assert len(frames) == TD.N_FRAMES[s] and max(d.shape[0] for d in frames) <= 12
        assert ((conf > 0.1) & (conf < 0.2)).any() and ((conf > 0.2) & (conf < 0.4)).any() \
            and ((conf > 0.4) & (conf < 0.6)).any() and (conf > 0.6).sum() > conf.size // 2
    assert TD.scene_frames(TD.EMPTY[0])[TD.EMPTY[1] - 1].shape[0] == 0


def test_configs_differ_on_the_oracle(oracle_rows):
    """A, B and C give pairwise different rows on every sequence: a table that applied the wrong
    entry, or none, cannot reproduce all three."""
    for s in range(TD.S):
        assert all(oracle_rows[k][s].shape[0] > 20 for k in range(TD.K))
        for i in range(TD.K):
            for j in range(i + 1, TD.K):
                a, b = oracle_rows[i][s], oracle_rows[j][s]
                assert a.shape != b.shape or not np.array_equal(a, b), (s, i, j)

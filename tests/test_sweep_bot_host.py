"""boxmot_amd.tune.sweep_bot and the per-sequence parameters of ByteTrack / BoT-SORT, host side, no
GPU: the sweep's refusals before any engine is built, what stays as it was (sweep, sweep_reid and
their tracker lists), the new C symbols and struct layout, and the check that the three configs of
the small sweep case tell themselves apart on the CPU oracle."""
import ctypes as C
import re

import numpy as np
import pytest

import boxmot_amd._native as N
from boxmot_amd import motio, tune
from tests import sweep_bot_data as BD

ROOT = N.REPO


@pytest.fixture
def no_engine(monkeypatch):
    """Any way to an engine fails the test (the pattern of tests/test_tune_host.py)."""
    from boxmot_amd import engine, tracker_zoo

    def fail(*a, **k):
        pytest.fail("an engine was built")

    monkeypatch.setattr(motio, "_batched_engine", fail)
    monkeypatch.setattr(tracker_zoo, "create_tracker", fail)
    for name in ("Engine", "TableEngine", "SequenceFeeder", "SharedSequenceFeeder"):
        monkeypatch.setattr(engine, name, fail)


def test_supported_lists():
    assert tune.SUPPORTED_BOT == ("bytetrack", "botsort")
    assert tune.SUPPORTED == ("ocsort",) and tune.SUPPORTED_REID == ("deepocsort", "hybridsort")
    assert motio.RESIDENT_TRACKERS == ("deepocsort", "hybridsort")


@pytest.mark.parametrize("kind", ["ocsort", "boosttrack", "strongsort", "deepocsort",
                                  "hybridsort", "nope"])
def test_sweep_bot_refuses_other_trackers(no_engine, tmp_path, kind):
    with pytest.raises(NotImplementedError, match="bytetrack, botsort"):
        tune.sweep_bot(kind, {"a": tmp_path / "a"}, [{}], exp_dir=tmp_path / "out")
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("kind", BD.KINDS)
def test_the_other_sweeps_still_refuse_these_trackers(no_engine, tmp_path, kind):
    with pytest.raises(NotImplementedError, match="tune.sweep drives ocsort only"):
        tune.sweep(kind, {"a": tmp_path / "a"}, [{}])
    with pytest.raises(NotImplementedError,
                       match="tune.sweep_reid drives deepocsort, hybridsort only"):
        tune.sweep_reid(kind, {"a": tmp_path / "a"}, [{}])
    with pytest.raises(NotImplementedError, match="resident=True"):
        motio.run_sequences(kind, {"a": tmp_path / "a"}, tmp_path / "out", resident=True)
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("kind", BD.KINDS)
def test_sweep_bot_refuses_per_class_caps_and_with_reid(no_engine, tmp_path, kind):
    seqs = {"a": tmp_path / "a"}
    with pytest.raises(NotImplementedError, match="per_class"):
        tune.sweep_bot(kind, seqs, [{}, {"per_class": True}])
    with pytest.raises(NotImplementedError, match="per_class"):
        tune.sweep_bot(kind, seqs, [{"per_class": False}])
    for cap in ("track_cap", "det_cap"):
        with pytest.raises(ValueError, match=cap):
            tune.sweep_bot(kind, seqs, [{cap: 32}, {cap: 64}])
        with pytest.raises(ValueError, match=cap):
            tune.sweep_bot(kind, seqs, [{}, {cap: 32}])
    with pytest.raises(ValueError, match="with_reid"):
        tune.sweep_bot(kind, seqs, [{}, {"with_reid": False}])
    with pytest.raises(ValueError, match="with_reid"):
        tune.sweep_bot(kind, seqs, [{"with_reid": True}, {"with_reid": False}])
    with pytest.raises(ValueError, match="at least one config"):
        tune.sweep_bot(kind, seqs, [])
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("kind", BD.KINDS)
def test_sweep_bot_refuses_what_check_refuses(no_engine, tmp_path, kind):
    seqs, gt = {"a": tmp_path / "a"}, {"a": np.zeros((0, 9))}
    with pytest.raises(ValueError, match="score must be one of"):
        tune.sweep_bot(kind, seqs, [{}], score="gpu")
    with pytest.raises(ValueError, match="give gt"):
        tune.sweep_bot(kind, seqs, [{}], score="device")
    with pytest.raises(ValueError, match="would return nothing"):
        tune.sweep_bot(kind, seqs, [{}], keep_results=False)
    with pytest.raises(ValueError, match="exp_dir needs the rows"):
        tune.sweep_bot(kind, seqs, [{}], gt=gt, keep_results=False, score="device",
                       exp_dir=tmp_path / "out")
    with pytest.raises(ValueError, match='score="host" needs the rows'):
        tune.sweep_bot(kind, seqs, [{}], gt=gt, keep_results=False)
    with pytest.raises(ValueError, match="same sequences in the same order"):
        tune.sweep_bot(kind, seqs, [{}], gt={"b": np.zeros((0, 9))}, score="device")
    assert not list(tmp_path.iterdir())


def test_warps_are_for_botsort(no_engine, tmp_path):
    with pytest.raises(ValueError, match="bytetrack takes no camera-motion warp"):
        tune.sweep_bot("bytetrack", {"a": tmp_path / "a"}, [{}], warps={"a": np.zeros((3, 6))})
    assert not list(tmp_path.iterdir())


def test_new_symbols_and_struct_layout():
    """As tests/test_native_abi.py checks the others: declared in the header, bound with the
    header's argument lists, exported by the library; and the ctypes struct has the header's
    fields in the header's order, with C's layout (eight doubles and three int32, the first
    int32 padded to the next double: 80 bytes)."""
    text = (ROOT / "include" / "bxassoc.h").read_text()
    for name in ("bx_engine_set_seq_params_host", "bx_engine_seq_params_host"):
        assert re.search(rf"^int {name}\(", text, re.M) and name in N.EXPORTS and name in N._SIGS
    assert N._SIGS["bx_engine_set_seq_params_host"] == (
        [C.c_void_p, C.c_int, C.c_int, C.POINTER(N.BxEngineSeqParams), C.c_void_p], C.c_int)
    assert N._SIGS["bx_engine_seq_params_host"] == (
        [C.c_void_p, C.c_int, C.POINTER(N.BxEngineSeqParams)], C.c_int)
    m = re.search(r"typedef struct \{([^}]*)\} bx_engine_seq_params;", text)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), C.c_double if ctype == "double" else C.c_int32)
                   for n in names.split(",")]
    assert fields == list(N.BxEngineSeqParams._fields_)
    assert [f[0] for f in fields] == [
        "min_conf", "track_thresh", "track_high_thresh", "track_low_thresh", "new_track_thresh",
        "proximity_thresh", "appearance_thresh", "fuse_first_associate", "match_thresh",
        "track_buffer", "frame_rate"]
    assert C.sizeof(N.BxEngineSeqParams) == 80
    assert [getattr(N.BxEngineSeqParams, f[0]).offset for f in fields] == \
        [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76]
    # the per-sequence fields are the config's fields that size no memory and pick no launches
    cfg = [f[0] for f in N.BxConfig._fields_]
    assert set(cfg) - {f[0] for f in fields} == {"kind", "n_seq", "track_cap", "det_cap",
                                                 "emb_dim", "emb_f64", "with_reid"}
    # and every EngineParams field but with_reid has its place in the struct
    from boxmot_amd.engine import EngineParams

    assert set(EngineParams.__dataclass_fields__) - {"with_reid"} == {f[0] for f in fields}
    lib = C.CDLL(str(N.build()))
    for name in ("bx_engine_set_seq_params_host", "bx_engine_seq_params_host"):
        assert getattr(lib, name)


def test_setter_refuses_a_null_engine():
    N.build()
    lib = N.load()
    assert lib.bx_engine_set_seq_params_host(None, 0, 1, None, None) == 1
    assert lib.bx_engine_seq_params_host(None, 0, C.byref(N.BxEngineSeqParams())) == 1


def test_table_engine_adds_three_methods():
    """Over Engine, TableEngine adds set_seq_params and seq_params, both inherited from the one
    _SeqTable (tests/test_sweep_boost_host.py checks all six table classes), and overrides grown."""
    from boxmot_amd.engine import Engine, TableEngine, _SeqTable

    def methods(cls):
        return {k for k in dir(cls) if callable(getattr(cls, k)) and not k.startswith("_")}

    assert issubclass(TableEngine, Engine)
    assert methods(TableEngine) - methods(Engine) == {"set_seq_params", "seq_params"}
    own = {k for k, v in vars(TableEngine).items() if callable(v) and not k.startswith("_")}
    assert own == {"grown"} and TableEngine.grown is not Engine.grown
    for m in ("set_seq_params", "seq_params"):
        assert m not in vars(TableEngine) and getattr(TableEngine, m) is getattr(_SeqTable, m)


def test_configs_resolve_as_run_sequences_resolves_them():
    a, b, c = (BD.resolved("bytetrack", x) for x in BD.configs("bytetrack"))
    assert (a["min_conf"], a["track_thresh"], a["match_thresh"], a["track_buffer"],
            a["frame_rate"]) == (0.1, 0.45, 0.8, 25, 30)
    assert (b["track_thresh"], b["match_thresh"], b["track_buffer"]) == (0.6, 0.6, 2)
    assert (c["min_conf"], c["track_thresh"], c["frame_rate"]) == (0.3, 0.35, 10)
    assert BD.resolved("bytetrack", {})["track_thresh"] == 0.6  # (no kwargs: the YAML defaults)
    a, b, c = (BD.resolved("botsort", x) for x in BD.configs("botsort"))
    assert (a["track_high_thresh"], a["new_track_thresh"], a["appearance_thresh"],
            a["proximity_thresh"], a["track_buffer"], a["with_reid"]) == \
        (0.5, 0.6, 0.25, 0.5, 30, True)
    assert (b["appearance_thresh"], b["proximity_thresh"], b["track_buffer"]) == (0.05, 0.9, 2)
    assert (c["track_high_thresh"], c["new_track_thresh"], c["fuse_first_associate"],
            c["match_thresh"]) == (0.35, 0.4, True, 0.6)
    assert BD.resolved("botsort", {})["new_track_thresh"] == 0.7


@pytest.fixture(scope="module")
def oracle_rows():
    """kind -> per config and sequence the C oracle's rows [n, 9] (frame first), frame by frame
    as tests/test_oracle.py drives it; a frame without detections is not an update."""
    from oracle import pyoracle as po

    out = {}
    for kind in BD.KINDS:
        out[kind] = []
        for cfg in BD.configs(kind):
            per_seq = []
            for s in range(BD.S):
                tr = po.OracleTracker(kind, **BD.resolved(kind, cfg))
                rows = [np.empty((0, 9))]
                for t, (d, e) in enumerate(BD.scene(s), 1):
                    if d.shape[0]:
                        o = tr.update(d, e if kind == "botsort" else None)
                        rows.append(np.column_stack([np.full(o.shape[0], float(t)), o]))
                per_seq.append(np.concatenate(rows))
            out[kind].append(per_seq)
    return out


@pytest.mark.parametrize("kind", BD.KINDS)
def test_configs_differ_on_the_oracle(oracle_rows, kind):
    """The K * S result sets are pairwise different and none is trivial: a table that applied the
    wrong entry, or none, cannot reproduce all of them."""
    sets = [oracle_rows[kind][k][s] for k in range(BD.K) for s in range(BD.S)]
    for k in range(BD.K):
        for s in range(BD.S):
            assert oracle_rows[kind][k][s].shape[0] > 2 * BD.N_FRAMES[s], (k, s)
    for i in range(len(sets)):
        for j in range(i + 1, len(sets)):
            a, b = sets[i], sets[j]
            assert a.shape != b.shape or not np.array_equal(a, b), (i, j)

"""boxmot_amd.tune.sweep_boost and the per-sequence parameters of BoostTrack, host side, no GPU: the
sweep's refusals before any engine is built, what stays as it was (the other sweeps and their
tracker lists), the new C symbols and struct layout, BoostTableEngine's checks that need no
device, and the two properties of the small sweep case on the CPU oracle: the six configs tell
themselves apart, and each of the 17 table fields changes some config's result."""
import ctypes as C
import re

import numpy as np
import pytest

import boxmot_amd._native as N
from boxmot_amd import motio, tune
from tests import sweep_boost_data as BD

ROOT = N.REPO


@pytest.fixture
def no_engine(monkeypatch):
    """Any way to an engine fails the test (the pattern of tests/test_tune_host.py)."""
    from boxmot_amd import engine, tracker_zoo

    def fail(*a, **k):
        pytest.fail("an engine was built")

    monkeypatch.setattr(motio, "_batched_engine", fail)
    monkeypatch.setattr(tracker_zoo, "create_tracker", fail)
    for name in ("BoostEngine", "BoostTableEngine", "SequenceFeeder", "SharedSequenceFeeder"):
        monkeypatch.setattr(engine, name, fail)


def test_supported_lists():
    assert tune.SUPPORTED_BOOST == ("boosttrack",)
    assert tune.SUPPORTED == ("ocsort",) and tune.SUPPORTED_REID == ("deepocsort", "hybridsort")
    assert tune.SUPPORTED_BOT == ("bytetrack", "botsort")
    assert motio.RESIDENT_TRACKERS == ("deepocsort", "hybridsort")


def test_signature():
    import inspect

    sig = inspect.signature(tune.sweep_boost).parameters
    assert list(sig) == ["sequences", "configs", "exp_dir", "gt", "benchmark", "seq_lengths",
                         "frame_ids", "score", "keep_results", "warps"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[2:])
    assert (sig["benchmark"].default, sig["score"].default) == ("MOT17", "host")
    # as sweep, sweep_reid and sweep_bot: with False the plainest call (configs and an exp_dir) is
    # one tune._check refuses
    assert sig["keep_results"].default is True
    assert all(sig[k].default is None for k in ("exp_dir", "gt", "seq_lengths", "frame_ids",
                                                "warps"))


def test_the_other_sweeps_and_the_resident_flow_still_refuse_boosttrack(no_engine, tmp_path):
    seqs = {"a": tmp_path / "a"}
    with pytest.raises(NotImplementedError, match="tune.sweep drives ocsort only"):
        tune.sweep("boosttrack", seqs, [{}])
    with pytest.raises(NotImplementedError,
                       match="tune.sweep_reid drives deepocsort, hybridsort only"):
        tune.sweep_reid("boosttrack", seqs, [{}])
    with pytest.raises(NotImplementedError, match="tune.sweep_bot drives bytetrack, botsort only"):
        tune.sweep_bot("boosttrack", seqs, [{}])
    with pytest.raises(NotImplementedError, match="resident=True"):
        motio.run_sequences("boosttrack", seqs, tmp_path / "out", resident=True)
    assert not list(tmp_path.iterdir())


def test_sweep_boost_refuses_per_class_caps_and_with_reid(no_engine, tmp_path):
    seqs = {"a": tmp_path / "a"}
    with pytest.raises(NotImplementedError, match="per_class"):
        tune.sweep_boost(seqs, [{}, {"per_class": True}])
    with pytest.raises(NotImplementedError, match="per_class"):
        tune.sweep_boost(seqs, [{"per_class": False}])
    for cap in ("track_cap", "det_cap"):
        with pytest.raises(ValueError, match=cap):
            tune.sweep_boost(seqs, [{cap: 32}, {cap: 64}])
        with pytest.raises(ValueError, match=cap):
            tune.sweep_boost(seqs, [{}, {cap: 32}])
    with pytest.raises(ValueError, match="with_reid"):
        tune.sweep_boost(seqs, [{"with_reid": True}, {"with_reid": False}])
    # as run_sequences resolves it: no kwargs are the YAML's (on), any kwargs the constructor's
    # (off)
    with pytest.raises(ValueError, match="with_reid"):
        tune.sweep_boost(seqs, [{}, {"max_age": 5}])
    with pytest.raises(ValueError, match="with_reid"):
        tune.sweep_boost(seqs, [{}, {"with_reid": False}])
    with pytest.raises(ValueError, match="at least one config"):
        tune.sweep_boost(seqs, [])
    assert not list(tmp_path.iterdir())


def test_sweep_boost_refuses_what_check_refuses(no_engine, tmp_path):
    seqs, gt = {"a": tmp_path / "a"}, {"a": np.zeros((0, 9))}
    with pytest.raises(ValueError, match="score must be one of"):
        tune.sweep_boost(seqs, [{}], score="gpu")
    with pytest.raises(ValueError, match="give gt"):
        tune.sweep_boost(seqs, [{}], score="device")
    with pytest.raises(ValueError, match="would return nothing"):
        tune.sweep_boost(seqs, [{}], keep_results=False)
    with pytest.raises(ValueError, match="exp_dir needs the rows"):
        tune.sweep_boost(seqs, [{}], gt=gt, keep_results=False, score="device",
                         exp_dir=tmp_path / "out")
    with pytest.raises(ValueError, match='score="host" needs the rows'):
        tune.sweep_boost(seqs, [{}], gt=gt, keep_results=False)
    with pytest.raises(ValueError, match="same sequences in the same order"):
        tune.sweep_boost(seqs, [{}], gt={"b": np.zeros((0, 9))}, score="device")
    assert not list(tmp_path.iterdir())


def test_with_reid_is_compared_again_after_resolving(monkeypatch, tmp_path):
    """Should the drop-in's default ever differ from what _boost_reid reads off the configs, the
    resolved parameters decide, before the table engine is built."""
    from boxmot_amd import engine
    from boxmot_amd.engine import BoostParams
    from tests import tune_data as TD

    rows = TD.packed_rows(TD.scene_frames(0)[:3])
    seqs = {"a": motio.pack_arrays(rows, None, tmp_path / "a.bxmot")}
    given = iter([True, False])
    monkeypatch.setattr(tune, "_resolve_reid",
                        lambda kind, F, cfg: (BoostParams(with_reid=next(given)), 32, 32))

    def fail(*a, **k):
        pytest.fail("an engine was built")

    monkeypatch.setattr(engine, "BoostTableEngine", fail)
    with pytest.raises(ValueError, match="with_reid resolves differently"):
        tune.sweep_boost(seqs, [{"with_reid": False}, {"with_reid": False, "max_age": 5}])


def test_warps_against_use_ecc_off(no_engine, tmp_path):
    with pytest.raises(ValueError, match="use_ecc"):
        tune.sweep_boost({"a": tmp_path / "a"}, [{"with_reid": False},
                                                 {"with_reid": False, "use_ecc": False}],
                         warps={"a": np.zeros((3, 6))})
    assert not list(tmp_path.iterdir())


def test_new_symbols_and_struct_layout():
    """As tests/test_native_abi.py checks the others: declared in the header, bound with the
    header's argument lists, exported by the library; and the ctypes struct has the header's
    fields in the header's order, with C's layout (two int32, eight doubles, seven int32, padded
    to a multiple of eight: 104 bytes)."""
    text = (ROOT / "include" / "bxboost.h").read_text()
    for name in ("bx_boost_set_seq_params_host", "bx_boost_seq_params_host"):
        assert re.search(rf"^int {name}\(", text, re.M) and name in N.EXPORTS and name in N._SIGS
    assert N._SIGS["bx_boost_set_seq_params_host"] == (
        [C.c_void_p, C.c_int, C.c_int, C.POINTER(N.BxBoostSeqParams), C.c_void_p], C.c_int)
    assert N._SIGS["bx_boost_seq_params_host"] == (
        [C.c_void_p, C.c_int, C.POINTER(N.BxBoostSeqParams)], C.c_int)
    m = re.search(r"typedef struct \{([^}]*)\} bx_boost_seq_params;", text)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), C.c_double if ctype == "double" else C.c_int32)
                   for n in names.split(",")]
    assert fields == list(N.BxBoostSeqParams._fields_)
    assert [f[0] for f in fields] == [
        "max_age", "min_hits", "det_thresh", "iou_threshold", "min_box_area",
        "aspect_ratio_thresh", "lambda_iou", "lambda_mhd", "lambda_shape", "dlo_boost_coef",
        "use_ecc", "use_dlo_boost", "use_duo_boost", "s_sim_corr", "use_rich_s", "use_sb",
        "use_vt"]
    assert C.sizeof(N.BxBoostSeqParams) == 104
    assert [getattr(N.BxBoostSeqParams, f[0]).offset for f in fields] == \
        [0, 4] + list(range(8, 72, 8)) + list(range(72, 100, 4))
    # the per-sequence fields are the config's fields that size no memory and pick no launch, in
    # the config's order
    cfg = [f[0] for f in N.BxBoostConfig._fields_]
    assert [f for f in cfg if f in dict(fields)] == [f[0] for f in fields]
    assert set(cfg) - {f[0] for f in fields} == {"n_seq", "track_cap", "det_cap", "emb_dim",
                                                 "with_reid"}
    # and every BoostParams field but with_reid has its place in the struct
    from boxmot_amd.engine import BoostParams

    assert set(BoostParams.__dataclass_fields__) - {"with_reid"} == {f[0] for f in fields}
    assert set(BD.FIELDS) == {f[0] for f in fields} and len(BD.FIELDS) == 17
    lib = C.CDLL(str(N.build()))
    for name in ("bx_boost_set_seq_params_host", "bx_boost_seq_params_host"):
        assert getattr(lib, name)


def test_setter_refuses_a_null_engine():
    N.build()
    lib = N.load()
    assert lib.bx_boost_set_seq_params_host(None, 0, 1, None, None) == 1
    assert lib.bx_boost_seq_params_host(None, 0, C.byref(N.BxBoostSeqParams())) == 1


def test_table_engine_adds_three_methods():
    """Over its base engine a table class adds set_seq_params and seq_params, both inherited from
    the one _SeqTable, and overrides grown; all six table classes do."""
    from boxmot_amd import engine as E

    def methods(cls):
        return {k for k in dir(cls) if callable(getattr(cls, k)) and not k.startswith("_")}

    assert issubclass(E.BoostTableEngine, E.BoostEngine)
    for table, base in ((E.BoostTableEngine, E.BoostEngine), (E.TableEngine, E.Engine),
                        (E.OcsortTableEngine, E.OcsortEngine), (E.SsTableEngine, E.SsEngine),
                        (E.DeepOcsortTableEngine, E.DeepOcsortEngine),
                        (E.HybridsortTableEngine, E.HybridsortEngine)):
        # (the occlusion pass lives on StrongSort's table class)
        occ = {"set_occlusion", "occlusion", "occlusion_buffer"} if table is E.SsTableEngine \
            else set()
        assert methods(table) - methods(base) == {"set_seq_params", "seq_params"} | occ, table
        own = {k for k, v in vars(table).items() if callable(v) and not k.startswith("_")}
        assert own == {"grown"} | occ and table.grown is not base.grown
        for m in ("set_seq_params", "seq_params"):
            assert m not in vars(table) and getattr(table, m) is getattr(E._SeqTable, m)


def test_with_reid_of_an_entry_must_be_the_engines():
    """Checked before the library is called: on an object without a handle."""
    from boxmot_amd.engine import BoostParams, BoostTableEngine

    e = BoostTableEngine.__new__(BoostTableEngine)
    e._h, e.n_seq, e._seq_over = None, 4, {}

    class NoCall:
        def __getattr__(self, name):
            pytest.fail(f"{name} was called")

    e._L = NoCall()
    for mine, theirs in ((True, False), (False, True)):
        e.params = BoostParams(with_reid=mine)
        with pytest.raises(ValueError, match="with_reid is engine-wide"):
            e.set_seq_params(0, [BoostParams(with_reid=mine), BoostParams(with_reid=theirs)])
    assert e._seq_over == {}


def test_configs_resolve_as_run_sequences_resolves_them():
    from boxmot_amd.engine import BoostParams

    assert BD.params_of({}) == BoostParams()  # (no kwargs: the YAML's BoostTrack++ with ReID)
    r = [BD.resolved(c) for c in BD.configs()]
    assert BD.params_of(BD.configs()[0]) == BoostParams()
    assert (r[1]["use_rich_s"], r[1]["use_sb"], r[1]["use_vt"], r[1]["dlo_boost_coef"]) == \
        (False, False, False, 1.3)
    assert (r[2]["use_dlo_boost"], r[2]["use_duo_boost"], r[2]["use_rich_s"]) == \
        (False, False, True)
    assert (r[3]["s_sim_corr"], r[3]["lambda_iou"], r[3]["lambda_mhd"], r[3]["lambda_shape"]) == \
        (True, 2.0, 1.0, 2.0)
    assert (r[4]["max_age"], r[4]["min_hits"], r[4]["det_thresh"], r[4]["iou_threshold"]) == \
        (2, 1, 0.4, 0.6)
    assert (r[5]["use_ecc"], r[5]["min_box_area"], r[5]["aspect_ratio_thresh"]) == \
        (False, 9500, 0.45)
    assert all(x["with_reid"] for x in r)
    assert not any(BD.resolved(c)["with_reid"] for c in BD.configs(reid=False))
    assert BD.resolved({"max_age": 5})["use_rich_s"] is False  # (kwargs: the constructor's)
    assert tune._boost_reid({}) and not tune._boost_reid({"max_age": 5})


def test_the_scene_is_the_tune_scene_plus_one_detection():
    from tests import sweep_reid_data as RD

    for s in range(BD.S):
        a, b = BD.scene(s), RD.scene(s)
        assert len(a) == len(b) == BD.N_FRAMES[s]
        extra = 0
        for (d, e), (d0, e0) in zip(a, b):
            assert d.shape[0] - d0.shape[0] in (0, 1) and e.shape == (d.shape[0], BD.F)
            assert np.array_equal(d[: d0.shape[0]], d0) and np.array_equal(e[: d0.shape[0]], e0)
            extra += d.shape[0] - d0.shape[0]
        assert extra > 10 and max(d.shape[0] for d, _ in a) <= 13
        assert any(d.shape[0] == 0 for d, _ in a) == (s == 1)
        w = BD.warps(s)
        assert w.shape == (BD.N_FRAMES[s], 6)
        assert not np.any(np.all(w == np.array([1.0, 0, 0, 0, 1.0, 0]), axis=1))


@pytest.fixture(scope="module")
def oracle_rows():
    """reid -> per config and sequence the C oracle's rows [n, 9] under the scene's warps."""
    return {reid: [[BD.oracle_rows(BD.resolved(c), s) for s in range(BD.S)]
                   for c in BD.configs(reid)] for reid in (True, False)}


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("reid", [True, False])
def test_configs_differ_on_the_oracle(oracle_rows, reid):
    """The K * S result sets are pairwise different and none is trivial: a table that applied the
    wrong entry, or none, cannot reproduce all of them."""
    assert BD.K >= 4
    sets = [oracle_rows[reid][k][s] for k in range(BD.K) for s in range(BD.S)]
    assert all(x.shape[0] >= 20 for x in sets)
    for i in range(len(sets)):
        for j in range(i + 1, len(sets)):
            assert not _same(sets[i], sets[j]), (i, j)


@pytest.mark.parametrize("reid", [True, False])
@pytest.mark.parametrize("field", BD.FIELDS)
def test_every_field_matters_on_the_oracle(oracle_rows, field, reid):
    """Some config changes the field, and with that one field back at the default its oracle
    result is another: a field the kernel's table did not carry would show against separate
    engines and against the oracle."""
    k = BD.FIELD_CONFIG[field]
    p = BD.resolved(BD.configs(reid)[k])
    q = dict(p, **{field: BD.defaults()[field]})
    assert p[field] != q[field]
    assert any(not _same(oracle_rows[reid][k][s], BD.oracle_rows(q, s)) for s in range(BD.S))

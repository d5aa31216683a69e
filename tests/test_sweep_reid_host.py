"""boxmot_amd.tune.sweep_reid and the per-sequence parameters of DeepOCSort and HybridSort, host
side, no GPU: every refusal of the sweep before any engine is built, tune.sweep unchanged, the new
C symbols and struct layouts, and the configs of the small sweep case as run_sequences resolves
them."""
import ctypes as C
import re

import numpy as np
import pytest

import boxmot_amd._native as N
from boxmot_amd import motio, tune
from tests import sweep_reid_data as RD

ROOT = N.REPO


@pytest.fixture
def no_engine(monkeypatch):
    """Any way to an engine fails the test (the pattern of tests/test_tune_host.py)."""
    from boxmot_amd import engine, tracker_zoo

    def fail(*a, **k):
        pytest.fail("an engine was built")

    monkeypatch.setattr(motio, "_batched_engine", fail)
    monkeypatch.setattr(tracker_zoo, "create_tracker", fail)
    for name in ("DeepOcsortEngine", "DeepOcsortTableEngine", "HybridsortEngine",
                 "HybridsortTableEngine", "OcsortEngine", "OcsortTableEngine", "SequenceFeeder",
                 "SharedSequenceFeeder"):
        monkeypatch.setattr(engine, name, fail)


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """Two packed sequences (F = 20) and one of another width."""
    N.build()
    d = tmp_path_factory.mktemp("reid_host_packed")
    out = {}
    for s in range(RD.S):
        rows, embs = RD.packed_rows(RD.scene(s)[:6])
        out[f"seq{s}"] = motio.pack_arrays(rows, embs, d / f"seq{s}.bxmot")
    rows, embs = RD.packed_rows(RD.scene(0)[:6])
    odd = motio.pack_arrays(rows, embs[:, :7].copy(), d / "odd.bxmot")
    return out, odd


@pytest.mark.parametrize("kind", ["bytetrack", "botsort", "boosttrack", "strongsort", "ocsort"])
def test_sweep_reid_refuses_other_trackers(no_engine, tmp_path, kind):
    with pytest.raises(NotImplementedError, match="deepocsort, hybridsort"):
        tune.sweep_reid(kind, {"a": tmp_path / "a"}, [{}], exp_dir=tmp_path / "out")
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("kind", ["deepocsort", "hybridsort"])
def test_sweep_still_refuses_the_reid_trackers(no_engine, tmp_path, kind):
    assert tune.SUPPORTED == ("ocsort",)
    assert tune.SUPPORTED_REID == ("deepocsort", "hybridsort")
    with pytest.raises(NotImplementedError, match="ocsort"):
        tune.sweep(kind, {"a": tmp_path / "a"}, [{}], exp_dir=tmp_path / "out")


@pytest.mark.parametrize("kind", ["deepocsort", "hybridsort"])
def test_sweep_reid_refusals_before_any_engine(no_engine, tmp_path, kind):
    seqs = {"a": tmp_path / "a"}  # (never opened: every refusal here comes first)
    with pytest.raises(NotImplementedError, match="per_class"):
        tune.sweep_reid(kind, seqs, [{}, {"per_class": True}])
    with pytest.raises(NotImplementedError, match="per_class"):
        tune.sweep_reid(kind, seqs, [{"per_class": False}])
    for cap in ("track_cap", "det_cap"):
        with pytest.raises(ValueError, match=cap):
            tune.sweep_reid(kind, seqs, [{cap: 32}, {cap: 64}])
        with pytest.raises(ValueError, match=cap):
            tune.sweep_reid(kind, seqs, [{}, {cap: 32}])
    with pytest.raises(ValueError, match="at least one config"):
        tune.sweep_reid(kind, seqs, [])
    # the score / keep_results combinations sweep refuses
    gt = {"a": np.zeros((0, 9))}
    with pytest.raises(ValueError, match="score must be"):
        tune.sweep_reid(kind, seqs, [{}], score="gpu")
    with pytest.raises(ValueError, match="give gt"):
        tune.sweep_reid(kind, seqs, [{}], score="device")
    with pytest.raises(ValueError, match="same sequences"):
        tune.sweep_reid(kind, seqs, [{}], score="device", gt={"b": gt["a"]})
    with pytest.raises(ValueError, match="without gt"):
        tune.sweep_reid(kind, seqs, [{}], keep_results=False)
    with pytest.raises(ValueError, match="exp_dir"):
        tune.sweep_reid(kind, seqs, [{}], keep_results=False, gt=gt, score="device",
                        exp_dir=tmp_path / "out")
    with pytest.raises(ValueError, match='score="host"'):
        tune.sweep_reid(kind, seqs, [{}], keep_results=False, gt=gt)
    assert not list(tmp_path.iterdir())


def test_sweep_reid_refusals_of_each_tracker(no_engine, tmp_path):
    seqs = {"a": tmp_path / "a"}
    w = {"a": np.zeros((3, 6))}
    with pytest.raises(ValueError, match="embedding_off"):
        tune.sweep_reid("deepocsort", seqs, [{}, {"embedding_off": True}])
    with pytest.raises(ValueError, match="embedding_off"):
        tune.sweep_reid("deepocsort", seqs, [{"embedding_off": False}, {"embedding_off": True}])
    for cfg in ({"cmc_off": True}, {"use_ecc": False}):
        with pytest.raises(ValueError, match="switched off"):
            tune.sweep_reid("deepocsort", seqs, [{}, cfg], warps=w)
    with pytest.raises(ValueError, match="hybridsort takes no camera-motion warp"):
        tune.sweep_reid("hybridsort", seqs, [{}], warps=w)
    with pytest.raises(NotImplementedError, match="use_byte"):
        tune.sweep_reid("hybridsort", seqs, [{}, {"use_byte": True}])
    assert not list(tmp_path.iterdir())


def test_sweep_reid_refuses_differing_embedding_widths(no_engine, packed, tmp_path):
    seqs, odd = packed
    with pytest.raises(ValueError, match=r"widths differ \(\[7, 20\]\)"):
        tune.sweep_reid("deepocsort", dict(seqs, odd=odd), [{}], exp_dir=tmp_path / "out")
    with pytest.raises(ValueError, match="no warps for seq1"):  # warps are checked as the flow's
        tune.sweep_reid("deepocsort", seqs, [{}], warps={"seq0": np.zeros((6, 6))})
    assert not list(tmp_path.iterdir())


def test_new_symbols_and_struct_layouts():
    """Declared in the headers, bound with the headers' argument lists, exported by the library;
    the ctypes structs have the headers' fields in the headers' order with C's layout; and the
    per-sequence fields are the config's fields that size no memory and decide no launch."""
    vp = C.c_void_p
    for hdr, prefix, st, name, order, size, engine_wide in (
            ("bxdeepocsort.h", "bx_deepoc", N.BxDeepocSeqParams, "bx_deepoc_seq_params",
             ["det_thresh", "iou_threshold", "inertia", "q_xy_scaling", "q_s_scaling",
              "w_association_emb", "alpha_fixed_emb", "aw_param", "max_age", "min_hits",
              "delta_t", "aw_off", "asso_kind"], 88,
             {"n_seq", "track_cap", "det_cap", "emb_dim", "embedding_off", "frame_w", "frame_h"}),
            ("bxhybridsort.h", "bx_hybrid", N.BxHybridSeqParams, "bx_hybrid_seq_params",
             ["det_thresh", "iou_threshold", "inertia", "longterm_reid_weight",
              "tcm_first_step_weight", "max_age", "min_hits", "delta_t", "asso_kind"], 56,
             {"n_seq", "track_cap", "det_cap", "emb_dim", "frame_w", "frame_h"})):
        text = (ROOT / "include" / hdr).read_text()
        setter, getter = f"{prefix}_set_seq_params_host", f"{prefix}_seq_params_host"
        for fn in (setter, getter):
            assert re.search(rf"^int {fn}\(", text, re.M) and fn in N.EXPORTS and fn in N._SIGS
        assert N._SIGS[setter] == ([vp, C.c_int, C.c_int, C.POINTER(st), vp], C.c_int)
        assert N._SIGS[getter] == ([vp, C.c_int, C.POINTER(st)], C.c_int)
        m = re.search(r"typedef struct \{([^}]*)\} " + name + ";", text)
        fields = []
        for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", m.group(1)):
            fields += [(n.strip(), C.c_double if ctype == "double" else C.c_int32)
                       for n in names.split(",")]
        assert fields == list(st._fields_) and [f[0] for f in fields] == order
        assert C.sizeof(st) == size
        cfg = N.BxDeepocConfig if prefix == "bx_deepoc" else N.BxHybridConfig
        assert {f[0] for f in cfg._fields_} - set(order) == engine_wide
    text = (ROOT / "include" / "bxfeed.h").read_text()
    assert re.search(r"^int bx_feed_create_shared\(", text, re.M)
    assert N._SIGS["bx_feed_create_shared"][0] == \
        N._SIGS["bx_feed_create"][0][:-1] + [vp, C.POINTER(vp)]
    lib = C.CDLL(str(N.build()))
    for fn in ("bx_deepoc_set_seq_params_host", "bx_deepoc_seq_params_host",
               "bx_hybrid_set_seq_params_host", "bx_hybrid_seq_params_host",
               "bx_feed_create_shared", "bx_feed_device_bytes"):
        assert getattr(lib, fn)


def test_entry_points_refuse_null_handles():
    N.build()
    lib = N.load()
    assert lib.bx_deepoc_set_seq_params_host(None, 0, 1, None, None) == 1
    assert lib.bx_deepoc_seq_params_host(None, 0, C.byref(N.BxDeepocSeqParams())) == 1
    assert lib.bx_hybrid_set_seq_params_host(None, 0, 1, None, None) == 1
    assert lib.bx_hybrid_seq_params_host(None, 0, C.byref(N.BxHybridSeqParams())) == 1
    assert lib.bx_feed_device_bytes(None, C.byref(C.c_int64())) == 1


def test_table_classes_add_only_the_table():
    """The base classes keep their method sets (tests/test_engine_api_host.py pins them); the
    table classes add set_seq_params and seq_params, and the shared feeder adds nothing."""
    from boxmot_amd import engine as E

    def public(cls):
        return {m for m in dir(cls) if not m.startswith("_") and callable(getattr(cls, m))}

    for base, table in ((E.DeepOcsortEngine, E.DeepOcsortTableEngine),
                        (E.HybridsortEngine, E.HybridsortTableEngine),
                        (E.OcsortEngine, E.OcsortTableEngine)):
        assert issubclass(table, base)
        assert public(table) - public(base) == {"set_seq_params", "seq_params"}
    assert public(E.SharedSequenceFeeder) == public(E.SequenceFeeder)


def test_configs_resolve_as_run_sequences_resolves_them():
    a, b, c = (RD.resolved("deepocsort", x) for x in RD.DEEPOC)
    assert (a["w_association_emb"], a["alpha_fixed_emb"], a["aw_param"], a["aw_off"]) == \
        (0.5, 0.95, 0.5, False)
    assert (b["w_association_emb"], b["aw_off"], b["max_age"], b["delta_t"]) == (0.0, True, 2, 1)
    assert (c["alpha_fixed_emb"], c["aw_param"], c["det_thresh"], c["asso_func"]) == \
        (0.5, 1.0, 0.4, "giou")
    a, b, c = (RD.resolved("hybridsort", x) for x in RD.HYBRID)
    assert (a["det_thresh"], a["TCM_first_step_weight"], a["longterm_reid_weight"]) == (0.3, 0, 0)
    assert (b["TCM_first_step_weight"], b["longterm_reid_weight"], b["max_age"]) == (1.0, 0.5, 2)
    assert (c["longterm_reid_weight"], c["asso_func"], c["min_hits"]) == (1.5, "giou", 1)


def test_the_scenes_carry_near_equal_rows_for_the_crossing_pair():
    for s in range(RD.S):
        base = RD.identity_rows(s)
        assert base[0] @ base[1] > 0.95 and abs(base[0] @ base[2]) < 0.6
        frames = RD.scene(s)
        assert len(frames) == RD.N_FRAMES[s]
        for d, e in frames:
            assert e.shape == (d.shape[0], RD.F) and e.dtype == np.float64
            np.testing.assert_allclose(np.linalg.norm(e, axis=1), 1.0, rtol=0, atol=1e-12)
        w = RD.frame_warps(s)
        assert w.shape == (RD.N_FRAMES[s], 6) and (np.abs(w - [1, 0, 0, 0, 1, 0]).max(1) > 0).all()
        assert np.array_equal(w, w.astype(np.float32))

"""tune.sweep_strong and the per-sequence StrongSort table without a GPU: the test configs on
the CPU oracle (they differ, every field matters, the scene enters crowd mode), the sweep's
refusals, and the ABI's names and layout.  Tracks are born Confirmed on the oracle, as under the
fork's GITHUB_ACTIONS switch: born Tentative they never reach the output."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import sweep_strong_data as SD

ROOT = Path(__file__).resolve().parents[1]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def oracle():
    return {(k, s): SD.oracle_rows(SD.resolved(c), s, born_confirmed=True)
            for k, c in enumerate(SD.CONFIGS) for s in range(SD.S)}


def test_configs_differ_pairwise(oracle):
    assert 6 <= SD.K <= 8 and all(r.shape[0] > 50 for r in oracle.values())
    for a in range(SD.K):
        for b in range(a + 1, SD.K):
            assert any(not same(oracle[a, s], oracle[b, s]) for s in range(SD.S)), (a, b)


@pytest.mark.parametrize("field", SD.FIELDS)
def test_every_field_matters(oracle, field):
    """The config that changes ``field`` gives another result with it back at the default."""
    assert set(SD.FIELD_CONFIG) == set(SD.FIELDS) and len(SD.FIELDS) == 12
    k = SD.FIELD_CONFIG[field]
    p = SD.resolved(SD.CONFIGS[k])
    assert p[field] != SD.defaults()[field]
    q = dict(p, **{field: SD.defaults()[field]})
    assert any(not same(SD.oracle_rows(q, s, born_confirmed=True), oracle[k, s])
               for s in range(SD.S))


def _oracle_fractions(params):
    """detect_crowd_situations' figure on the oracle's tracks after every update of the crowd
    sequence."""
    from oracle import pyoracle as po

    tr = po.OracleTracker("strongsort", **params, born_confirmed=True)
    # a prototype of this test's own: the shared library object's attributes stay as they are
    tracks = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_void_p)(("bxo_ss_tracks", po.lib()))
    out = []
    for d, e in SD.scene(SD.CROWD_SEQ):
        if not d.shape[0]:
            continue
        tr.update(d, e)
        ids, st = np.zeros(256, np.int32), np.zeros(256, np.int32)
        mean, cov = np.zeros((256, 8)), np.zeros((256, 64))
        n = tracks(tr.h, 256, ids.ctypes.data, st.ctypes.data, mean.ctypes.data,
                            cov.ctypes.data)
        m = mean[:n]
        w = m[:, 2] * m[:, 3]
        out.append((n, SD.crowd_fraction(
            np.column_stack([m[:, 0] - w / 2, m[:, 1] - m[:, 3] / 2, w, m[:, 3]]))))
    return out


def test_crowd_mode_entered_and_left(oracle):
    """The tracks the crowd test sees pass its threshold in the crowd stretch and not after it,
    and crowd_detection=False gives another result on that sequence only."""
    fr = _oracle_fractions(SD.resolved({}))
    assert all(n >= 3 and f > 0.3 for n, f in fr[1:len(SD.CROWD_FRAMES)])
    assert all(f <= 0.3 for _, f in fr[len(SD.CROWD_FRAMES) + 2:])
    on, off = 3, 5  # twins but for crowd_detection
    assert SD.CONFIGS[off] == dict(SD.CONFIGS[on], crowd_detection=False)
    assert not same(oracle[on, SD.CROWD_SEQ], oracle[off, SD.CROWD_SEQ])
    assert same(oracle[on, 1 - SD.CROWD_SEQ], oracle[off, 1 - SD.CROWD_SEQ])
    dflt = SD.oracle_rows(SD.resolved(dict(crowd_detection=False)), SD.CROWD_SEQ,
                          born_confirmed=True)
    assert not same(oracle[0, SD.CROWD_SEQ], dflt)  # under the default config too


def test_detections_are_float32_values():
    for s in range(SD.S):
        for d, _ in SD.scene(s):
            assert np.array_equal(d.astype(np.float32).astype(np.float64), d)


# ---------------------------------------------------------------------------- refusals
SEQS = {"seq0": "unused0.bxmot", "seq1": "unused1.bxmot"}  # never opened: refused before


@pytest.mark.parametrize("cfgs,kw,exc", [
    ([dict(handle_occlusions=False), dict()], {}, ValueError),
    ([dict(track_cap=64), dict(track_cap=128)], {}, ValueError),
    ([dict(det_cap=64), dict()], {}, ValueError),
    ([dict(vec_cap=16), dict(vec_cap=32)], {}, ValueError),
    ([dict(per_class=True)], {}, NotImplementedError),
    ([dict(cmc_off=True)], dict(warps={"seq0": np.zeros((1, 6))}), ValueError),
    ([dict()], dict(score="device", gt={"seq0": None, "seq1": None}), ValueError),
    ([dict(handle_occlusions=False)], dict(score="device"), ValueError),
    ([dict(handle_occlusions=False)], dict(score="nowhere"), ValueError),
    ([dict(handle_occlusions=False)], dict(keep_results=False), ValueError),
    ([], {}, ValueError),
])
def test_refused_before_any_engine(monkeypatch, cfgs, kw, exc):
    from boxmot_amd import engine, tune

    def no_engine(*a, **k):
        raise AssertionError("an engine was built")

    monkeypatch.setattr(engine.SsEngine, "__init__", no_engine)
    with pytest.raises(exc):
        tune.sweep_strong(SEQS, cfgs, **kw)


def test_detections_off_float32_refused_before_any_engine(monkeypatch, tmp_path):
    """A sequence packed from decimals such as 0.912 is no float32 data: the feeder would hold
    other values than run_sequences feeds, so it is refused, before any engine is built."""
    from boxmot_amd import engine, motio, tune

    rows, embs = SD.packed_rows(SD.scene(0)[:3])
    rows[0, 5] = 0.912
    seq = motio.pack_arrays(rows, embs, tmp_path / "seq.bxmot")

    def no_engine(*a, **k):
        raise AssertionError("an engine was built")

    monkeypatch.setattr(engine.SsEngine, "__init__", no_engine)
    with pytest.raises(ValueError, match="float32"):
        tune.sweep_strong({"seq": seq}, [dict(handle_occlusions=False)])


# ---------------------------------------------------------------------------- the ABI
def test_new_names_exist():
    from boxmot_amd import _native as N
    from boxmot_amd import engine, tune

    for name, hdr in (("bx_ss_set_seq_params_host", "bxstrongsort.h"),
                      ("bx_ss_seq_params_host", "bxstrongsort.h"),
                      ("bx_feed_create_shared_fmt", "bxfeed.h")):
        text = (ROOT / "include" / hdr).read_text()
        assert re.search(rf"^int {name}\(", text, re.M) and name in N.EXPORTS and name in N._SIGS
    assert issubclass(engine.SsTableEngine, engine.SsEngine)
    for m in ("set_seq_params", "seq_params", "grown"):
        assert callable(getattr(engine.SsTableEngine, m))
    assert not hasattr(engine.SsEngine, "set_seq_params")
    assert callable(tune.sweep_strong) and "bx_strongsort_tab.hip" in N.SOURCES


def test_struct_matches_header():
    """bx_ss_seq_params: the 13 fields of bx_ss_config that size no memory, in its order."""
    from boxmot_amd import _native as N

    text = (ROOT / "include" / "bxstrongsort.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} bx_ss_seq_params;", text).group(1)
    names, types = [], []
    for ty, decl in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        for nm in decl.split(","):
            names.append(nm.strip())
            types.append(C.c_double if ty == "double" else C.c_int32)
    assert names == [f for f, _ in N.BxSsSeqParams._fields_] and len(names) == 13
    assert types == [t for _, t in N.BxSsSeqParams._fields_]
    cfg = [f for f, _ in N.BxSsConfig._fields_]
    assert names == cfg[cfg.index("min_conf"):]
    assert C.sizeof(N.BxSsSeqParams) == 88

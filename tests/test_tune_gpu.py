"""OCSort's per-sequence parameter table and boxmot_amd.tune.sweep on the GPU: one engine of
K * S sequences with the table against K engines of S sequences, bit for bit; sub-range steps;
set, clear and reset; validation; the neighbouring engines; the sweep against run_sequences, file
for file; and the sweep's scores against evaluate_mot."""
from pathlib import Path

import numpy as np
import pytest

from tests import tune_data as TD

pytestmark = pytest.mark.gpu

S, K = TD.S, TD.K
GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return t


@pytest.fixture(scope="module")
def frames():
    return [TD.scene_frames(s) for s in range(S)]


def engine(n_seq, cfg=None, table=False):
    from boxmot_amd.engine import OcsortEngine, OcsortTableEngine

    cls = OcsortTableEngine if table else OcsortEngine
    return cls(n_seq=n_seq, params=TD.params_of(cfg or {}), **TD.CAPS)


def table_engine(base=None):
    """K * S sequences, sequence k * S + s under config k; the engine's own parameters are
    config `base`'s (None: A's)."""
    e = engine(K * S, base, table=True)
    for k, cfg in enumerate(TD.CONFIGS):
        e.set_seq_params(k * S, [TD.params_of(cfg)] * S)
    return e


def step(torch, eng, dets, seq0=0):
    """One frame of sequences [seq0, seq0 + len(dets)); per sequence its output rows."""
    off = np.zeros(len(dets) + 1, np.int32)
    off[1:] = np.cumsum([d.shape[0] for d in dets])
    d = torch.from_numpy(np.concatenate(dets).astype(np.float32)).cuda()
    o = torch.full((max(int(off[-1]), 1), 8), -7.0, dtype=torch.float64, device="cuda")
    c = torch.full((len(dets),), -1, dtype=torch.int32, device="cuda")
    eng.step(d, torch.from_numpy(off).cuda(), o, c, seq0=seq0, nseq=len(dets))
    torch.cuda.synchronize()
    o, c = o.cpu().numpy(), c.cpu().numpy()
    return [o[off[q]: off[q] + c[q]] for q in range(len(dets))], c


def frame_dets(frames, t):
    """Frame t (0-based) of every sequence; a sequence past its end repeats its last frame and an
    empty frame stays empty (a step with no detections is a frame of misses)."""
    return [f[min(t, len(f) - 1)] for f in frames]


def state(eng, q):
    tr = eng.tracks(q)
    return eng.counters(q), tr["id"].tolist(), tr["x"].tobytes(), tr["P"].tobytes()


@pytest.fixture(scope="module")
def separate(torch, frames):
    """The reference of tests 1-3: per config an engine of S sequences stepped over all frames;
    rows[k][t][s], counts, and the end state per (k, s)."""
    rows, end = [], []
    for cfg in TD.CONFIGS:
        e = engine(S, cfg)
        rows.append([step(torch, e, frame_dets(frames, t))[0] for t in range(max(TD.N_FRAMES))])
        assert e.status() == 0
        end.append(([state(e, s) for s in range(S)], e.frame_stats()))
        e.close()
    return rows, end


def test_table_matches_separate_engines(torch, frames, separate):
    rows, end = separate
    e = table_engine()
    differ = set()
    for t in range(max(TD.N_FRAMES)):
        got, cnt = step(torch, e, frame_dets(frames, t) * K)
        for k in range(K):
            for s in range(S):
                want = rows[k][t][s]
                assert cnt[k * S + s] == want.shape[0], (t, k, s)
                assert got[k * S + s].tobytes() == want.tobytes(), (t, k, s)
                for j in range(k):
                    if rows[j][t][s].tobytes() != want.tobytes():
                        differ.add((j, k))
    assert e.status() == 0
    for k in range(K):
        assert [state(e, k * S + s) for s in range(S)] == end[k][0]
        assert e.frame_stats(k * S, S) == end[k][1]
    assert differ == {(0, 1), (0, 2), (1, 2)}
    e.close()


def test_sub_range_steps_index_by_sequence(torch, frames, separate):
    """step(seq0=1, nseq=4) covers the second sequence of A, both of B and the first of C: a table
    indexed by the block, not by seq0 + block, gives them their neighbours' parameters."""
    rows, _ = separate
    e = table_engine()
    for t in range(12):
        d = (frame_dets(frames, t) * K)[1:5]
        got, _ = step(torch, e, d, seq0=1)
        for q in range(1, 5):
            assert got[q - 1].tobytes() == rows[q // S][t][q % S].tobytes(), (t, q)
    for q in (0, 5):
        assert e.counters(q) == {"frame_count": 0, "id_count": 0, "n_tracks": 0}
    for q in range(1, 5):
        assert e.counters(q)["frame_count"] == 12
    e.close()


def test_set_clear_and_reset(torch, frames, separate):
    rows, _ = separate
    e = table_engine(base=TD.C)
    want = [TD.params_of(c) for c in TD.CONFIGS for _ in range(S)]
    for t in range(5):
        step(torch, e, frame_dets(frames, t) * K)
    e.reset()
    assert [e.seq_params(q) for q in range(K * S)] == want  # a reset keeps the table
    assert e.counters(3) == {"frame_count": 0, "id_count": 0, "n_tracks": 0}
    for t in range(12):  # ... and the table still decides
        got, _ = step(torch, e, frame_dets(frames, t) * K)
        assert all(got[q].tobytes() == rows[q // S][t][q % S].tobytes() for q in range(K * S)), t
    e.set_seq_params(0, None, nseq=2 * S)  # A's and B's sequences back to the engine's own: C's
    e.reset()
    assert [e.seq_params(q) for q in range(K * S)] == [TD.params_of(TD.C)] * (K * S)
    for t in range(max(TD.N_FRAMES)):
        got, _ = step(torch, e, frame_dets(frames, t) * K)
        assert all(got[q].tobytes() == rows[2][t][q % S].tobytes() for q in range(K * S)), t
    e.close()
    plain = engine(1, table=True)  # clearing an engine that never had a table is not an error
    plain.set_seq_params(0, None)
    assert plain.seq_params(0) == TD.params_of(TD.A)
    plain.close()


def test_validation_changes_nothing():
    from dataclasses import replace

    from boxmot_amd import _native as N

    e = table_engine()
    before = [e.seq_params(q) for q in range(K * S)]
    ok = TD.params_of(TD.B)
    for bad in (replace(ok, delta_t=8), replace(ok, delta_t=0)):
        with pytest.raises(ValueError, match="delta_t"):
            e.set_seq_params(2, [ok, bad])  # the valid entry in front is not applied either
    with pytest.raises(ValueError, match="Invalid association mode"):
        e.set_seq_params(0, [replace(ok, asso_func="nope")])
    raw = N.BxOcsortSeqParams(delta_t=3, asso_kind=6)
    assert e._L.bx_ocsort_set_seq_params_host(e._h, 0, 1, raw, None) == 1
    raw.asso_kind = -1
    assert e._L.bx_ocsort_set_seq_params_host(e._h, 0, 1, raw, None) == 1
    for seq0, n in ((K * S - 1, 2), (-1, 1), (K * S, 1)):
        with pytest.raises(ValueError, match="range"):
            e.set_seq_params(seq0, [ok] * n)
        with pytest.raises(ValueError, match="range"):
            e.set_seq_params(seq0, None, nseq=n)
    for q in (-1, K * S):
        with pytest.raises(ValueError):
            e.seq_params(q)
    assert [e.seq_params(q) for q in range(K * S)] == before
    e.close()


def test_grown_engine_keeps_the_table():
    e = table_engine()
    g = e.grown(64, 64)
    assert type(g) is type(e)
    assert [g.seq_params(q) for q in range(K * S)] == [e.seq_params(q) for q in range(K * S)]
    e.close()
    g.close()


def test_max_obs_follows_the_sequence(torch):
    """max_age 60 on an engine created with max_age 30: a still object seen for 6 frames, missed
    for 52 and seen again.  With the engine's max_obs (50) the last box would have left the
    observation history before the object returns, and the re-update would be skipped."""
    from dataclasses import replace

    p = replace(TD.params_of(TD.A), max_age=60, min_hits=1)
    box = np.array([[500.0, 300.0, 560.0, 450.0, 0.9, 0.0]])
    far = np.array([[1500.0, 800.0, 1560.0, 950.0, 0.9, 0.0]])
    seen = lambda t: t < 6 or t >= 58  # noqa: E731
    from boxmot_amd.engine import OcsortEngine

    ref = OcsortEngine(n_seq=1, params=p, **TD.CAPS)
    e = engine(2, table=True)
    e.set_seq_params(1, [p])
    for t in range(62):
        d = [np.concatenate([box, far]) if seen(t) else far]
        want, _ = step(torch, ref, d)
        got, _ = step(torch, e, d, seq0=1)
        assert got[0].tobytes() == want[0].tobytes(), t
    assert state(e, 1) == state(ref, 0) and ref.counters(0)["id_count"] == 2
    e.close()
    ref.close()


@pytest.mark.parametrize("kind", ["deepoc", "hybrid"])
def test_neighbouring_engines_are_unaffected(torch, kind):
    """DeepOCSort and HybridSort embed the same device structure with no table: after an OCSort
    table was set in this process they still match their small golden case."""
    from tests import test_deepocsort_gpu as tdo
    from tests import test_hybridsort_gpu as thy

    e = table_engine()
    step(torch, e, [np.array([[10.0, 10.0, 60.0, 110.0, 0.9, 0.0]])] * (K * S))
    mod = tdo if kind == "deepoc" else thy
    mod.test_fixture_parity(torch, GOLDEN / f"{kind}_grid24_f20.npz")
    e.close()


# --------------------------------------------------------------------------------- the sweep
@pytest.fixture(scope="module")
def packed(frames, tmp_path_factory):
    from boxmot_amd import motio

    d = tmp_path_factory.mktemp("tune_packed")
    return {f"seq{s}": motio.pack_arrays(TD.packed_rows(frames[s]), None, d / f"seq{s}.bxmot")
            for s in range(S)}


@pytest.fixture(scope="module")
def loop(torch, packed, tmp_path_factory):
    """The loop the sweep replaces: run_sequences once per config (with the caps as kwargs)."""
    from boxmot_amd import motio

    root = tmp_path_factory.mktemp("tune_loop")
    for k, cfg in enumerate(TD.CONFIGS):
        motio.run_sequences("ocsort", packed, root / f"{k:04d}", tracker_kwargs=cfg)
    return root


def test_sweep_resolves_configs_as_run_sequences(torch):
    from boxmot_amd import tune

    for cfg in TD.CONFIGS:
        p, tc, dc = tune._resolve(cfg)
        assert p == TD.params_of(cfg) and (tc, dc) == (256, 256)
    # (with the caps A is no longer empty: the constructor's defaults, as in run_sequences)
    for cfg in (dict(c, **TD.CAPS) for c in TD.CONFIGS):
        p, tc, dc = tune._resolve(cfg)
        assert p == TD.params_of(cfg) and (tc, dc) == (32, 32)
    assert tune._resolve(dict(TD.CAPS))[0] != tune._resolve({})[0]


def test_sweep_files_match_run_sequences(torch, packed, loop, tmp_path):
    """Byte-identical files, with a frame without detections in one sequence (TD.EMPTY) and
    sequences of different lengths (TD.N_FRAMES); the returned arrays hold the files' values."""
    from boxmot_amd import tune

    res = tune.sweep("ocsort", packed, TD.CONFIGS, exp_dir=tmp_path)
    assert [r["config"] for r in res] == TD.CONFIGS and all(r["summary"] is None for r in res)
    texts = []
    for k in range(K):
        for nm in packed:
            got = (tmp_path / f"{k:04d}" / f"{nm}.txt").read_bytes()
            assert got == (loop / f"{k:04d}" / f"{nm}.txt").read_bytes(), (k, nm)
            assert len(got) > 500
            texts.append(got)
            rows = res[k]["results"][nm]
            file_rows = np.loadtxt(tmp_path / f"{k:04d}" / f"{nm}.txt", delimiter=",", ndmin=2)
            assert rows.dtype == np.float64 and rows.shape == file_rows.shape
            np.testing.assert_array_equal(rows[:, :8], file_rows[:, :8])
            np.testing.assert_array_equal([float("%.6f" % c) for c in rows[:, 8]], file_rows[:, 8])
    assert len(set(texts)) == K * S
    assert sorted(p.name for p in tmp_path.iterdir()) == ["0000", "0001", "0002"]


def test_sweep_honours_frame_ids_and_caps(torch, packed, tmp_path):
    """frame_ids as in run_sequences (a sub-range of one sequence), caps given in every config."""
    from boxmot_amd import motio, tune

    fids = {"seq0": list(range(5, 30))}
    cfgs = [dict(c, **TD.CAPS) for c in TD.CONFIGS[1:]]
    tune.sweep("ocsort", packed, cfgs, exp_dir=tmp_path / "sweep", frame_ids=fids,
               frame_sizes={"seq1": (1280, 720)})
    for k, cfg in enumerate(cfgs):
        motio.run_sequences("ocsort", packed, tmp_path / "loop" / f"{k:04d}", frame_ids=fids,
                            frame_sizes={"seq1": (1280, 720)}, tracker_kwargs=cfg)
        for nm in packed:
            assert (tmp_path / "sweep" / f"{k:04d}" / f"{nm}.txt").read_bytes() == \
                (tmp_path / "loop" / f"{k:04d}" / f"{nm}.txt").read_bytes(), (k, nm)


def test_sweep_scores_match_evaluate_mot(torch, packed, loop):
    from boxmot_amd import evaluate_mot, mot_summary, tune

    gt = {f"seq{s}": TD.synthetic_gt(s) for s in range(S)}
    res = tune.sweep("ocsort", packed, TD.CONFIGS, gt=gt)
    summaries = []
    for k in range(K):
        want = mot_summary(evaluate_mot(gt, loop / f"{k:04d}"))
        assert res[k]["summary"] == want, k
        assert want["HOTA"] > 5.0
        summaries.append(tuple(want.values()))
    assert len(set(summaries)) == K

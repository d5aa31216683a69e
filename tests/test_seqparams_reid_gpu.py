"""The per-sequence parameter tables of DeepOCSort and HybridSort on the GPU: round trip and
validation; one table engine of K * S sequences against K * S separate engines, bit for bit, with
sub-range steps mixed in (and, for DeepOCSort, under a warp per frame); max_obs following the
sequence's max_age; and set-then-cleared against never set over the small golden case."""
import ast
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

from tests import sweep_reid_data as RD

pytestmark = pytest.mark.gpu

S, K, F = RD.S, RD.K, RD.F
GOLDEN = Path(__file__).resolve().parent / "golden"
KINDS = ["deepocsort", "hybridsort"]
STATE = {"deepocsort": ("x", "P", "emb"),
         "hybridsort": ("x", "P", "emb", "bank_mean", "vel", "bank_count")}


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return t


@pytest.fixture(scope="module")
def scenes():
    return [RD.scene(s) for s in range(S)]


def classes(kind):
    from boxmot_amd import _native as N
    from boxmot_amd import engine as E

    if kind == "deepocsort":
        return E.DeepOcsortEngine, E.DeepOcsortTableEngine, N.BxDeepocSeqParams, "bx_deepoc"
    return E.HybridsortEngine, E.HybridsortTableEngine, N.BxHybridSeqParams, "bx_hybrid"


def engine(kind, n_seq, cfg=None, table=False, emb_dim=F):
    cls = classes(kind)[1 if table else 0]
    return cls(n_seq=n_seq, emb_dim=emb_dim, params=RD.params_of(kind, cfg or {}), **RD.CAPS)


def table_engine(kind, base=None):
    """K * S sequences, sequence k * S + s under config k; the engine's own parameters are config
    `base`'s (None: the first's)."""
    e = engine(kind, K * S, base, table=True)
    for k, cfg in enumerate(RD.CONFIGS[kind]):
        e.set_seq_params(k * S, [RD.params_of(kind, cfg)] * S)
    return e


def step(torch, kind, eng, frames, seq0=0, warps=None):
    """One frame of sequences [seq0, seq0 + len(frames)) from (dets, embs) pairs; per sequence its
    output rows.  warps: [len(frames), 6] or None (DeepOCSort only)."""
    off = np.zeros(len(frames) + 1, np.int32)
    off[1:] = np.cumsum([d.shape[0] for d, _ in frames])
    pad = 0 if off[-1] else 1  # (a frame without any detection still hands over valid pointers)
    d = torch.from_numpy(np.concatenate([d for d, _ in frames] + [np.zeros((pad, 6))])
                         .astype(np.float32)).cuda()
    e = torch.from_numpy(np.ascontiguousarray(
        np.concatenate([e for _, e in frames] + [np.zeros((pad, F))]), np.float64)).cuda()
    o = torch.full((max(int(off[-1]), 1), 8), -7.0, dtype=torch.float64, device="cuda")
    c = torch.full((len(frames),), -1, dtype=torch.int32, device="cuda")
    od = torch.from_numpy(off).cuda()
    if kind == "deepocsort":
        w = None if warps is None else torch.from_numpy(np.ascontiguousarray(warps)).cuda()
        eng.step(d, od, e, w, o, c, seq0=seq0, nseq=len(frames))
    else:
        eng.step(d, od, e, o, c, seq0=seq0, nseq=len(frames))
    torch.cuda.synchronize()
    o, c = o.cpu().numpy(), c.cpu().numpy()
    return [o[off[q]: off[q] + c[q]] for q in range(len(frames))]


def frame_of(scenes, t):
    """Frame t (0-based) of every sequence; a sequence past its end repeats its last frame."""
    return [sc[min(t, len(sc) - 1)] for sc in scenes]


def warps_at(t):
    return np.stack([RD.frame_warps(s)[min(t, RD.N_FRAMES[s] - 1)] for s in range(S)])


def state(kind, eng, q):
    tr = eng.tracks(q)
    return (eng.counters(q), tr["id"].tolist()) + tuple(tr[k].tobytes() for k in STATE[kind])


CASES = [("deepocsort", False), ("deepocsort", True), ("hybridsort", False)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: c[0] + ("-warp" if c[1] else ""))
def separate(request, torch, scenes):
    """Per (config, sequence) a plain one-sequence engine created with the config, stepped over
    all frames: rows[k][s][t] and the end state."""
    kind, warp = request.param
    rows, end = [], []
    for cfg in RD.CONFIGS[kind]:
        rows.append([])
        end.append([])
        for s in range(S):
            e = engine(kind, 1, cfg)
            got = []
            for t in range(max(RD.N_FRAMES)):
                w = warps_at(t)[s: s + 1] if warp else None
                got.append(step(torch, kind, e, [frame_of(scenes, t)[s]], warps=w)[0])
            assert e.status() == 0
            rows[-1].append(got)
            end[-1].append(state(kind, e, 0))
            e.close()
    return kind, warp, rows, end


def test_table_matches_separate_engines(torch, scenes, separate):
    """Whole launches and, two frames in three, the same frame as two sub-range launches
    (seq0 != 0, nseq < K * S): a table indexed by the block instead of seq0 + block gives the
    second launch's sequences their neighbours' parameters."""
    kind, warp, rows, end = separate
    e = table_engine(kind)
    differ = set()
    for t in range(max(RD.N_FRAMES)):
        fr = frame_of(scenes, t) * K
        w = np.tile(warps_at(t), (K, 1)) if warp else None
        cut = (0, 1, 4)[t % 3]  # 0: one launch; else [0, cut) then [cut, K * S)
        got = []
        for a, b in ((0, K * S),) if not cut else ((0, cut), (cut, K * S)):
            got += step(torch, kind, e, fr[a:b], seq0=a, warps=None if w is None else w[a:b])
        for k in range(K):
            for s in range(S):
                want = rows[k][s][t]
                assert got[k * S + s].shape == want.shape, (t, k, s)
                assert got[k * S + s].tobytes() == want.tobytes(), (t, k, s)
                differ |= {(j, k) for j in range(k) if rows[j][s][t].tobytes() != want.tobytes()}
    assert e.status() == 0
    for k in range(K):
        assert [state(kind, e, k * S + s) for s in range(S)] == end[k], k
    assert sum(r.shape[0] for r in rows[0][0]) > 100
    assert differ == {(0, 1), (0, 2), (1, 2)}  # the three configs tell themselves apart
    e.close()


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_reset_and_copy(torch, scenes, kind):
    base = RD.CONFIGS[kind][2]
    e = table_engine(kind, base=base)
    want = [RD.params_of(kind, c) for c in RD.CONFIGS[kind] for _ in range(S)]
    assert [e.seq_params(q) for q in range(K * S)] == want
    for t in range(4):
        step(torch, kind, e, frame_of(scenes, t) * K)
    e.reset()
    assert [e.seq_params(q) for q in range(K * S)] == want  # a reset keeps the table
    assert e.counters(3)["frame_count"] == 0 and e.counters(3)["n_tracks"] == 0
    # a state copy carries tracks only: the plain class's grown() leaves the new engine's
    # sequences on its own parameters, the table class's sets the table again
    plain_cls, table_cls = classes(kind)[:2]
    g = plain_cls.grown(e, 160, 64)
    probe = table_cls.seq_params
    assert [probe(g, q) for q in range(K * S)] == [RD.params_of(kind, base)] * (K * S)
    g.close()
    g = e.grown(160, 64)
    assert type(g) is type(e) and [g.seq_params(q) for q in range(K * S)] == want
    g.close()
    e.set_seq_params(S, None, nseq=S)  # NULL clears a range: config 1's sequences
    assert [e.seq_params(q) for q in range(K * S)] == \
        want[:S] + [RD.params_of(kind, base)] * S + want[2 * S:]
    e.close()
    plain = engine(kind, 1, table=True)  # clearing an engine that never had a table is no error
    plain.set_seq_params(0, None)
    assert plain.seq_params(0) == RD.params_of(kind, {})
    plain.close()


@pytest.mark.parametrize("kind", KINDS)
def test_validation_changes_nothing(kind):
    e = table_engine(kind)
    raw_cls, prefix = classes(kind)[2:]
    setter = getattr(e._L, prefix + "_set_seq_params_host")
    before = [e.seq_params(q) for q in range(K * S)]
    ok = RD.params_of(kind, RD.CONFIGS[kind][1])
    for bad in (replace(ok, delta_t=8), replace(ok, delta_t=0)):
        with pytest.raises(ValueError, match="delta_t"):
            e.set_seq_params(2, [ok, bad])  # the valid entry in front is not applied either
    with pytest.raises(ValueError, match="Invalid association mode"):
        e.set_seq_params(0, [replace(ok, asso_func="nope")])
    for kind_id in (6, -1):
        raw = raw_cls(delta_t=3, asso_kind=kind_id)
        assert setter(e._h, 0, 1, raw, None) == 1
    if kind == "hybridsort":  # bx_hybrid_create refuses a negative det_thresh
        with pytest.raises(ValueError, match="det_thresh"):
            e.set_seq_params(0, [replace(ok, det_thresh=-0.1)])
    else:
        with pytest.raises(ValueError, match="embedding_off"):
            e.set_seq_params(0, [replace(ok, embedding_off=True)])
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


@pytest.mark.parametrize("kind", KINDS)
def test_max_obs_follows_the_sequence(torch, kind):
    """max_age 60 on an engine created with max_age 30: a still object seen for 6 frames, missed
    for 55 and seen again.  With the engine's max_obs (50) the last box would have left the
    observation history before the object returns, and the re-update would be skipped."""
    p = replace(RD.params_of(kind, {}), max_age=60, min_hits=1)
    box = np.array([[500.0, 300.0, 560.0, 450.0, 0.9, 0.0]])
    far = np.array([[1500.0, 800.0, 1560.0, 950.0, 0.9, 0.0]])
    emb = np.eye(F)[:2]
    seen = lambda t: t < 6 or t >= 61  # noqa: E731
    ref = classes(kind)[0](n_seq=1, emb_dim=F, params=p, **RD.CAPS)
    e = engine(kind, 2, table=True)
    e.set_seq_params(1, [p])
    for t in range(65):
        fr = [(np.concatenate([box, far]), emb) if seen(t) else (far, emb[1:])]
        want = step(torch, kind, ref, fr)
        got = step(torch, kind, e, fr, seq0=1)
        assert got[0].tobytes() == want[0].tobytes(), t
    assert state(kind, e, 1) == state(kind, ref, 0)
    assert len(ref.tracks(0)["id"]) == 2 and ref.counters(0)["id_count"] == 3  # (ids from 1)
    e.close()
    ref.close()


@pytest.mark.parametrize("kind", KINDS)
def test_set_then_cleared_equals_never_set(torch, kind):
    """The small golden case through update_host: a sequence whose entry was set and cleared, its
    neighbour whose entry is still set, and a plain engine.  The first and the last agree bit for
    bit and with the reference-captured rows; the neighbour's other parameters do not leak."""
    from tests.golden_util import compare_outputs
    from tests.scenes import scene_of

    stem = "deepoc" if kind == "deepocsort" else "hybrid"
    with np.load(GOLDEN / f"{stem}_grid24_f20.npz") as fx:
        args = ast.literal_eval(str(fx["tracker_args"]))
        assert "warp_seed" not in fx.files
        scene, nf, ref = scene_of(fx), int(fx["n_frames"]), fx["outputs"]
    p = RD.params_of(kind, args)
    other = replace(p, max_age=1, min_hits=1, inertia=0.9, iou_threshold=0.6)
    plain_cls, table_cls = classes(kind)[:2]
    caps = dict(track_cap=64, det_cap=64)
    plain = plain_cls(n_seq=1, emb_dim=20, params=p, **caps)
    e = table_cls(n_seq=2, emb_dim=20, params=p, **caps)
    e.set_seq_params(0, [other, other])
    e.set_seq_params(0, None, nseq=1)
    rows, differs = [], False
    for t in range(1, nf + 1):
        d, em, _ = scene.frame(t)
        want = plain.update_host(0, d, em)
        got = e.update_host(0, d, em)
        assert got.tobytes() == want.tobytes(), t
        differs |= e.update_host(1, d, em).tobytes() != want.tobytes()
        rows.append(np.concatenate([np.full((got.shape[0], 1), float(t)), got], 1))
    assert differs and state(kind, e, 0) == state(kind, plain, 0)
    compare_outputs(np.concatenate(rows), ref, box_atol=1e-9)
    e.close()
    plain.close()

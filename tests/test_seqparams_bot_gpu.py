"""The per-sequence parameter table of bx_engine (ByteTrack, BoT-SORT) on the GPU: one TableEngine
of K * S sequences against K plain engines of S sequences, bit for bit, over every kernel that reads
a parameter (the three cosine kernels, the fixed-width builds, under warps, without ReID); against
the CPU oracle; chunked launches; both association builds and the scheduling modes; max_time_lost
following the sequence; round trip, reset, copy; validation; and set-then-cleared against never
set."""
from dataclasses import replace

import numpy as np
import pytest

from tests import sweep_bot_data as BD
from tests import sweep_reid_data as RD

pytestmark = pytest.mark.gpu

S, K = BD.S, BD.K
T = max(BD.N_FRAMES)


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return t


class Case:
    """kind, feature width, embedding type, warps, ReID: what an engine of the case is built
    with and fed."""

    def __init__(self, name, kind, F=0, f64=True, warp=False, reid=True):
        self.name, self.kind, self.F, self.f64, self.warp = name, kind, F, f64, warp
        self.reid = kind == "botsort" and reid
        self.extra = {} if kind == "bytetrack" or reid else {"with_reid": False}

    def params(self, cfg):
        return BD.params_of(self.kind, dict(cfg, **self.extra))

    def configs(self):
        return [self.params(c) for c in BD.configs(self.kind)]

    def engine(self, n_seq, params, table=False, **caps):
        from boxmot_amd import engine as E

        cls = E.TableEngine if table else E.Engine
        return cls(self.kind, n_seq=n_seq, emb_dim=self.F if self.reid else 0, emb_f64=self.f64,
                   params=params, **(caps or BD.CAPS))

    def table_engine(self, base=0):
        """K * S sequences, sequence k * S + s under config k; the engine's own parameters are
        config `base`'s."""
        e = self.engine(K * S, self.configs()[base], table=True)
        for k, p in enumerate(self.configs()):
            e.set_seq_params(k * S, [p] * S)
        return e

    def scenes(self):
        if self.F not in _SCENES:
            _SCENES[self.F] = [BD.scene(s, self.F or RD.F) for s in range(S)]
        return _SCENES[self.F]


_SCENES = {}
BYTE = Case("bytetrack", "bytetrack")
BOT20 = Case("botsort-f20-f64", "botsort", 20)            # cosine_kernel_any
BOT32 = Case("botsort-f32-f64", "botsort", 32)            # the chunked rows kernel, F at run time
BOT512 = Case("botsort-f512-f32", "botsort", 512, f64=False)  # the fixed-width builds of K1, K1c
BOTWARP = Case("botsort-f20-warp", "botsort", 20, warp=True)
BOTNOREID = Case("botsort-noreid", "botsort", 20, reid=False)
CASES = [BYTE, BOT20, BOT32, BOT512, BOTWARP, BOTNOREID]


def frame_of(case, t):
    """Frame t (0-based) of every sequence; a sequence past its end repeats its last frame."""
    return [sc[min(t, len(sc) - 1)] for sc in case.scenes()]


def warps_at(t):
    return np.stack([RD.frame_warps(s)[min(t, RD.N_FRAMES[s] - 1)] for s in range(S)])


def step(torch, case, eng, frames, seq0=0, warps=None):
    """One frame of sequences [seq0, seq0 + len(frames)) from (dets, embs) pairs; per sequence its
    output rows.  The inputs are complete before the step is called and untouched until the device
    is idle again: what overlap mode and early-features mode ask of the caller."""
    off = np.zeros(len(frames) + 1, np.int32)
    off[1:] = np.cumsum([d.shape[0] for d, _ in frames])
    pad = 0 if off[-1] else 1  # (a frame without any detection still hands over valid pointers)
    d = torch.from_numpy(np.concatenate([d for d, _ in frames] + [np.zeros((pad, 6))])
                         .astype(np.float32)).cuda()
    e = None
    if case.reid:
        e = torch.from_numpy(np.ascontiguousarray(
            np.concatenate([e for _, e in frames] + [np.zeros((pad, case.F))]),
            np.float64 if case.f64 else np.float32)).cuda()
    w = None if warps is None else torch.from_numpy(np.ascontiguousarray(warps)).cuda()
    o = torch.full((max(int(off[-1]), 1), 8), -7.0, dtype=torch.float64, device="cuda")
    c = torch.full((len(frames),), -1, dtype=torch.int32, device="cuda")
    od = torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    eng.step(d, od, e, w, o, c, seq0=seq0, nseq=len(frames))
    torch.cuda.synchronize()
    o, c = o.cpu().numpy(), c.cpu().numpy()
    return [o[off[q]: off[q] + c[q]] for q in range(len(frames))]


def state(eng, q):
    tr = eng.tracks(q)
    return (eng.counters(q), tr["id"].tolist(), tr["state"].tolist(), tr["frame_id"].tolist(),
            tr["mean"].tobytes(), tr["covariance"].tobytes())


def run(torch, case, eng, n_cfg, cuts=None, n_frames=T):
    """Step `eng` (n_cfg * S sequences, each config's block fed the S scenes) over the frames;
    rows[q][t] and every sequence's end state.  cuts(t): launch boundaries inside (0, n_cfg * S),
    none for one launch."""
    n = n_cfg * S
    rows = [[] for _ in range(n)]
    for t in range(n_frames):
        fr = frame_of(case, t) * n_cfg
        w = np.tile(warps_at(t), (n_cfg, 1)) if case.warp else None
        edges = [0] + list(cuts(t) if cuts else ()) + [n]
        got = []
        for a, b in zip(edges[:-1], edges[1:]):
            got += step(torch, case, eng, fr[a:b], seq0=a, warps=None if w is None else w[a:b])
        for q in range(n):
            rows[q].append(got[q])
    assert eng.status() == 0
    return rows, [state(eng, q) for q in range(n)]


_CACHE = {}


def separate(torch, case):
    """The reference of every test here, computed once per case and left unchanged: K plain
    engines of S sequences, one per config, stepped frame by frame."""
    key = ("separate", case.name)
    if key not in _CACHE:
        rows, end = [], []
        for p in case.configs():
            e = case.engine(S, p)
            r, st = run(torch, case, e, 1)
            e.close()
            rows += r
            end += st
        _CACHE[key] = (rows, end)
    return _CACHE[key]


def table(torch, case):
    """One TableEngine of K * S sequences, one launch per frame."""
    key = ("table", case.name)
    if key not in _CACHE:
        e = case.table_engine()
        _CACHE[key] = run(torch, case, e, K)
        e.close()
    return _CACHE[key]


def same(got, want):
    for q, (a, b) in enumerate(zip(got[0], want[0])):
        for t, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (q, t)
    assert got[1] == want[1]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_table_matches_separate_engines(torch, case):
    got, want = table(torch, case), separate(torch, case)
    same(got, want)
    rows = want[0]
    assert all(sum(r.shape[0] for r in rows[q]) > 2 * BD.N_FRAMES[q % S] for q in range(K * S))
    whole = [b"".join(r.tobytes() for r in rows[q]) for q in range(K * S)]
    assert len(set(whole)) == K * S  # the configs tell themselves apart on every sequence


@pytest.mark.parametrize("case", [BYTE, BOT20], ids=lambda c: c.name)
def test_table_matches_the_oracle(torch, case):
    """Every table sequence against the CPU oracle created with that sequence's config: a table
    that every sequence ignored would pass the comparison above whenever configs agree."""
    from oracle import pyoracle as po

    rows = table(torch, case)[0]
    for k, cfg in enumerate(BD.configs(case.kind)):
        for s in range(S):
            orc = po.OracleTracker(case.kind, **BD.resolved(case.kind, cfg))
            for t in range(T):
                d, e = frame_of(case, t)[s]
                want = orc.update(d, e if case.reid else None)
                np.testing.assert_array_equal(rows[k * S + s][t], want, err_msg=f"{k} {s} {t}")


@pytest.mark.parametrize("case", [BYTE, BOT20, BOT512], ids=lambda c: c.name)
def test_chunked_launches(torch, case):
    """Two launches per frame whose boundary cuts through a config's block (seq0 != 0, nseq <
    K * S): an override indexed by the block instead of seq0 + block gives the second launch's
    sequences their neighbours' parameters."""
    e = case.table_engine()
    got = run(torch, case, e, K, cuts=lambda t: [S + 1] if t % 2 else [1, 2 * S + 1])
    e.close()
    same(got, table(torch, case))


@pytest.mark.parametrize("case", [BYTE, BOT20], ids=lambda c: c.name)
def test_both_association_builds(torch, case):
    for mode in (0, 1):
        e = case.table_engine()
        e.force_assoc_build(mode)
        got = run(torch, case, e, K)
        e.close()
        same(got, table(torch, case))


@pytest.mark.parametrize("case", [BOT20, BOT512], ids=lambda c: c.name)
def test_overlap_and_early_features(torch, case):
    e = case.table_engine()
    e.set_overlap(True)
    e.set_early_features(True)
    got = run(torch, case, e, K)
    e.close()
    same(got, table(torch, case))


@pytest.mark.parametrize("case", [BYTE, BOTNOREID], ids=lambda c: c.name)
def test_max_time_lost_follows_the_sequence(torch, case):
    """An engine created with track_buffer 30; sequence 0 gets track_buffer 2, sequence 1 the same
    max_time_lost through frame_rate ((int)(15 / 30.0 * 4) = 2), sequence 2 stays on the engine's.
    A track seen in frames 1..3 is lost from frame 4; at frame 6 it has been lost for 3 frames,
    more than 2: sequences 0 and 1 mark it removed in that frame and, as the reference subtracts
    the removed tracks of earlier frames only (bytetrack.py:278-289), list it no more from frame
    7; sequence 2 still lists it as lost."""
    base = replace(case.configs()[0], track_buffer=30, frame_rate=30)
    e = case.engine(3, base, table=True)
    e.set_seq_params(0, [replace(base, track_buffer=2),
                         replace(base, track_buffer=4, frame_rate=15)])
    box = np.array([[500.0, 300.0, 560.0, 450.0, 0.9, 0.0]])
    far = np.array([[1500.0, 800.0, 1560.0, 950.0, 0.9, 0.0]])
    none = np.zeros((0, 20))
    lost, last = [], []
    for t in range(1, 9):
        d = np.concatenate([box, far]) if t <= 3 else far
        step(torch, case, e, [(d, none)] * 3)
        lost.append([e.counters(q)["n_lost"] for q in range(3)])
        last.append([e.tracks(q)["state"].tolist()[-1] for q in range(3)])
        assert [e.counters(q)["n_active"] for q in range(3)] == [2 if t <= 3 else 1] * 3, t
    assert lost == [[0, 0, 0]] * 3 + [[1, 1, 1]] * 3 + [[0, 0, 1]] * 2
    # frames 4 and 5: lost everywhere; frame 6: removed where the buffer is 2
    assert last[3] == last[4] == [last[3][2]] * 3 == last[5][2:] * 3
    assert last[5][0] == last[5][1] != last[5][2]
    assert [len(e.tracks(q)["id"]) for q in range(3)] == [1, 1, 2]
    assert e.tracks(2)["frame_id"].tolist() == [8, 3]
    e.close()


@pytest.mark.parametrize("case", [BYTE, BOT20], ids=lambda c: c.name)
def test_round_trip_reset_and_copy(torch, case):
    from boxmot_amd import engine as E

    e = case.table_engine(base=2)
    base = case.configs()[2]
    want = [p for p in case.configs() for _ in range(S)]
    assert [e.seq_params(q) for q in range(K * S)] == want
    for t in range(4):
        step(torch, case, e, frame_of(case, t) * K)
    e.reset()
    assert [e.seq_params(q) for q in range(K * S)] == want  # a reset keeps the table
    assert e.counters(3)["frame_count"] == 0 and e.counters(3)["n_active"] == 0
    for t in range(4):
        step(torch, case, e, frame_of(case, t) * K)
    # a state copy carries tracks only: the plain class's grown() leaves the new engine's
    # sequences on its own parameters, the table class's sets the table again
    g = E.Engine.grown(e, 160, 64)
    assert type(g) is E.Engine
    assert [E.TableEngine.seq_params(g, q) for q in range(K * S)] == [base] * (K * S)
    g.close()
    g = e.grown(160, 64)
    assert type(g) is E.TableEngine and [g.seq_params(q) for q in range(K * S)] == want
    assert (g.track_cap, g.det_cap) == (160, 64)
    for t in range(4, 8):  # the grown engine goes on as the table engine does
        fr = frame_of(case, t) * K
        a, b = step(torch, case, e, fr), step(torch, case, g, fr)
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b], t
        sep = separate(torch, case)[0]
        assert [x.tobytes() for x in a] == [sep[q][t].tobytes() for q in range(K * S)], t
    g.close()
    e.set_seq_params(S, None, nseq=S)  # NULL clears a range: config 1's sequences
    assert [e.seq_params(q) for q in range(K * S)] == want[:S] + [base] * S + want[2 * S:]
    e.close()
    plain = case.engine(1, case.configs()[0], table=True)
    plain.set_seq_params(0, None)  # clearing an engine that never had a table is no error
    assert plain.seq_params(0) == case.configs()[0]
    plain.close()


@pytest.mark.parametrize("case", [BYTE, BOT20], ids=lambda c: c.name)
def test_validation_changes_nothing(torch, case):
    from boxmot_amd import _native as N

    e = case.table_engine()
    before = [e.seq_params(q) for q in range(K * S)]
    ok = case.configs()[1]
    for bad, what in ((replace(ok, track_buffer=-1), "track_buffer"),
                      (replace(ok, frame_rate=0), "frame_rate"),
                      (replace(ok, frame_rate=-30), "frame_rate")):
        with pytest.raises(ValueError, match=what):
            e.set_seq_params(2, [ok, bad])  # the valid entry in front is not applied either
    for seq0, n in ((K * S - 1, 2), (-1, 1), (K * S, 1)):
        with pytest.raises(ValueError, match="range"):
            e.set_seq_params(seq0, [ok] * n)
        with pytest.raises(ValueError, match="range"):
            e.set_seq_params(seq0, None, nseq=n)
    with pytest.raises(ValueError, match="range"):
        e.set_seq_params(1, None, nseq=2 ** 31 - 1)  # (seq0 + nseq would wrap)
    raw = N.BxEngineSeqParams(track_buffer=1, frame_rate=30)
    assert e._L.bx_engine_set_seq_params_host(e._h, 1, 2 ** 31 - 1, raw, None) == 1
    assert e._L.bx_engine_set_seq_params_host(e._h, 0, -1, raw, None) == 1
    for q in (-1, K * S):
        with pytest.raises(ValueError):
            e.seq_params(q)
    assert [e.seq_params(q) for q in range(K * S)] == before
    got = run(torch, case, e, K, n_frames=12)
    want = separate(torch, case)[0]
    for q in range(K * S):
        assert [r.tobytes() for r in got[0][q]] == [r.tobytes() for r in want[q][:12]], q
    e.close()


@pytest.mark.parametrize("case", [BYTE, BOT20], ids=lambda c: c.name)
def test_set_then_cleared_equals_never_set(torch, case):
    """A sequence whose entry was set and cleared, its neighbour whose entry is still set, and the
    plain engines: the first agrees with never set bit for bit, the neighbour's other parameters
    do not leak, and the neighbour runs on them."""
    a, b = case.configs()[0], case.configs()[1]
    e = case.engine(2 * S, a, table=True)
    e.set_seq_params(0, [b] * (2 * S))
    e.set_seq_params(0, None, nseq=S)
    got = run(torch, case, e, 2)
    e.close()
    want = separate(torch, case)
    same(([r for r in got[0]], got[1]), ([r for r in want[0][: 2 * S]], want[1][: 2 * S]))
    assert any(x.tobytes() != y.tobytes() for x, y in zip(want[0][0], want[0][S]))

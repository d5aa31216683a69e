"""The per-sequence parameter table of bx_boost (BoostTrack) on the GPU: one BoostTableEngine of
K * S sequences against K plain BoostEngines of S sequences, rows and track state bit for bit on
every frame, with ReID, without, under warps (with use_ecc off in the engine and on in entries and
the other way round), at the capacities whose cost matrix spills to HBM, and through
update_classes_host; against the CPU oracle; chunked launches; the confidence table growing with
an entry's max_age; round trip, reset, copy, grown; validation; set-then-cleared against never
set."""
from dataclasses import replace

import numpy as np
import pytest

from tests import sweep_boost_data as BD

pytestmark = pytest.mark.gpu

S, K, F = BD.S, BD.K, BD.F
T = max(BD.N_FRAMES)
# bx_boost_create: above 768 sequences a workgroup's LDS is capped at 40 KB and the frame's track
# rows stay in HBM (tb_lds off); 384 track slots leave the cost matrix 86 entries of LDS
# (cost_lds), so every frame with 13 detections and 7 tracks or more takes cost_g / e_g.  The
# smallest such setting: 352 slots leave 470 entries, which these scenes' frames (at most 13 x 30)
# mostly fit.
HBM = dict(n_seq=769, track_cap=384, det_cap=32)


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return t


class Case:
    """ReID, warps, capacities and which config the table engine itself is created with."""

    def __init__(self, name, reid=True, warp=False, base=0, caps=None):
        self.name, self.reid, self.warp, self.base = name, reid, warp, base
        self.caps = dict(caps or BD.CAPS)
        self.n_seq = self.caps.pop("n_seq", None)

    def configs(self):
        return [BD.params_of(c) for c in BD.configs(self.reid)]

    def engine(self, n_seq, params, table=False):
        from boxmot_amd import engine as E

        cls = E.BoostTableEngine if table else E.BoostEngine
        return cls(n_seq=self.n_seq or n_seq, emb_dim=F if self.reid else 0, params=params,
                   **self.caps)

    def table_engine(self):
        """Sequence k * S + s runs under config k; the engine's own parameters are config
        `base`'s."""
        e = self.engine(K * S, self.configs()[self.base], table=True)
        for k, p in enumerate(self.configs()):
            e.set_seq_params(k * S, [p] * S)
        return e


REID = Case("reid-f20")
NOREID = Case("noreid", reid=False)
# the engine's own use_ecc is off (config 5) and the entries of configs 0-4 switch it on
WARP = Case("reid-warp", warp=True, base=5)
# the engine's own config is the plain BoostTrack: e_g exists only because entries ask for it
HBM_REID = Case("hbm-reid-warp", warp=True, base=1, caps=HBM)
HBM_NOREID = Case("hbm-noreid", reid=False, caps=HBM)
CASES = [REID, NOREID, WARP, HBM_REID, HBM_NOREID]

_SCENES = [BD.scene(s) for s in range(S)]


def frame_of(t):
    """Frame t (0-based) of every sequence; a sequence past its end repeats its last frame."""
    return [sc[min(t, len(sc) - 1)] for sc in _SCENES]


def warps_at(t):
    return np.stack([BD.warps(s)[min(t, BD.N_FRAMES[s] - 1)] for s in range(S)])


def step(torch, case, eng, frames, seq0=0, warps=None):
    """One frame of sequences [seq0, seq0 + len(frames)) from (dets, embs) pairs; per sequence its
    output rows."""
    off = np.zeros(len(frames) + 1, np.int32)
    off[1:] = np.cumsum([d.shape[0] for d, _ in frames])
    pad = 0 if off[-1] else 1  # (a frame without any detection still hands over valid pointers)
    d = torch.from_numpy(np.concatenate([d for d, _ in frames] + [np.zeros((pad, 6))])
                         .astype(np.float32)).cuda()
    e = None
    if case.reid:
        e = torch.from_numpy(np.ascontiguousarray(
            np.concatenate([e for _, e in frames] + [np.zeros((pad, F))]), np.float64)).cuda()
    w = None if warps is None else torch.from_numpy(np.ascontiguousarray(warps)).cuda()
    o = torch.full((max(int(off[-1]), 1), 8), -7.0, dtype=torch.float64, device="cuda")
    c = torch.full((len(frames),), -1, dtype=torch.int32, device="cuda")
    od = torch.from_numpy(off).cuda()
    eng.step(d, od, e, w, o, c, seq0=seq0, nseq=len(frames))
    torch.cuda.synchronize()
    o, c = o.cpu().numpy(), c.cpu().numpy()
    return [o[off[q]: off[q] + c[q]] for q in range(len(frames))]


def state(eng, q):
    """counters and tracks() of sequence q as bytes."""
    tr = eng.tracks(q)
    return (tuple(sorted(eng.counters(q).items())),) + tuple(
        np.ascontiguousarray(tr[k]).tobytes() for k in sorted(tr))


def run(torch, case, eng, n_cfg, cuts=None, frames=range(T), states=True):
    """Step `eng` (its first n_cfg * S sequences, each config's block fed the S scenes) over the
    frames; rows[q][t] and state[q][t] after every frame.  cuts: launch boundaries inside
    (0, n_cfg * S), none for one launch."""
    n = n_cfg * S
    rows, st = [[] for _ in range(n)], [[] for _ in range(n)]
    for t in frames:
        fr = frame_of(t) * n_cfg
        w = np.tile(warps_at(t), (n_cfg, 1)) if case.warp else None
        edges = [0] + list(cuts or ()) + [n]
        got = []
        for a, b in zip(edges[:-1], edges[1:]):
            got += step(torch, case, eng, fr[a:b], seq0=a, warps=None if w is None else w[a:b])
        for q in range(n):
            rows[q].append(got[q])
            if states:
                st[q].append(state(eng, q))
    assert eng.status() == 0
    return rows, st


_CACHE = {}


def separate(torch, case):
    """The reference of the tests here, computed once per case and left unchanged: K plain
    engines, one per config, stepped frame by frame."""
    key = ("separate", case.name)
    if key not in _CACHE:
        rows, st = [], []
        for p in case.configs():
            e = case.engine(S, p)
            r, s = run(torch, case, e, 1)
            e.close()
            rows += r
            st += s
        _CACHE[key] = (rows, st)
    return _CACHE[key]


def table(torch, case):
    """One BoostTableEngine, the K * S sequences in one launch per frame."""
    key = ("table", case.name)
    if key not in _CACHE:
        e = case.table_engine()
        _CACHE[key] = run(torch, case, e, K)
        e.close()
    return _CACHE[key]


def same_rows(got, want):
    assert len(got) == len(want)
    for q, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b)
        for t, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (q, t)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_table_matches_separate_engines(torch, case):
    got, want = table(torch, case), separate(torch, case)
    same_rows(got[0], want[0])
    for q in range(K * S):
        for t in range(T):
            assert got[1][q][t] == want[1][q][t], (q, t)
    rows = want[0]
    assert all(sum(r.shape[0] for r in rows[q]) >= 20 for q in range(K * S))
    whole = [b"".join(r.tobytes() for r in rows[q]) for q in range(K * S)]
    assert len(set(whole)) == K * S  # the configs tell themselves apart on every sequence


def cost_lds(n_seq, track_cap, det_cap):
    """(cost_lds, tb_lds) as bx_boost_create sizes them (bx_boost.hip: lds_bytes and the budget
    in bx_boost_create), restated: the entries of the cost matrix a workgroup keeps in LDS."""
    S, T, D = n_seq, track_cap, det_cap
    N = max(T, D)

    def ints(n):
        return (n * 4 + 7) // 8 * 8

    def lds_bytes(cl, tb):
        return (D * 11 * 8 + cl * 8 + T * 8 + 2 * N * 8 + 16 + (T * 16 * 8 if tb else 0)
                + 2 * ints(D) + 2 * ints(T) + 2 * ints(2 * N) + 2 * ints(D + T) + 10 * ints(N)
                + 2 * ints(8))

    cap = min(max(160 * 1024 // ((S + 255) // 256), 40 * 1024), 152 * 1024)
    tb = S <= 512 and lds_bytes(0, 0) + T * 16 * 8 + 64 * 8 <= cap
    cl = max(min(max(cap - lds_bytes(0, tb), 0) // 8, D * T), 64)
    return cl, tb


def test_the_hbm_cases_take_the_hbm_path(torch):
    """The frames' pairs (detections x tracks entering the frame) exceed the LDS entries
    bx_boost_create leaves at HBM's capacities; at the small cases' capacities the whole matrix
    fits."""
    assert cost_lds(**HBM) == (86, False)
    assert cost_lds(K * S, **BD.CAPS) == (BD.CAPS["track_cap"] * BD.CAPS["det_cap"], True)
    e = HBM_NOREID.engine(S, HBM_NOREID.configs()[0])
    most = 0
    for t in range(12):
        step(torch, HBM_NOREID, e, frame_of(t))
        most = max(most, max(e.frame_stats(q, 1)["pairs"] for q in range(S)))
    e.close()
    assert most > cost_lds(**HBM)[0]


@pytest.mark.parametrize("case", [REID, NOREID, WARP, HBM_REID], ids=lambda c: c.name)
def test_table_matches_the_oracle(torch, case):
    """Every table sequence against the CPU oracle created with that sequence's config: a table
    that every sequence ignored would pass the comparison above whenever configs agree."""
    from oracle import pyoracle as po

    rows = table(torch, case)[0]
    for k, cfg in enumerate(BD.configs(case.reid)):
        for s in range(S):
            orc = po.OracleTracker("boosttrack", **BD.resolved(cfg))
            for t in range(T):
                d, e = frame_of(t)[s]
                want = orc.update(d, e if case.reid else None,
                                  warps_at(t)[s].reshape(2, 3) if case.warp else None)
                np.testing.assert_array_equal(rows[k * S + s][t], want, err_msg=f"{k} {s} {t}")


@pytest.mark.parametrize("case", [REID, HBM_REID], ids=lambda c: c.name)
def test_chunked_launches(torch, case):
    """Launches that cut through the middle of a config's block: seq0 != 0, nseq < S."""
    e = case.table_engine()
    got = run(torch, case, e, K, cuts=(1, 5, 6, 9), states=False)
    e.close()
    same_rows(got[0], separate(torch, case)[0])


def test_update_classes_host(torch):
    """per_class frames of one sequence with two classes: every class call runs on the sequence's
    entry."""
    case, n = REID, 20
    te = case.table_engine()
    for k, p in enumerate(case.configs()):
        pe = case.engine(1, p)
        seq = k * S  # scene 0 under config k
        for t in range(n):
            d, e = frame_of(t)[0]
            d = d.copy()
            d[:, 5] = np.arange(d.shape[0]) % 2
            w = np.stack([BD.warps(0)[t], BD.warps(1)[t]])
            a = te.update_classes_host(seq, d, e, w, n_classes=2)
            b = pe.update_classes_host(0, d, e, w, n_classes=2)
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, t)
            assert state(te, seq) == state(pe, 0), (k, t)
        assert te.counters(seq)["id_count"] > 0
        pe.close()
    te.close()


def _gap_frames(gap):
    """Object A for three frames, `gap` frames with only a far object B, then A again at
    confidence 0.35 (above the test's det_thresh 0.3, low enough for the DLO boost to raise it):
    its track is matched after time_since_update - 1 = gap steps without it."""
    a = np.array([[100.0, 100.0, 160.0, 250.0, 0.9, 0.0]])
    b = np.array([[900.0, 600.0, 960.0, 750.0, 0.9, 0.0]])
    back = np.vstack([a, b])
    back[0, 4] = 0.35
    return [np.vstack([a, b])] * 3 + [b] * gap + [back]


def test_confidence_table_grows_with_max_age(torch):
    """An engine created with max_age 2 holds 10 entries of 0.9 ** k.  An entry with max_age 40
    keeps a track alive for 22 frames without a match; get_confidence then reads index 21.  With
    the table left at 10 entries the index would be clamped to 9, the track's confidence would be
    0.9 ** 9 instead of 0.9 ** 21, and the soft-BIoU term of the DLO boost, which widens the boxes
    by the track's confidence, would boost the returning detection to another value."""
    case = NOREID
    long = replace(BD.params_of(BD.configs(False)[0]), max_age=40, min_hits=1, det_thresh=0.3)
    short = replace(long, max_age=2)
    te = case.engine(2, short, table=True)
    te.set_seq_params(1, [long])
    pe = case.engine(1, long)
    frames = _gap_frames(21)
    for t, d in enumerate(frames):
        got = step(torch, case, te, [(d, None), (d, None)])
        want = step(torch, case, pe, [(d, None)])[0]
        assert got[1].tobytes() == want.tobytes(), t
        assert state(te, 1) == state(pe, 0), t
    # the returning detection was matched to track 1 and boosted (the boost reads the confidence)
    last = want[want[:, 4] == 1]
    assert last.shape[0] == 1 and last[0, 5] > 0.35 + 1e-3
    # sequence 0 ran on max_age 2: there the track died and the detection started a new one
    assert not np.any(got[0][:, 4] == 1)
    # a table that shrinks nothing: the short sequences still read their indices
    te.set_seq_params(1, None)
    te.close()
    pe.close()


def test_round_trip_reset_copy_and_grown(torch):
    case = REID
    cfgs = case.configs()
    e = case.table_engine()
    for k in range(K):
        for s in range(S):
            assert e.seq_params(k * S + s) == cfgs[k]
    e.set_seq_params(2, None, nseq=3)
    assert [e.seq_params(q) for q in (2, 3, 4)] == [cfgs[0]] * 3  # (the engine's own)
    assert e.seq_params(5) == cfgs[2] and e.seq_params(1) == cfgs[0]
    e.set_seq_params(2, [cfgs[1], cfgs[1], cfgs[2]])
    # reset keeps the table, and a run after it is the run of a fresh engine
    half = range(T // 2)
    run(torch, case, e, K, frames=half, states=False)
    e.reset()
    assert all(e.seq_params(k * S + s) == cfgs[k] for k in range(K) for s in range(S))
    first = run(torch, case, e, K, frames=half)
    want = separate(torch, case)
    same_rows(first[0], [r[: T // 2] for r in want[0]])
    # grown(): tracks by bx_boost_copy_state, the table set again
    g = e.grown(160, 48)
    e.close()
    assert (g.track_cap, g.det_cap) == (160, 48)
    assert all(g.seq_params(k * S + s) == cfgs[k] for k in range(K) for s in range(S))
    rest = run(torch, case, g, K, frames=range(T // 2, T))
    same_rows(rest[0], [r[T // 2:] for r in want[0]])
    assert [s[-1] for s in rest[1]] == [s[-1] for s in want[1]]
    # bx_boost_copy_state itself copies tracks only: a plain copy runs on its own parameters
    from boxmot_amd import _native as N
    from boxmot_amd.engine import BoostTableEngine

    h = BoostTableEngine(n_seq=K * S, track_cap=160, det_cap=48, emb_dim=F, params=cfgs[0])
    N.check(N.load().bx_boost_copy_state(h._h, g._h), "bx_boost_copy_state")
    assert all(h.seq_params(q) == cfgs[0] for q in range(K * S))
    assert state(h, K * S - 1) == state(g, K * S - 1)
    h.close()
    g.close()


def test_validation_changes_nothing(torch):
    case = NOREID
    cfgs = case.configs()
    e = case.table_engine()
    bad = [replace(cfgs[3], max_age=-1), replace(cfgs[3], min_hits=-1),
           replace(cfgs[3], max_age=100001)]
    for p in bad:
        with pytest.raises(ValueError):
            e.set_seq_params(0, [cfgs[3], p])  # (the first entry is fine: nothing is written)
    for seq0, n in ((-1, 1), (K * S, 1), (K * S - 1, 2)):
        with pytest.raises(ValueError):
            e.set_seq_params(seq0, [cfgs[3]] * n)
        with pytest.raises(ValueError):
            e.set_seq_params(seq0, None, nseq=n)
    with pytest.raises(ValueError):
        e.seq_params(K * S)
    assert all(e.seq_params(k * S + s) == cfgs[k] for k in range(K) for s in range(S))
    got = run(torch, case, e, K, states=False)
    e.close()
    same_rows(got[0], separate(torch, case)[0])
    # an engine without a table refuses the same and stays without one
    e = case.engine(S, cfgs[0], table=True)
    with pytest.raises(ValueError):
        e.set_seq_params(0, [bad[0]])
    e.set_seq_params(0, None)  # (nothing to clear)
    assert e.seq_params(1) == cfgs[0]
    e.close()


def test_set_then_cleared_equals_never_set(torch):
    case = WARP
    p = case.configs()[0]
    e = case.engine(S, p, table=True)
    e.set_seq_params(0, [case.configs()[4], case.configs()[5]])
    e.set_seq_params(0, None)
    assert [e.seq_params(q) for q in range(S)] == [p, p]
    got = run(torch, case, e, 1)
    e.close()
    want = separate(torch, case)
    same_rows(got[0], want[0][:S])
    assert got[1] == want[1][:S]

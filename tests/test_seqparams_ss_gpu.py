"""Per-sequence StrongSort parameters (bx_ss_set_seq_params_host) on the GPU: one table engine
of K x 2 sequences against K plain engines, byte for byte on every frame (rows, tracks, track
attributes, counters), with and without warps, born Confirmed and not, through the crowd stretch
with crowd_detection off as the engine's own value, in both LSAP modes and at the sequence counts
where ss_launch changes shape; against the CPU oracle; and the contract with the state crowd mode
adapts."""
import dataclasses

import numpy as np
import pytest

from tests import sweep_strong_data as SD

pytestmark = pytest.mark.gpu

S, K, F = SD.S, SD.K, SD.F
CAPS = (SD.CAPS["track_cap"], SD.CAPS["det_cap"], F, SD.CAPS["vec_cap"])
# ss_launch: nseq >= 8 moves the crowd test and the predict to the side stream, nseq >= 64 takes
# 2 crowd blocks per sequence instead of 16; ss_nn_kernel's grid is ceil(2048 / nseq) waves,
# rounded up to a multiple of 8 from 64 waves on: 64 at nseq 32, 63 at nseq 33
LAUNCH_COUNTS = (1, 7, 8, 32, 33, 63, 64)


@pytest.fixture(scope="module")
def E():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import engine

    return engine


@pytest.fixture(scope="module")
def scenes():
    return [SD.scene(s) for s in range(S)]


def snapshot(eng, q):
    t, a, c = eng.tracks(q), eng.track_attrs(q), eng.counters(q)
    return (b"".join(np.ascontiguousarray(t[k]).tobytes() for k in sorted(t)),
            b"".join(np.ascontiguousarray(a[k]).tobytes() for k in sorted(a)),
            tuple(sorted(c.items())))


def run(eng, seqs, scenes, warps=False, fast=True, every=True):
    """Frame by frame through update_host: engine sequence q runs scene seqs[q].  Returns per
    sequence the rows of every frame and (every=True) a snapshot after every frame."""
    eng.set_lsap_mode(fast)
    out = [[] for _ in seqs]
    for t in range(max(SD.N_FRAMES)):
        for q, s in enumerate(seqs):
            if t >= len(scenes[s]) or not scenes[s][t][0].shape[0]:
                continue
            d, e = scenes[s][t]
            r = eng.update_host(q, d, e, SD.warps(s)[t] if warps else None)
            out[q].append((r.tobytes(), snapshot(eng, q) if every else None))
    assert eng.status() == 0
    return out


def plain(E, cfgs, scenes, born=False, **kw):
    """K plain engines of S sequences each, one per config."""
    out = []
    for c in cfgs:
        eng = E.SsEngine(S, *CAPS, params=SD.params_of(c, born))
        try:
            out += run(eng, list(range(S)), scenes, **kw)
        finally:
            eng.close()
    return out


def table(E, cfgs, scenes, born=False, base=None, **kw):
    eng = E.SsTableEngine(len(cfgs) * S, *CAPS, params=base or SD.params_of({}, born))
    try:
        for k, c in enumerate(cfgs):
            eng.set_seq_params(k * S, [SD.params_of(c, born)] * S)
        return run(eng, list(range(S)) * len(cfgs), scenes, **kw)
    finally:
        eng.close()


@pytest.mark.parametrize("warps,born,fast", [(False, True, True), (True, True, True),
                                             (True, True, False)])
def test_table_matches_separate_engines(E, scenes, warps, born, fast):
    want = plain(E, SD.CONFIGS, scenes, born, warps=warps, fast=fast)
    got = table(E, SD.CONFIGS, scenes, born, warps=warps, fast=fast)
    assert got == want
    if born:  # the configs tell themselves apart
        rows = [tuple(r for r, _ in q) for q in got]
        assert len({rows[k * S + SD.CROWD_SEQ] for k in range(K)}) == K


def test_born_confirmed_in_one_entry(E, scenes):
    """Over the first ten frames: born Tentative, every unmatched detection of every frame takes
    a slot for good, which the whole scene does not fit."""
    head = [sc[:10] for sc in scenes]
    eng = E.SsTableEngine(2 * S, *CAPS, params=SD.params_of({}, False))
    try:
        eng.set_seq_params(S, [SD.params_of({}, True)] * S)
        got = run(eng, list(range(S)) * 2, head)
    finally:
        eng.close()
    assert got[:S] == plain(E, [{}], head, False)
    assert got[S:] == plain(E, [{}], head, True)
    assert got[0] != got[S]


def test_crowd_on_in_entries_off_in_engine(E, scenes):
    """The engine's own crowd_detection is off, so without the table no crowd kernel would be
    launched: the entries switch it on, and the tracks born in the crowd stretch carry
    int(1.5 * max_age)."""
    base = SD.params_of(dict(crowd_detection=False), True)
    on = SD.params_of(dict(max_age=30), True)
    eng = E.SsTableEngine(2 * S, *CAPS, params=base)
    ref = E.SsEngine(S, *CAPS, params=on)
    try:
        eng.set_seq_params(0, [on] * S)
        got = run(eng, list(range(S)) * 2, scenes)
        ages = set(eng.track_attrs(SD.CROWD_SEQ)["max_age"].tolist())
        assert 45 in ages and 30 in ages and not ages - {30, 45}  # born in crowd mode / not
        assert set(eng.track_attrs(S + SD.CROWD_SEQ)["max_age"].tolist()) == {50}
        assert got[:S] == run(ref, list(range(S)), scenes)
    finally:
        eng.close()
        ref.close()
    assert got[S:] == plain(E, [dict(crowd_detection=False)], scenes, True)


def test_table_matches_oracle(E, scenes):
    got = table(E, SD.CONFIGS, scenes, True, warps=True, every=False)
    for k, c in enumerate(SD.CONFIGS):
        for s in range(S):
            want = SD.oracle_rows(SD.resolved(c), s, with_warps=True, born_confirmed=True)
            rows = np.concatenate([np.frombuffer(r, np.float64).reshape(-1, 10)
                                   for r, _ in got[k * S + s]])
            np.testing.assert_array_equal(rows, want[:, 1:])


@pytest.mark.parametrize("n_seq", LAUNCH_COUNTS)
def test_step_ranges_at_launch_shapes(E, scenes, n_seq):
    """bx_ss_step over n_seq sequences whose configs alternate, launched as two ranges that cut
    through a config's block, against update_host on plain engines."""
    import torch

    cfgs = [SD.CONFIGS[(q // S) % K] for q in range(n_seq)]
    eng = E.SsTableEngine(n_seq, *CAPS, params=SD.params_of({}, True))
    want = {}
    try:
        for q, c in enumerate(cfgs):
            eng.set_seq_params(q, [SD.params_of(c, True)])
        dev = torch.device("cuda")
        cut = 1 if n_seq > 1 else 0
        got = [[] for _ in range(n_seq)]
        for t in range(8):
            for q0, q1 in ((0, cut), (cut, n_seq)):
                if q0 == q1:
                    continue
                fr = [scenes[q % S][t] for q in range(q0, q1)]
                off = np.zeros(q1 - q0 + 1, np.int32)
                off[1:] = np.cumsum([d.shape[0] for d, _ in fr])
                dd = torch.from_numpy(np.concatenate([d for d, _ in fr])).to(dev)
                ee = torch.from_numpy(np.concatenate([e for _, e in fr])).to(dev)
                out = torch.empty((int(off[-1]), 10), dtype=torch.float64, device=dev)
                cnt = torch.empty(q1 - q0, dtype=torch.int32, device=dev)
                eng.step(dd, torch.from_numpy(off).to(dev), ee, None, out, cnt, seq0=q0,
                         nseq=q1 - q0)
                o, c = out.cpu().numpy(), cnt.cpu().numpy()
                for q in range(q0, q1):
                    got[q].append(o[off[q - q0]: off[q - q0] + c[q - q0]].tobytes())
        assert eng.status() == 0
        short = [sc[:8] for sc in scenes]
        for k in range(min(K, (n_seq + S - 1) // S)):
            ref = E.SsEngine(S, *CAPS, params=SD.params_of(SD.CONFIGS[k], True))
            try:
                for s, rows in enumerate(run(ref, list(range(S)), short, every=False)):
                    want[k, s] = [r for r, _ in rows]
            finally:
                ref.close()
        for q in range(n_seq):
            assert got[q] == want[(q // S) % K, q % S], q
    finally:
        eng.close()


def test_adapted_state_contract(E, scenes):
    mine = SD.params_of(dict(max_age=30, nn_budget=40, max_cos_dist=0.3), True)
    eng = E.SsTableEngine(S, *CAPS, params=SD.params_of({}, True))
    try:
        sc = scenes[SD.CROWD_SEQ]
        eng.set_seq_params(0, [mine])
        assert eng.seq_params(0) == mine and eng.seq_params(1) == SD.params_of({}, True)
        for d, e in sc[:11]:  # (frame 9 has no detection)
            if d.shape[0]:
                eng.update_host(0, d, e)
        # born at frame 1 on the seed, and behind the stretch, in crowd mode, on int(1.5 * seed)
        assert set(eng.track_attrs(0)["max_age"].tolist()) == {30, 45}
        before = snapshot(eng, 0)
        with pytest.raises(ValueError):  # frame counter > 0
            eng.set_seq_params(0, [SD.params_of({}, True)])
        with pytest.raises(ValueError):
            eng.set_seq_params(0, None, 1)
        assert eng.seq_params(0) == mine and snapshot(eng, 0) == before
        for d, e in sc[11:]:  # crowd mode is left: restored to the entry's 30, never the engine's
            if d.shape[0]:
                eng.update_host(0, d, e)
        assert set(eng.track_attrs(0)["max_age"].tolist()) <= {30, 45}
        eng.reset(0, 1)  # re-seeds from the entry, and the table is kept
        assert eng.seq_params(0) == mine and eng.counters(0)["frame_count"] == 0
        d, e = scenes[0][0]
        eng.update_host(0, d, e)
        assert set(eng.track_attrs(0)["max_age"].tolist()) == {30}
        eng.reset(0, 1)
        eng.set_seq_params(0, [SD.params_of(dict(max_age=7), True)])  # accepted after reset
        eng.update_host(0, d, e)
        assert set(eng.track_attrs(0)["max_age"].tolist()) == {7}
    finally:
        eng.close()


def test_validation_changes_nothing(E):
    eng = E.SsTableEngine(S, *CAPS, params=SD.params_of(dict(nn_budget=100), True))
    try:
        ok = SD.params_of(dict(nn_budget=100, max_age=9), True)
        eng.set_seq_params(0, [ok])
        for bad in (dict(nn_budget=0), dict(max_age=-1), dict(nn_budget=400),
                    dict(nn_budget=101)):  # (the last: above the engine's own, which sized the
            with pytest.raises(ValueError):  # galleries)
                eng.set_seq_params(0, [ok, dataclasses.replace(ok, **bad)])
            assert eng.seq_params(0) == ok and eng.seq_params(1).max_age == 50
        for rng in ((-1, [ok]), (S, [ok]), (1, [ok, ok])):
            with pytest.raises(ValueError):
                eng.set_seq_params(*rng)
    finally:
        eng.close()
    with pytest.raises(ValueError):  # bx_ss_create's own limit on the same figure
        E.SsEngine(1, *CAPS, params=SD.params_of(dict(nn_budget=400)))


def test_set_then_cleared_equals_plain(E, scenes):
    eng = E.SsTableEngine(S, *CAPS, params=SD.params_of({}, True))
    try:
        eng.set_seq_params(0, [SD.params_of(SD.CONFIGS[3], True)] * S)
        eng.set_seq_params(0, None)
        assert eng.seq_params(0) == SD.params_of({}, True)
        got = run(eng, list(range(S)), scenes)
    finally:
        eng.close()
    assert got == plain(E, [{}], scenes, True)


def test_copy_state_and_grown(E, scenes):
    """copy_state carries the tracks and the adapted state, not the table; grown() sets the
    table again, and the grown engine goes on as the original does."""
    p = SD.params_of(SD.CONFIGS[6], True)
    a = E.SsTableEngine(S, *CAPS, params=SD.params_of({}, True))
    b = None
    try:
        a.set_seq_params(1, [p])
        head = [sc[:12] for sc in scenes]
        run(a, list(range(S)), head, every=False)
        b = a.grown(CAPS[0] * 2, CAPS[1])
        assert isinstance(b, E.SsTableEngine) and b.seq_params(1) == p
        assert b.seq_params(0) == SD.params_of({}, True)
        assert [snapshot(b, q) for q in range(S)] == [snapshot(a, q) for q in range(S)]
        tail = [[(d[:0], e[:0])] * 12 + sc[12:20] for sc, (d, e) in zip(scenes, [s[0] for s in scenes])]
        assert run(b, list(range(S)), tail) == run(a, list(range(S)), tail)
        c = E.SsEngine(S, *CAPS, params=SD.params_of({}, True))
        try:
            from boxmot_amd import _native as N

            N.check(N.load().bx_ss_copy_state(c._h, a._h), "bx_ss_copy_state")
            assert [snapshot(c, q) for q in range(S)] == [snapshot(a, q) for q in range(S)]
        finally:
            c.close()
    finally:
        a.close()
        if b is not None:
            b.close()

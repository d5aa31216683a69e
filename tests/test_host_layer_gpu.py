"""The host layer the six tracker engines share (csrc/bx_host.h, csrc/bx_ocs_host.h, the base
classes of boxmot_amd/engine.py): the timing probe's contract, the counter cache of update_host,
the growth path and create's refusals — the same four checks over every engine, at the smallest
shapes the creates accept (2 sequences, 16 track and detection slots, 3 detections a frame)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, CAP, ND = 2, 16, 3
KINDS = ["botsort", "ocsort", "deepocsort", "hybridsort", "boosttrack", "strongsort"]
# embedding width: the smallest each create accepts (BoT-SORT's norm kernel needs 128 * 2^k)
F = {"botsort": 128, "ocsort": 0, "deepocsort": 8, "hybridsort": 8, "boosttrack": 8,
     "strongsort": 8}
# stages an engine legitimately skips here: BoT-SORT's covariance predict runs only with a warp
SKIPPED = {"botsort": {"cov_predict"}}
# event pairs per step where it is not one: below 8 sequences StrongSort times "pre" in two
# parts, the crowd/motion kernels on the main stream and the pre/sort kernels on the side stream
PAIRS = {("strongsort", "pre"): 2}


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return t


def make(kind, track_cap=CAP, det_cap=CAP, emb_dim=None, n_seq=S, **params):
    from boxmot_amd import engine as E

    f = F[kind] if emb_dim is None else emb_dim
    if kind == "botsort":
        return E.Engine("botsort", n_seq, track_cap, det_cap, f, params=E.EngineParams(**params))
    if kind == "ocsort":
        return E.OcsortEngine(n_seq, track_cap, det_cap, E.OcsortParams(**params))
    if kind == "deepocsort":
        return E.DeepOcsortEngine(n_seq, track_cap, det_cap, f, E.DeepOcsortParams(**params))
    if kind == "hybridsort":
        return E.HybridsortEngine(n_seq, track_cap, det_cap, f, E.HybridsortParams(**params))
    if kind == "boosttrack":
        return E.BoostEngine(n_seq, track_cap, det_cap, f, E.BoostParams(**params))
    return E.SsEngine(n_seq, track_cap, det_cap, f, params=E.SsParams(**params))


def frame(kind, t, seq):
    """Three confident, well separated boxes drifting with t, and unit embedding rows."""
    rng = np.random.default_rng(100 * seq + 7)
    d = np.zeros((ND, 6), np.float64 if kind == "strongsort" else np.float32)
    for k in range(ND):
        x, y = 100 + 300 * k + 2 * t + 10 * seq, 200 + 5 * t
        d[k] = [x, y, x + 80, y + 160, 0.9, 0]
    e = None
    if F[kind]:
        e = rng.standard_normal((ND, F[kind]))  # the same rows every frame: they re-associate
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        e = e.astype(np.float32 if kind == "botsort" else np.float64)
    return d, e


def update_host(eng, kind, seq, t):
    d, e = frame(kind, t, seq)
    return eng.update_host(seq, d) if kind == "ocsort" else eng.update_host(seq, d, e)


def step(torch, eng, kind, t):
    fr = [frame(kind, t, q) for q in range(S)]
    d = torch.from_numpy(np.concatenate([f[0] for f in fr])).cuda()
    off = torch.arange(0, ND * (S + 1), ND, dtype=torch.int32).cuda()
    e = torch.from_numpy(np.concatenate([f[1] for f in fr])).cuda() if F[kind] else None
    out = torch.zeros((ND * S, 10 if kind == "strongsort" else 8), dtype=torch.float64,
                      device="cuda")
    cnt = torch.zeros(S, dtype=torch.int32, device="cuda")
    if kind == "ocsort":
        eng.step(d, off, out, cnt)
    elif kind == "hybridsort":
        eng.step(d, off, e, out, cnt)
    else:
        eng.step(d, off, e, None, out, cnt)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
def test_probe_contract(torch, kind):
    eng = make(kind)
    t = 0
    stages = [True] if kind == "ocsort" else list(eng.STAGES)
    for st in stages:
        eng.reset()  # (three frames of tracks at a time: the slots never run out)
        eng.probe(st)
        for _ in range(3):
            t += 1
            step(torch, eng, kind, t)
        ms, n = eng.probe_read()
        print(kind, st, ms, n)
        if st in SKIPPED.get(kind, ()):
            assert (ms, n) == (0.0, 0)
        else:
            assert n == 3 * PAIRS.get((kind, st), 1) and ms > 0.0
        assert eng.probe_read() == (0.0, 0)
    eng.reset()
    eng.probe(False if kind == "ocsort" else None)
    for _ in range(3):
        t += 1
        step(torch, eng, kind, t)
    assert eng.probe_read() == (0.0, 0)
    assert eng.status() == 0
    eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_counter_cache_coherence(torch, kind):
    eng = make(kind)
    for t in (1, 2):
        update_host(eng, kind, 0, t)
    cached = eng.counters(0)  # answered from the row update_host brought back
    assert cached["frame_count"] == 2
    if hasattr(eng, "set_id_count"):  # drops the cache: the same counters, read from the device
        eng.set_id_count(0, cached["id_count"])
        assert eng.counters(0) == cached
    update_host(eng, kind, 0, 3)
    cached = eng.counters(0)
    update_host(eng, kind, 1, 1)  # the cache now holds sequence 1's row
    assert eng.counters(1)["frame_count"] == 1
    assert eng.counters(0) == cached and cached["frame_count"] == 3
    eng.close()


def snapshot(eng):
    return [({k: np.asarray(v).tolist() for k, v in eng.tracks(q).items()}, eng.counters(q))
            for q in range(S)]


@pytest.mark.parametrize("kind", KINDS)
def test_growth_path(torch, kind):
    eng = make(kind)
    for t in (1, 2, 3):
        step(torch, eng, kind, t)
    big = eng.grown(32, 32)
    assert (big.track_cap, big.det_cap) == (32, 32)
    assert snapshot(big) == snapshot(eng)
    a, b = step(torch, eng, kind, 4), step(torch, big, kind, 4)
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[0], b[0])
    assert snapshot(big) == snapshot(eng)
    eng.close()
    big.close()


RANGE = "n_seq/track_cap/det_cap out of range"
# (engine, bad arguments) -> the message create refuses them with, None where create accepts them
# (the BoT-SORT engine takes up to 32767 track slots, StrongSort's up to 1024)
REFUSALS = [
    ("botsort", dict(track_cap=513), None),
    ("ocsort", dict(track_cap=513), RANGE),
    ("deepocsort", dict(track_cap=513), RANGE),
    ("hybridsort", dict(track_cap=513), RANGE),
    ("boosttrack", dict(track_cap=513), "n_seq/track_cap/det_cap/max_age out of range"),
    ("strongsort", dict(track_cap=513), None),
    ("ocsort", dict(delta_t=0), r"delta_t must be in \[1, 7\]"),
    ("deepocsort", dict(delta_t=0), r"delta_t must be in \[1, 7\]"),
    ("hybridsort", dict(delta_t=0), r"delta_t must be in \[1, 7\]"),
    ("botsort", dict(emb_dim=0), "with_reid needs emb_dim > 0"),
    ("deepocsort", dict(emb_dim=0), "emb_dim must be positive unless embedding_off"),
    ("hybridsort", dict(emb_dim=0), "emb_dim must be positive"),
    ("boosttrack", dict(emb_dim=0), "with_reid BoostTrack needs emb_dim > 0"),
    ("strongsort", dict(emb_dim=0), "bx_ss_config out of range"),
]


@pytest.mark.parametrize("kind,bad,msg", REFUSALS,
                         ids=[f"{k}-{'-'.join(b)}" for k, b, _ in REFUSALS])
def test_create_refusals(torch, kind, bad, msg):
    if msg is None:
        make(kind, **bad).close()
    else:
        with pytest.raises(ValueError, match=msg):
            make(kind, **bad)
    eng = make(kind)  # a good create straight afterwards
    assert eng.status() == 0 and eng.counters(0)["frame_count"] == 0
    eng.close()

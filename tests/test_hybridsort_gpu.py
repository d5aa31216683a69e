"""HybridSort on the GPU: parity with the reference-captured fixtures (tests/golden/hybrid_*.npz,
written by tests/golden/make_golden_hybridsort.py), the cosine distance and the feature-bank mean
as ops, the batched engine against single-sequence engines, capacity growth, the state round trip,
leading empty frames and ids."""
import ast
from collections import deque
from pathlib import Path

import numpy as np
import pytest

from boxmot_amd import HybridSort
from tests.emb_ref import cosdist_bound
from tests.golden_util import compare_outputs
from tests.scenes import scene_of

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = sorted(GOLDEN.glob("hybrid_*.npz"))
IMG = np.zeros((1080, 1920, 3), np.uint8)
U = 2.0 ** -53


@pytest.fixture(scope="module")
def native():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return torch


def make_tracker(args=None, **caps):
    kw = dict(det_thresh=0.3)
    kw.update(args or {})
    return HybridSort(reid_weights=None, device="cuda", half=False, **kw, **caps)


def run(tr, scene, n_frames, empty_at=(), snap_at=(), snaps=None):
    rows = []
    for t in range(1, n_frames + 1):
        d, e, _ = scene.frame(t)
        if t in empty_at:
            d, e = d[:0], e[:0]
        o = np.asarray(tr.update(d, IMG, e), np.float64).reshape(-1, 8)
        rows.append(np.concatenate([np.full((o.shape[0], 1), t, np.float64), o], 1))
        if t in snap_at:
            snaps[t] = tr.engine.tracks(0)
    return np.concatenate(rows, 0)


def test_fixtures_exist():
    assert len(FIXTURES) >= 9


def compare_state(got, ref, where):
    """The engine's tracks() against the reference's per-track state (list order).
    ids and bank push counts: exact.
    kf.x, kf.P: 1e-9 absolute, the bound the box columns carry, for entries of box magnitude;
      areas and covariances reach 1e4..1e5, where 1e-9 is a handful of ulps, so larger entries
      get the same relative room: 1e-11 of their size (the 5x5 inverse and the matrix products
      run in another summation order than LAPACK / BLAS; a wrong Q, R or P0 entry moves them by
      1e-3 and more).
    velocities: the reference holds them in float32 (sums of up to delta_t = 3 unit vectors, each
      from about 8 float32 roundings of values <= 1): 3 * 8 * 2^-24 = 1.5e-6 absolute.  The same
      bound is kept for hybrid_dt7, whose sums have up to 7 terms (7 * 8 * 2^-24 = 3.3e-6 by
      that count, which takes every rounding at its worst): it measures 5.7e-7 there.
    smooth_feat, bank mean: unit-size entries after up to 120 moving-average steps (the longest
      run), each a few float64 roundings with the norm summed in another order, so some
      120 * 5 * 2^-53 = 7e-14: 1e-12 absolute."""
    np.testing.assert_array_equal(got["id"], ref["id"], err_msg=where)
    np.testing.assert_array_equal(got["bank_count"], ref["bank_count"], err_msg=where)
    for k in ("x", "P"):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-11, atol=1e-9, err_msg=f"{where} {k}")
    np.testing.assert_allclose(got["vel"], ref["vel"], rtol=0, atol=1.5e-6, err_msg=where)
    for k in ("emb", "bank_mean"):
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-12, err_msg=f"{where} {k}")


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.stem[len("hybrid_"):])
def test_fixture_parity(native, path):
    """Boxes within 1e-9, every other column and the row count per frame exact; and, after four
    of the frames, every track's filter state, corner velocities, smoothed feature and bank mean
    against the reference's (compare_state): output boxes are observations, so only this pins
    the filter, the ORU replay and the feature kernel."""
    with np.load(path) as fx:
        for k in ast.literal_eval(str(fx["needs"])):
            assert int(fx[k]) > 0, f"the fixture never reached {k}"
        assert int(fx["lap_degenerate"]) == 0
        ref = fx["outputs"]
        args = ast.literal_eval(str(fx["tracker_args"]))
        scene, nf = scene_of(fx), int(fx["n_frames"])
        frames, off = [int(f) for f in fx["state_frames"]], fx["state_off"]
        state = {k[len("state_"):]: fx[k] for k in fx.files if k.startswith("state_")}
    tr = make_tracker(args)
    snaps = {}
    got = run(tr, scene, nf, snap_at=frames, snaps=snaps)
    assert tr.engine.status() == 0 and len(frames) == 4 and off[-1] > 0
    np.testing.assert_array_equal(np.bincount(got[:, 0].astype(int), minlength=nf + 1),
                                  np.bincount(ref[:, 0].astype(int), minlength=nf + 1))
    compare_outputs(got, ref, box_atol=1e-9)
    want = [{k: state[k][off[j]: off[j + 1]] for k in ("id", "x", "P", "vel", "emb", "bank_mean",
                                                        "bank_count")} for j in range(4)]
    worst = {}
    for f, w in zip(frames, want):  # printed before any of it is asserted
        for k in ("x", "P", "vel", "emb", "bank_mean"):
            if snaps[f][k].shape == w[k].shape and w[k].size:
                worst[k] = max(worst.get(k, 0.0), float(np.abs(snaps[f][k] - w[k]).max()))
    print(f"{path.stem}: max |device - reference| " + " ".join(f"{k}={v:.3e}" for k, v in worst.items()))
    for j, f in enumerate(frames):
        compare_state(snaps[f], want[j], f"frame {f}")


def cosdist_ref(T, D):
    """np.maximum(0, cdist(T, D, "cosine")).T: scipy's 1 - u.v / (|u| |v|)."""
    nt = np.sqrt((T * T).sum(1))
    nd = np.sqrt((D * D).sum(1))
    return np.maximum(0.0, 1.0 - (D @ T.T) / (nd[:, None] * nt[None, :]))


@pytest.mark.parametrize("nt,nd,F", [(1, 1, 1), (3, 5, 20), (65, 33, 64), (64, 64, 130)])
def test_cosdist_op(native, nt, nd, F):
    torch = native
    from boxmot_amd.engine import hybrid_cosdist

    rng = np.random.default_rng([nt, nd, F])
    T = rng.standard_normal((nt, F))
    D = rng.standard_normal((nd, F))
    D[0] = T[0] * 3.0  # a parallel pair: distance 0 up to rounding, never negative
    out = torch.full((nd, nt), float("nan"), dtype=torch.float64, device="cuda")
    hybrid_cosdist(torch.from_numpy(D).cuda(), torch.from_numpy(T).cuda(), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    err = np.abs(got - cosdist_ref(T, D))
    bound = cosdist_bound(T, D)
    print(f"cosdist ({nt},{nd},{F}): max err {err.max():.3e}, min slack {(bound - err).min():.3e}")
    assert (err <= bound).all()
    assert (got >= 0.0).all() and got[0, 0] <= bound[0, 0]


@pytest.mark.parametrize("pushed", [1, 29, 30, 31])
def test_bank_mean_op(native, pushed):
    """The mean of the rows present in the 30-deep ring (the empty-slot denominator at 1 and 29,
    the full ring at 30, the wrap at 31), and the distance to it."""
    torch = native
    from boxmot_amd.engine import hybrid_bank_mean, hybrid_cosdist

    nt, nd, F = 5, 7, 20
    rng = np.random.default_rng([pushed, F])
    bank = np.full((nt, 30, F), np.nan)  # rows never pushed must not be read
    dq = [deque(maxlen=30) for _ in range(nt)]
    for t in range(nt):
        for k in range(pushed):
            v = rng.standard_normal(F)
            bank[t, k % 30] = v
            dq[t].append(v)
    ref = np.stack([np.vstack(list(q)).mean(0) for q in dq])
    absum = np.stack([np.abs(np.vstack(list(q))).sum(0) for q in dq])
    n = min(pushed, 30)
    mean = torch.full((nt, F), float("nan"), dtype=torch.float64, device="cuda")
    hybrid_bank_mean(torch.from_numpy(bank).cuda(),
                     torch.full((nt,), pushed, dtype=torch.int32, device="cuda"), mean)
    torch.cuda.synchronize()
    got = mean.cpu().numpy()
    # a sum of n terms in any order, then one division, on each side
    assert (np.abs(got - ref) <= 2 * (n * U * absum / n + U * np.abs(ref))).all()
    D = rng.standard_normal((nd, F))
    out = torch.full((nd, nt), float("nan"), dtype=torch.float64, device="cuda")
    hybrid_cosdist(torch.from_numpy(D).cuda(), mean, out)
    torch.cuda.synchronize()
    err = np.abs(out.cpu().numpy() - cosdist_ref(got, D))
    assert (err <= cosdist_bound(got, D)).all()


def batched_case(torch):
    from boxmot_amd.engine import HybridsortEngine, HybridsortParams
    from boxmot_amd.synth import SyntheticScene

    F = 24
    skw = dict(layout="crowded", emb_dim=F, emb_dtype="float64", conf_lo=0.31, jitter=4.0)
    scenes = [SyntheticScene(n_obj=12, seed=81, **skw), SyntheticScene(n_obj=30, seed=82, **skw),
              SyntheticScene(n_obj=20, seed=83, **skw)]
    mk = lambda n: HybridsortEngine(n_seq=n, track_cap=64, det_cap=32, emb_dim=F,  # noqa: E731
                                    params=HybridsortParams())
    return scenes, mk


def step_range(torch, eng, scenes, ts, seq0):
    """One step of sequences [seq0, seq0 + len(ts)) at their own frame numbers ts."""
    fr = [scenes[seq0 + k].frame(t) for k, t in enumerate(ts)]
    ds = [f[0].astype(np.float32) for f in fr]
    off = np.concatenate([[0], np.cumsum([d.shape[0] for d in ds])]).astype(np.int32)
    n = int(off[-1])
    dets = torch.from_numpy(np.concatenate(ds, 0)).cuda()
    embs = torch.from_numpy(np.concatenate([f[1] for f in fr], 0)).cuda()
    out = torch.zeros((max(n, 1), 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(len(ts), dtype=torch.int32, device="cuda")
    eng.step(dets, torch.from_numpy(off).cuda(), embs, out, cnt, seq0=seq0, nseq=len(ts))
    torch.cuda.synchronize()
    o, c = out.cpu().numpy(), cnt.cpu().numpy()
    return [o[off[k]: off[k] + c[k]] for k in range(len(ts))]


def test_batched_equals_single(native):
    """Three scenes in one n_seq=3 engine and in three n_seq=1 engines, bitwise over 30 frames;
    at frames 11-15 the middle sequence is stepped alone through seq0/nseq (a ragged batch: it
    runs five frames ahead, the others catch up afterwards)."""
    torch = native
    scenes, mk = batched_case(torch)
    NF = 30
    single = []
    for q in range(3):
        e = mk(1)
        single.append([e.update_host(0, *scenes[q].frame(t)[:2]) for t in range(1, NF + 1)])
        assert e.status() == 0
        e.close()
    eng = mk(3)
    got = [[], [], []]
    for t in range(1, 11):
        for q, o in enumerate(step_range(torch, eng, scenes, [t, t, t], 0)):
            got[q].append(o)
    for t in range(11, 16):
        got[1].append(step_range(torch, eng, scenes, [t], 1)[0])
    for t in range(11, 16):
        o0 = step_range(torch, eng, scenes, [t], 0)[0]
        o2 = step_range(torch, eng, scenes, [t], 2)[0]
        got[0].append(o0)
        got[2].append(o2)
    for t in range(16, NF + 1):
        for q, o in enumerate(step_range(torch, eng, scenes, [t, t, t], 0)):
            got[q].append(o)
    assert eng.status() == 0
    rows = 0
    for q in range(3):
        for t in range(NF):
            np.testing.assert_array_equal(got[q][t], single[q][t], err_msg=f"seq {q} frame {t + 1}")
            rows += got[q][t].shape[0]
    assert rows > 100
    eng.close()


def test_growth_is_bitwise(native, monkeypatch):
    from boxmot_amd.engine import HybridsortEngine

    with np.load(GOLDEN / "hybrid_crowd40_dense.npz") as fx:
        scene = scene_of(fx)
        args = ast.literal_eval(str(fx["tracker_args"]))
    nf = 40
    grown = HybridsortEngine.grown
    steps = []  # (track_cap before, after, live tracks carried over) of every growth

    def counted(self, track_cap, det_cap):
        steps.append((self.track_cap, track_cap, self.slots_used(0)))
        return grown(self, track_cap, det_cap)

    monkeypatch.setattr(HybridsortEngine, "grown", counted)
    small = make_tracker(args, track_cap=8, det_cap=8)
    a = run(small, scene, nf)
    n_small = len(steps)
    b = run(make_tracker(args), scene, nf)
    assert len(steps) == n_small  # the default capacities never grow on this scene
    np.testing.assert_array_equal(a, b)
    assert len(steps) >= 2 and any(live > 0 for _, _, live in steps)
    assert small.engine.track_cap == steps[-1][1] > 8 and small.engine.det_cap > 8
    assert small.engine.status() == 0 and a.shape[0] > 50


def test_state_round_trip(native):
    from boxmot_amd.engine import HybridsortEngine, HybridsortParams
    from boxmot_amd.synth import SyntheticScene

    F = 16
    scene = SyntheticScene(n_obj=20, seed=91, layout="crowded", emb_dim=F, emb_dtype="float64",
                           conf_lo=0.31)
    mk = lambda: HybridsortEngine(n_seq=1, track_cap=32, det_cap=32, emb_dim=F,  # noqa: E731
                                  params=HybridsortParams())
    frames = [scene.frame(t)[:2] for t in range(1, 25)]
    a = mk()
    ref = [a.update_host(0, d, e) for d, e in frames]
    b = mk()
    for d, e in frames[:12]:
        b.update_host(0, d, e)
    blob = b.state_save(0)
    snap = b.tracks(0)
    assert snap["id"].shape[0] > 0 and (snap["bank_count"] > 0).all()
    np.testing.assert_allclose(np.linalg.norm(snap["emb"], axis=1), 1.0, rtol=0, atol=1e-15)
    c = mk()  # a fresh engine continues from the blob exactly as the uninterrupted run
    c.state_load(0, blob)
    for k, (d, e) in enumerate(frames[12:]):
        np.testing.assert_array_equal(c.update_host(0, d, e), ref[12 + k], err_msg=f"frame {13 + k}")
    assert sum(r.shape[0] for r in ref[12:]) > 0 and c.status() == 0
    # A perturbed score state of one track: tracks() returns what was written, for that track
    # and no other.  The score is clipped to [0.6, 1] before it reaches the association, so a
    # finite change need not move any output; a NaN does.  HybridSort's predict() returns
    # convert_x_to_bbox(kf.x), five columns with the score x[3] last (hybridsort.py:55-67,329),
    # so np.any(np.isnan(pos)) (:484) sees it and the track is popped: the object returns under
    # a new id.
    later = np.concatenate(ref[12:], 0)[:, 4]
    victim = next(int(i) for i in snap["id"] if i in later)
    k = int(np.flatnonzero(snap["id"] == victim)[0])
    x = snap["x"][k].copy()
    x[3] = np.nan
    p = mk()
    p.state_load(0, blob)
    p.state_set(0, [victim], x[None])
    back = p.tracks(0)
    np.testing.assert_array_equal(back["x"][k], x)
    np.testing.assert_array_equal(np.delete(back["x"], k, 0), np.delete(snap["x"], k, 0))
    np.testing.assert_array_equal(back["P"], snap["P"])
    got = [p.update_host(0, d, e) for d, e in frames[12:]]
    assert victim not in np.concatenate(got, 0)[:, 4]
    assert any(not np.array_equal(u, v) for u, v in zip(got, ref[12:]))
    assert p.status() == 0
    for e_ in (a, b, c, p):
        e_.close()


def test_leading_empty_frames_and_ids(native):
    """A video that starts without detections: the drop-in learns the embedding width (20 here)
    from the first detections and still counts the empty frames, so its output equals an engine
    of that width fed the same frames; ids start at 1 in every new instance."""
    from boxmot_amd.engine import HybridsortEngine, HybridsortParams
    from boxmot_amd.synth import SyntheticScene

    scene = SyntheticScene(n_obj=12, seed=93, emb_dim=20, emb_dtype="float64", p_det=0.9)
    tr = make_tracker()
    eng = HybridsortEngine(n_seq=1, emb_dim=20, params=HybridsortParams())
    empty = np.empty((0, 6))
    for t in range(1, 9):
        d, e, _ = scene.frame(t)
        if t <= 2:  # two empty frames; the first detections arrive at frame 3
            o = tr.update(empty, IMG, None)
            assert o.shape == (0, 8) and tr.engine is None
            assert eng.update_host(0, empty).shape[0] == 0
            continue
        got = np.asarray(tr.update(d, IMG, e), np.float64).reshape(-1, 8)
        np.testing.assert_array_equal(got, eng.update_host(0, d, e), err_msg=f"frame {t}")
    assert tr.frame_count == 8 and tr.engine.emb_dim == 20
    assert tr.engine.counters(0)["frame_count"] == 8 and got.shape[0] > 0
    eng.close()
    d, e, _ = SyntheticScene(n_obj=10, seed=92, emb_dim=16, emb_dtype="float64", p_det=1.0).frame(1)
    for _ in range(2):  # a second instance restarts the class-global counter
        o = np.asarray(make_tracker().update(d, IMG, e)).reshape(-1, 8)
        assert sorted(o[:, 4]) == list(range(1, 11))
    with pytest.raises(ValueError):
        make_tracker().update(d, IMG, None)

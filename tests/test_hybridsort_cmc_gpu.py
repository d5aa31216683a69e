"""HybridSort's camera-motion compensation (the reference's ECC switch) on the GPU: parity with
the reference-captured fixtures tests/golden/hybcmc_*.npz (tests/golden/
make_golden_hybridsort_cmc.py), the identity warp, per-sequence switches in one batched engine,
track-count edges against the numpy restatement of camera_update (tests/hybcmc_util.py), the
score-zero deviation, and the file flows and the sweep against drop-ins fed the same warps."""
import ast
from pathlib import Path

import numpy as np
import pytest

from boxmot_amd import HybridSort
from tests.golden_util import compare_outputs
from tests.hybcmc_util import ReplayCMC, camera_update
from tests.scenes import scene_of
from tests.test_hybridsort_gpu import IMG, compare_state, make_tracker, native, run  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = sorted(GOLDEN.glob("hybcmc_*.npz"))
WARP = np.array([[1.001, -0.002, 3.25], [0.002, 0.999, -1.5]], np.float32).astype(np.float64)


def load(path):
    with np.load(path) as fx:
        return dict(ref=fx["outputs"], args=ast.literal_eval(str(fx["tracker_args"])),
                    scene=scene_of(fx), nf=int(fx["n_frames"]), warps=fx["warps"],
                    frames=[int(f) for f in fx["state_frames"]], off=fx["state_off"],
                    state={k[len("state_"):]: fx[k] for k in fx.files if k.startswith("state_")})


def run_fixture(fx, ecc=True):
    tr = make_tracker(fx["args"])
    tr.ECC = ecc
    tr.cmc = ReplayCMC(fx["warps"])
    snaps = {}
    got = run(tr, fx["scene"], fx["nf"], snap_at=fx["frames"], snaps=snaps)
    assert tr.engine.status() == 0 and tr.cmc.calls == (fx["nf"] if ecc else 0)
    return got, snaps, tr


def test_fixtures_exist():
    assert [p.stem for p in FIXTURES] == ["hybcmc_crowd40", "hybcmc_identity", "hybcmc_noisy40"]


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.stem)
def test_fixture_parity(native, path):
    """The drop-in with ECC=True and a cmc that replays the fixture's warps: boxes within 1e-9,
    ids, the other columns and the row count per frame exact, and the four state snapshots within
    the existing suite's bounds (compare_state)."""
    fx = load(path)
    got, snaps, tr = run_fixture(fx)
    nf, ref, off = fx["nf"], fx["ref"], fx["off"]
    np.testing.assert_array_equal(np.bincount(got[:, 0].astype(int), minlength=nf + 1),
                                  np.bincount(ref[:, 0].astype(int), minlength=nf + 1))
    compare_outputs(got, ref, box_atol=1e-9)
    for j, f in enumerate(fx["frames"]):
        want = {k: fx["state"][k][off[j]: off[j + 1]] for k in ("id", "x", "P", "vel", "emb",
                                                                "bank_mean", "bank_count")}
        if want["x"].size and snaps[f]["x"].shape == want["x"].shape:
            print(f"{path.stem} frame {f}: max |x - ref| = "
                  f"{np.abs(snaps[f]['x'] - want['x']).max():.3e}")
        compare_state(snaps[f], want, f"{path.stem} frame {f}")
        # The summation order of the 2x3 product, against the fixture: kf.x bit for bit, at every
        # snapshot of the identity fixture and at the first of the shake fixtures.  (The phase
        # alone is pinned twice more: tests/test_hybridsort_cmc_host.py holds the restatement to
        # the fixtures' cam_before / cam_after, the edge test below holds the kernel to it.)
        # Bit for bit on the rows the phase writes (u, v, s, r); the others equal in value: the
        # predict's clamp `x[7] *= 0.0` (hybridsort.py:320-321, not part of this phase) leaves a
        # zero in the ds row whose sign differs from numpy's at one track of noisy40.
        if path.stem == "hybcmc_identity" or j == 0:
            cols = [0, 1, 2, 4]
            assert snaps[f]["x"][:, cols].tobytes() == want["x"][:, cols].tobytes(), \
                f"{path.stem} frame {f}"
            assert np.array_equal(snaps[f]["x"], want["x"]), f"{path.stem} frame {f}"
    assert tr.engine.ecc(0) == {"on": True, "score_zero_skips": 0}


def test_identity_warp_still_rewrites_the_state(native):
    """ECC=True under identity warps: the fixture's state, and not the ECC=False run's bits."""
    fx = load(GOLDEN / "hybcmc_identity.npz")
    assert np.array_equal(fx["warps"], np.tile(np.eye(2, 3), (fx["nf"], 1, 1)))
    _, on, _ = run_fixture(fx)
    _, off, tr = run_fixture(fx, ecc=False)
    assert not hasattr(tr.engine, "ecc")  # the plain engine: no switch was ever set
    last = fx["frames"][-1]
    j = len(fx["frames"]) - 1
    ref = fx["state"]["x"][fx["off"][j]: fx["off"][j + 1]]
    assert on[last]["x"][:, [0, 1, 2, 4]].tobytes() == ref[:, [0, 1, 2, 4]].tobytes()
    assert np.array_equal(on[last]["x"], ref)
    assert on[last]["x"].shape == off[last]["x"].shape
    assert on[last]["x"].tobytes() != off[last]["x"].tobytes()


# ------------------------------------------------------------------ engine level
F = 8


def grid_frame(n, t, rng):
    """n separated boxes drifting with t, scores in (0.5, 1), unit embeddings."""
    k = np.arange(n)
    x, y = 20.0 + 90.0 * (k % 20) + 1.5 * t, 20.0 + 80.0 * (k // 20) + 0.75 * t
    d = np.stack([x, y, x + 40.0 + (k % 3), y + 60.0 + (k % 5), 0.5 + 0.49 * rng.random(n),
                  np.zeros(n)], 1).astype(np.float32)
    return d


def embs_of(n, seed):
    e = np.random.default_rng(seed).standard_normal((n, F))
    return e / np.linalg.norm(e, axis=1, keepdims=True)


def engine(n_seq=1, cap=256):
    from boxmot_amd.engine import HybridsortCmcEngine, HybridsortParams

    return HybridsortCmcEngine(n_seq=n_seq, track_cap=cap, det_cap=cap, emb_dim=F,
                               params=HybridsortParams(det_thresh=0.3))


def same_tracks(a, b):
    assert a["id"].tolist() == b["id"].tolist()
    for k in ("x", "P", "vel", "emb", "bank_mean"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256])
def test_track_count_edges_against_numpy(native, n):
    """n live tracks (the engine's track_cap is 256) under a non-identity warp: engine A runs the
    phase, engine B has the numpy restatement's state written in and runs the same frame with
    its switch off; every track's state is the same bytes."""
    rng = np.random.default_rng(n)
    A, B = engine(), engine()
    e = embs_of(n, n)
    d1, d2 = grid_frame(n, 1, rng), grid_frame(n, 2, rng)
    for E in (A, B):
        assert E.update_host(0, d1, e).shape[0] <= n and E.counters(0)["n_tracks"] == n
    before = B.tracks(0)
    want, skipped = camera_update(before["x"], WARP)
    assert skipped == 0 and not np.array_equal(want, before["x"])
    B.state_set(0, before["id"], x=want)
    A.set_ecc(0, True)
    oa, ob = A.update_host(0, d2, e, WARP), B.update_host(0, d2, e)
    assert oa.tobytes() == ob.tobytes() and A.status() == 0
    same_tracks(A.tracks(0), B.tracks(0))
    assert A.ecc(0) == {"on": True, "score_zero_skips": 0} and B.ecc(0)["on"] is False


def test_score_zero_is_skipped_and_counted(native):
    """A state score of exactly 0 is where the reference raises: the track is left as it was,
    the others are warped, and the sequence's counter reads 1."""
    n = 5
    rng = np.random.default_rng(3)
    A, B = engine(), engine()
    e, d1, d2 = embs_of(n, 3), grid_frame(n, 1, rng), grid_frame(n, 2, rng)
    for E in (A, B):
        E.update_host(0, d1, e)
    x = A.tracks(0)["x"].copy()
    x[2, 3] = 0.0
    ids = A.tracks(0)["id"]
    A.state_set(0, ids, x=x)
    want, skipped = camera_update(x, WARP)
    assert skipped == 1 and np.array_equal(want[2], x[2]) and not np.array_equal(want[1], x[1])
    B.state_set(0, ids, x=want)
    A.set_ecc(0, [True])
    A.update_host(0, d2, e, WARP)
    B.update_host(0, d2, e)
    same_tracks(A.tracks(0), B.tracks(0))
    assert A.ecc(0)["score_zero_skips"] == 1 and A.status() == 0
    A.reset()
    assert A.ecc(0) == {"on": False, "score_zero_skips": 0}


def step_all(torch, eng, frames, embs, warps=None):
    """One batched step of every sequence of `eng` from device tensors."""
    off = np.zeros(len(frames) + 1, np.int32)
    off[1:] = np.cumsum([d.shape[0] for d in frames])
    dd = torch.from_numpy(np.concatenate(frames)).cuda()
    ee = torch.from_numpy(np.concatenate(embs)).cuda()
    out = torch.zeros((int(off[-1]), 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(len(frames), dtype=torch.int32, device="cuda")
    w = None if warps is None else torch.from_numpy(np.ascontiguousarray(warps)).cuda()
    eng.step(dd, torch.from_numpy(off).cuda(), ee, out, cnt, warps=w)
    torch.cuda.synchronize()
    o, c = out.cpu().numpy(), cnt.cpu().numpy()
    return [o[off[k]: off[k] + c[k]] for k in range(len(frames))]


def test_batched_switches_are_per_sequence(native):
    """Three sequences in one engine, switches on / off / on and different warps, stepped in one
    launch: each equals its own single-sequence engine byte for byte."""
    torch = native
    ns, nf = [30, 70, 45], 6
    warps = np.stack([WARP.reshape(6), np.array([1, 0, 50.0, 0, 1, 50.0]),
                      np.array([0.998, 0.003, -2.0, -0.003, 1.002, 4.5], np.float32)
                      .astype(np.float64)])
    on = [True, False, True]
    big = engine(3)
    big.set_ecc(0, on)
    singles = [engine() for _ in ns]
    for q, s in enumerate(singles):
        if on[q]:
            s.set_ecc(0, True)
    rngs = [np.random.default_rng(10 + q) for q in range(3)]
    embs = [embs_of(n, 20 + q) for q, n in enumerate(ns)]
    with pytest.raises(ValueError, match="warps of shape"):
        step_all(torch, big, [grid_frame(n, 1, np.random.default_rng(0)) for n in ns], embs,
                 warps[:2])
    for t in range(1, nf + 1):
        frames = [grid_frame(n, t, rngs[q]) for q, n in enumerate(ns)]
        got = step_all(torch, big, frames, embs, warps)
        for q, s in enumerate(singles):
            want = s.update_host(0, frames[q], embs[q], warps[q].reshape(2, 3))
            assert got[q].tobytes() == want.tobytes(), (t, q)
    for q, s in enumerate(singles):
        same_tracks(big.tracks(q), s.tracks(0))
    # the sequence whose switch is off ignored its (large) warp: a plain engine's state
    plain = engine()
    rng = np.random.default_rng(11)
    for t in range(1, nf + 1):
        plain.update_host(0, grid_frame(ns[1], t, rng), embs[1])
    same_tracks(big.tracks(1), plain.tracks(0))
    assert big.status() == 0


def test_switch_never_set_is_the_parent_behaviour(native):
    """An engine on which no switch was ever set (a call that only switches off included) runs an
    existing fixture as before, warps or not."""
    with np.load(GOLDEN / "hybrid_grid24_f20.npz") as fx:
        ref, args = fx["outputs"], ast.literal_eval(str(fx["tracker_args"]))
        scene, nf = scene_of(fx), int(fx["n_frames"])
    from boxmot_amd.engine import HybridsortCmcEngine

    tr = make_tracker(args)
    tr._make_engine = lambda emb_dim: HybridsortCmcEngine(
        n_seq=1, track_cap=tr._caps[0], det_cap=tr._caps[1], emb_dim=emb_dim, params=tr._params)
    got = run(tr, scene, nf)
    assert isinstance(tr.engine, HybridsortCmcEngine)
    tr.engine.set_ecc(0, False)
    assert tr.engine.ecc(0) == {"on": False, "score_zero_skips": 0}
    compare_outputs(got, ref, box_atol=1e-9)


def test_switching_on_later_moves_the_engine(native):
    """ECC switched on at frame 6: the drop-in's plain engine becomes one that takes warps, state
    carried over.  Same bytes as a drop-in that had such an engine from the start."""
    from boxmot_amd.engine import HybridsortCmcEngine, HybridsortEngine

    fx = load(GOLDEN / "hybcmc_noisy40.npz")
    runs = []
    for early in (False, True):
        tr = make_tracker(fx["args"])
        if early:
            tr._make_engine = lambda emb_dim, tr=tr: HybridsortCmcEngine(
                n_seq=1, track_cap=tr._caps[0], det_cap=tr._caps[1], emb_dim=emb_dim,
                params=tr._params)
        tr.cmc = ReplayCMC(fx["warps"][5:])
        rows = []
        for t in range(1, 21):
            if t == 6:
                assert early or type(tr.engine) is HybridsortEngine
                tr.ECC = True
            d, e, _ = fx["scene"].frame(t)
            rows.append(np.asarray(tr.update(d, IMG, e), np.float64).reshape(-1, 8))
        assert isinstance(tr.engine, HybridsortCmcEngine) and tr.cmc.calls == 15
        assert tr.engine.ecc(0) == {"on": True, "score_zero_skips": 0}
        runs.append((np.concatenate(rows), tr.engine.tracks(0)))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][0].shape[0] > 100
    same_tracks(runs[0][1], runs[1][1])


# ------------------------------------------------------------------ per class
NC = 3


def class_frame(n, t, rng, empty=None):
    """grid_frame with classes 0..NC-1 by row; `empty`: a class left without rows."""
    d = grid_frame(n, t, rng)
    d[:, 5] = np.arange(n) % NC
    keep = d[:, 5] != empty if empty is not None else np.ones(n, bool)
    return d, keep


def test_step_classes_warps_are_per_class_sequence(native):
    """Two sequences of three classes in one engine, one step_classes call per frame with a
    [2 * 3, 6] table of distinct warps and mixed switches; class 1 of sequence 1 has no rows in
    frames 3 and 4.  Every class sequence's tracks are, byte for byte, those of a single-sequence
    engine fed that class's rows and that warp, and the merged rows are theirs in class order
    (ids aside, which the merge makes class-global)."""
    torch = native
    ns, nf = [31, 47], 6
    rng_w = np.random.default_rng(5)
    warps = np.tile(np.eye(2, 3).reshape(6), (2 * NC, 1))
    warps[:, [2, 5]] = rng_w.uniform(-6, 6, (2 * NC, 2))
    warps[:, [0, 4]] += rng_w.uniform(-0.002, 0.002, (2 * NC, 2))
    warps = warps.astype(np.float32).astype(np.float64)
    on = [True, True, True, True, False, True]
    big = engine(2 * NC)
    big.set_ecc(0, on)
    singles = [engine() for _ in on]
    for q, s in enumerate(singles):
        s.set_ecc(0, on[q])
    rngs = [np.random.default_rng(30 + k) for k in range(2)]
    embs = [embs_of(n, 40 + k) for k, n in enumerate(ns)]
    with pytest.raises(ValueError, match="warps of shape"):
        big.step_classes(None, None, None, None, None, NC, warps=torch.zeros((2, 6)))
    for t in range(1, nf + 1):
        fr, em = [], []
        for k, n in enumerate(ns):
            d, keep = class_frame(n, t, rngs[k], empty=1 if (k == 1 and t in (3, 4)) else None)
            fr.append(d[keep])
            em.append(embs[k][keep])
        off = np.zeros(3, np.int32)
        off[1:] = np.cumsum([d.shape[0] for d in fr])
        o = torch.full((int(off[-1]), 8), np.nan, dtype=torch.float64, device="cuda")
        c = torch.zeros(2, dtype=torch.int32, device="cuda")
        big.step_classes(torch.from_numpy(np.concatenate(fr)).cuda(), torch.from_numpy(off).cuda(),
                         torch.from_numpy(np.concatenate(em)).cuda(), o, c, NC,
                         warps=torch.from_numpy(warps).cuda())
        torch.cuda.synchronize()
        o, c = o.cpu().numpy(), c.cpu().numpy()
        for k in range(2):
            got = o[off[k]: off[k] + c[k]]
            want = []
            for q in range(NC):
                m = fr[k][:, 5] == q
                want.append(singles[k * NC + q].update_host(
                    0, fr[k][m], em[k][m] if m.any() else None, warps[k * NC + q]))
            want = np.concatenate(want)
            cols = [0, 1, 2, 3, 5, 6, 7]
            assert got.shape == want.shape and got[:, cols].tobytes() == want[:, cols].tobytes(), \
                (t, k)
    assert big.status() == 0
    for q, s in enumerate(singles):
        same_tracks(big.tracks(q), s.tracks(0))
        assert big.ecc(q)["on"] is on[q]
    # the warps mattered: class sequence 0 is not what it is without them
    plain = engine()
    rng = np.random.default_rng(30)
    for t in range(1, nf + 1):
        d, _ = class_frame(ns[0], t, rng)
        m = d[:, 5] == 0
        plain.update_host(0, d[m], embs[0][m])
    assert big.tracks(0)["x"].tobytes() != plain.tracks(0)["x"].tobytes()


def test_per_class_dropin_calls_cmc_once_per_class(native):
    """HybridSortPerClass(ECC=True): one cmc call per class call, each class's tracks those of a
    single-sequence engine under that call's warp; and other tracks than with ECC off."""
    from boxmot_amd import HybridSortPerClass

    n, nf = 31, 6
    w2 = WARP.copy()
    w2[:, 2] += 2.5
    warps = np.stack([WARP, w2, np.eye(2, 3)] * nf)  # call k is class k % 3's
    embs = embs_of(n, 40)

    def dropin(ecc):
        tr = HybridSortPerClass(None, "cuda", False, 0.3, nr_classes=NC, ECC=ecc)
        tr.cmc = ReplayCMC(warps)
        rng = np.random.default_rng(30)
        for t in range(1, nf + 1):
            d, _ = class_frame(n, t, rng)
            tr.update(d, IMG, embs)
        return tr

    tr = dropin(True)
    assert tr.cmc.calls == nf * NC and tr.engine.status() == 0
    singles = [engine() for _ in range(NC)]
    rng = np.random.default_rng(30)
    for s in singles:
        s.set_ecc(0, True)
    for t in range(1, nf + 1):
        d, _ = class_frame(n, t, rng)
        for q, s in enumerate(singles):
            m = d[:, 5] == q
            s.update_host(0, d[m], embs[m], warps[q])
    off = dropin(False)
    assert off.cmc.calls == 0
    for q, s in enumerate(singles):
        same_tracks(tr.engine.tracks(q), s.tracks(0))
    assert tr.engine.tracks(0)["x"].tobytes() != off.engine.tracks(0)["x"].tobytes()


# ------------------------------------------------------------------ flows and the sweep
@pytest.fixture(scope="module")
def flow_scene(tmp_path_factory, native):
    """Two sequences of 12 iterated frames, one with a frame left without detections; boxes whose
    motion decides (noisy features) under a shake of up to 60 px a frame, past the 40 px box width."""
    from boxmot_amd import motio
    from boxmot_amd.synth import synth_warp

    tmp = tmp_path_factory.mktemp("hyb_cmc_flow")
    packed, fids, warps, truth = {}, {}, {}, {"SHAKE-A": [], "SHAKE-B": []}
    for q, (nm, hole) in enumerate({"SHAKE-A": None, "SHAKE-B": 5}.items()):
        rng = np.random.default_rng(60 + q)
        n, nf = 12, 12
        base = rng.standard_normal((n, F))
        pos = np.stack([100.0 + 130.0 * (np.arange(n) % 6), 100.0 + 300.0 * (np.arange(n) // 6)], 1)
        rows, embs, ws, cam = [], [], [], np.zeros(2)
        for t in range(1, nf + 1):
            w = synth_warp(70 + q, t, shift=60.0).astype(np.float32).astype(np.float64)
            cam = cam + w[:, 2]
            ws.append(w.reshape(6))
            if t - 1 == hole:
                continue
            d = np.zeros((n, 7))
            d[:, 0] = t
            truth[nm].append(np.column_stack([np.full(n, t), np.arange(1, n + 1), pos + cam,
                                              np.full(n, 40.0), np.full(n, 80.0),
                                              np.ones((n, 3))]))
            p = pos + cam + rng.normal(0, 0.5, pos.shape)
            d[:, 1:3], d[:, 3:5], d[:, 5] = p, p + [40.0, 80.0], 0.6 + 0.3 * rng.random(n)
            e = base + 3.0 * rng.standard_normal(base.shape)
            rows.append(d)
            embs.append(e / np.linalg.norm(e, axis=1, keepdims=True))
        packed[nm] = motio.pack_arrays(np.concatenate(rows), np.concatenate(embs),
                                       tmp / f"{nm}.bxmot")
        fids[nm], warps[nm] = list(range(1, nf + 1)), np.stack(ws)
    GT.update({nm: np.concatenate(v) for nm, v in truth.items()})
    return packed, fids, warps, tmp


GT = {}  # name -> gt rows [n, 9] (frame, id, x, y, w, h, 1, 1, 1) of flow_scene's objects


def dropin_files(packed, fids, warps, out, ecc):
    from boxmot_amd import motio

    for nm, p in packed.items():
        tr = make_tracker()
        tr.ECC = ecc
        seq = motio.BinSequence(p)
        stepped = [t for t, fid in enumerate(fids[nm]) if seq.frame(fid)[0].size]
        tr.cmc = ReplayCMC(warps[nm][stepped])
        res = []
        for t in stepped:
            d, e = seq.frame(fids[nm][t])
            rows = np.asarray(tr.update(d, IMG, e), np.float64)
            if rows.size:
                res.append(motio.convert_to_mot_format(rows.reshape(rows.shape[0], -1),
                                                       fids[nm][t]))
        motio.write_mot_results(Path(out) / f"{nm}.txt", np.vstack(res) if res else np.empty((0, 0)))


def files(d, names):
    return {nm: (Path(d) / f"{nm}.txt").read_bytes() for nm in names}


KW = dict(det_thresh=0.3, ECC=True)


@pytest.mark.parametrize("resident", [False, True], ids=["assembled", "resident"])
def test_flow_equals_dropins(flow_scene, resident):
    from boxmot_amd import motio

    packed, fids, warps, tmp = flow_scene
    tag = tmp / ("res" if resident else "asm")
    dropin_files(packed, fids, warps, tag / "single", True)
    single = files(tag / "single", packed)
    assert all(len(b) > 0 for b in single.values())
    motio.run_sequences("hybridsort", packed, tag / "flow", frame_ids=fids, tracker_kwargs=KW,
                        warps=warps, resident=resident)
    assert files(tag / "flow", packed) == single
    motio.run_sequences("hybridsort", packed, tag / "none", frame_ids=fids,
                        tracker_kwargs=dict(det_thresh=0.3), resident=resident)
    none = files(tag / "none", packed)
    dropin_files(packed, fids, warps, tag / "single_none", False)
    assert none == files(tag / "single_none", packed)
    for nm in packed:
        assert none[nm] != single[nm], f"{nm}: the warps changed nothing"


def test_sweep_mixes_the_switch(flow_scene):
    """sweep_reid over [{}, {ECC: True}] with warps: each config's files are run_sequences' for
    that config (the first runs uncompensated in the same engine)."""
    from boxmot_amd import motio, tune

    packed, fids, warps, tmp = flow_scene
    cfgs = [dict(det_thresh=0.3), dict(KW)]
    tune.sweep_reid("hybridsort", packed, cfgs, exp_dir=tmp / "sweep", frame_ids=fids,
                    warps=warps)
    motio.run_sequences("hybridsort", packed, tmp / "r0", frame_ids=fids, tracker_kwargs=cfgs[0],
                        resident=True)
    motio.run_sequences("hybridsort", packed, tmp / "r1", frame_ids=fids, tracker_kwargs=cfgs[1],
                        warps=warps, resident=True)
    assert files(tmp / "sweep" / "0000", packed) == files(tmp / "r0", packed)
    assert files(tmp / "sweep" / "0001", packed) == files(tmp / "r1", packed)
    assert files(tmp / "r0", packed) != files(tmp / "r1", packed)


def test_sweep_device_scoring_equals_host(flow_scene):
    """score="device", keep_results=False: the summaries score="host" gives, per config; and the
    compensated config scores better than the uncompensated one on a shaking camera."""
    from boxmot_amd import tune

    packed, fids, warps, tmp = flow_scene
    cfgs = [dict(det_thresh=0.3), dict(KW)]
    kw = dict(frame_ids=fids, warps=warps, gt=dict(GT),
              seq_lengths={nm: len(f) for nm, f in fids.items()})
    host = tune.sweep_reid("hybridsort", packed, cfgs, **kw)
    lean = tune.sweep_reid("hybridsort", packed, cfgs, score="device", keep_results=False, **kw)
    for k in range(2):
        assert host[k]["summary"] is not None and lean[k]["summary"] == host[k]["summary"], k
        assert lean[k]["results"] is None
    assert host[0]["summary"] != host[1]["summary"]

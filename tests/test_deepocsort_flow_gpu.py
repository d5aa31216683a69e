"""DeepOcSort in the many-sequence file flow (motio.run_sequences) and the device-resident feeder
behind ``resident=True`` (include/bxfeed.h): the batched flow against one drop-in per sequence
and against the reference-captured fixtures, the resident path against the default one byte for
byte, ragged schedules, the gather and the MOT append as ops, the overflow latch and GSI."""
import ast
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
IMG = np.zeros((1080, 1920, 3), np.uint8)


@pytest.fixture(scope="module")
def native():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return torch


def scene_rows(scene, n_frames, empty_at=()):
    """(dets7 [rows, 7] with the frame in column 0, embs [rows, F]) of frames 1..n_frames."""
    dets, embs = [], []
    for t in range(1, n_frames + 1):
        d, e, _ = scene.frame(t)
        if t in empty_at:
            continue
        dets.append(np.concatenate([np.full((d.shape[0], 1), t), d], 1))
        embs.append(e)
    return np.concatenate(dets), np.concatenate(embs)


def pack_text(tmp, name, dets7, embs):
    """Through val.py's text files (np.savetxt '%f') and motio.pack_sequence."""
    from boxmot_amd import motio

    dp, ep = tmp / f"{name}.dets.txt", tmp / f"{name}.embs.txt"
    np.savetxt(dp, dets7, fmt="%f", header=name)
    np.savetxt(ep, embs, fmt="%f")
    return motio.pack_sequence(dp, ep, tmp / f"{name}.bxmot")


def dropin_file(packed, fids, path, **kw):
    """process_sequence (val.py:337-353) with one fresh DeepOcSort drop-in."""
    from boxmot_amd import DeepOcSort, motio

    seq = motio.BinSequence(packed)
    tr = DeepOcSort(**kw)
    out = []
    for fid in fids:
        d, e = seq.frame(fid)
        if not d.size:
            continue
        rows = np.asarray(tr.update(d, IMG, e), np.float64).reshape(-1, 8)
        if rows.shape[0]:
            out.append(motio.convert_to_mot_format(rows, int(fid)))
    motio.write_mot_results(path, np.vstack(out) if out else np.empty((0, 0)))
    if tr.engine is not None:
        assert tr.engine.status() == 0


def files(d, names):
    return {nm: (Path(d) / f"{nm}.txt").read_bytes() for nm in names}


# ------------------------------------------------------------------ three sequences, two widths
CASES = {"f20": (20, (24, 40, 24)), "f64": (64, (40, 24, 40))}


@pytest.fixture(scope="module", params=sorted(CASES))
def three(request, native, tmp_path_factory):
    """Three synthetic sequences of 20, 35 and 50 frames packed with pack_sequence, and the files
    of one drop-in per sequence (computed once, shared by the tests below)."""
    from boxmot_amd import motio
    from boxmot_amd.synth import SyntheticScene

    F, n_obj = CASES[request.param]
    tmp = tmp_path_factory.mktemp(f"three_{request.param}")
    packed = {}
    for q, (nf, n) in enumerate(zip((20, 35, 50), n_obj)):
        sc = SyntheticScene(n_obj=n, seed=300 + 10 * q + F, emb_dim=F, emb_dtype="float64",
                            layout="crowded" if q == 1 else "grid", conf_lo=0.31, jitter=3.0)
        packed[f"SEQ-{q}"] = pack_text(tmp, f"SEQ-{q}", *scene_rows(sc, nf))
    for nm, p in packed.items():
        dropin_file(p, motio.BinSequence(p).frame_ids, tmp / "single" / f"{nm}.txt")
    return packed, files(tmp / "single", packed), tmp


def test_flow_equals_single_dropins(three):
    from boxmot_amd import motio

    packed, single, tmp = three
    ids = motio.run_sequences("deepocsort", packed, tmp / "batched")
    assert [len(v) for v in ids.values()] == [20, 35, 50]
    got = files(tmp / "batched", packed)
    for nm in packed:
        assert got[nm] == single[nm], f"{nm}: the batched flow differs from the drop-in"
        assert len(got[nm]) > 0
        rows = np.loadtxt(tmp / "batched" / f"{nm}.txt", delimiter=",")
        assert rows[:, 1].min() == 1  # every sequence's ids start at 1


def test_resident_equals_default(three):
    from boxmot_amd import motio

    packed, single, tmp = three
    motio.run_sequences("deepocsort", packed, tmp / "default")
    motio.run_sequences("deepocsort", packed, tmp / "resident", resident=True)
    a, b = files(tmp / "default", packed), files(tmp / "resident", packed)
    for nm in packed:
        assert a[nm] == b[nm] == single[nm], nm


# --------------------------------------------------------------------- the reference's fixtures
@pytest.mark.parametrize("resident", [False, True], ids=["default", "resident"])
@pytest.mark.parametrize("name", ["deepoc_grid24_f20", "deepoc_crowd40_f64"])
def test_flow_vs_reference_fixture(native, tmp_path, name, resident):
    """The fixture's scene, packed without a round trip through text and batched with a second,
    different sequence: the flow's file against the fixture's outputs after MOT formatting —
    boxes within 1e-9 (the DeepOcSort suite's bound), every other column exact."""
    from boxmot_amd import motio
    from boxmot_amd.synth import SyntheticScene

    with np.load(GOLDEN / f"{name}.npz") as fx:
        ref = fx["outputs"]
        args = ast.literal_eval(str(fx["tracker_args"]))
        scene_args = ast.literal_eval(str(fx["scene"]))
        nf = int(fx["n_frames"])
    assert args == {"cmc_off": True}  # (the flow's warps are the identity)
    other = SyntheticScene(n_obj=17, seed=977, emb_dim=scene_args["emb_dim"], emb_dtype="float64",
                           layout="crowded", conf_lo=0.31)
    packed = {
        "OTHER": motio.pack_arrays(*scene_rows(other, 33), tmp_path / "other.bxmot"),
        "FIX": motio.pack_arrays(*scene_rows(SyntheticScene(**scene_args), nf),
                                 tmp_path / "fix.bxmot"),
    }
    motio.run_sequences("deepocsort", packed, tmp_path / "out", tracker_kwargs=args,
                        resident=resident)
    want = np.vstack([motio.convert_to_mot_format(ref[ref[:, 0] == t][:, 1:], int(t))
                      for t in np.unique(ref[:, 0])])
    motio.write_mot_results(tmp_path / "want.txt", want)
    got = np.loadtxt(tmp_path / "out" / "FIX.txt", delimiter=",").reshape(-1, 9)
    exp = np.loadtxt(tmp_path / "want.txt", delimiter=",").reshape(-1, 9)
    assert got.shape == exp.shape and got.shape[0] > 100
    print(f"{name}: max box difference {np.abs(got[:, 2:6] - exp[:, 2:6]).max():.3e}")
    np.testing.assert_array_equal(got[:, [0, 1, 6, 7, 8]], exp[:, [0, 1, 6, 7, 8]])
    np.testing.assert_allclose(got[:, 2:6], exp[:, 2:6], rtol=0, atol=1e-9)
    assert (tmp_path / "out" / "OTHER.txt").stat().st_size > 0


# ---------------------------------------------------------------------------------- ragged edges
@pytest.fixture(scope="module")
def ragged(native, tmp_path_factory):
    """A: 30 image frames with no detections at frame 12; EMPTY: no rows at all; C: 18 frames; LAST:
    45 frames, so the frame indices past 30 have detections in the last sequence only.  det_cap is
    the largest detection count of any frame: at least one frame has exactly det_cap."""
    from boxmot_amd.synth import SyntheticScene

    tmp = tmp_path_factory.mktemp("ragged")
    F = 20
    kw = dict(emb_dim=F, emb_dtype="float64", conf_lo=0.31, jitter=3.0)
    rows = {
        "A": scene_rows(SyntheticScene(n_obj=24, seed=501, **kw), 30, empty_at=(12,)),
        "EMPTY": (np.empty((0, 7)), np.empty((0, F))),
        "C": scene_rows(SyntheticScene(n_obj=40, seed=502, layout="crowded", **kw), 18),
        "LAST": scene_rows(SyntheticScene(n_obj=24, seed=503, **kw), 45),
    }
    packed = {nm: pack_text(tmp, nm, *r) for nm, r in rows.items()}
    frame_ids = {"A": list(range(1, 31))}  # the image list: frame 12 is there, without detections
    per_frame = np.concatenate([np.bincount(r[0][:, 0].astype(int)) for r in rows.values()
                                if r[0].shape[0]])
    caps = dict(det_cap=int(per_frame.max()), track_cap=128)
    assert caps["det_cap"] <= 40
    return tmp, packed, frame_ids, caps


def test_ragged_edges(ragged):
    from boxmot_amd import motio

    tmp, packed, frame_ids, caps = ragged
    for nm, p in packed.items():
        fids = frame_ids.get(nm, motio.BinSequence(p).frame_ids)
        dropin_file(p, fids, tmp / "single" / f"{nm}.txt", **caps)
    single = files(tmp / "single", packed)
    out = {}
    for resident in (False, True):
        d = tmp / f"resident_{resident}"
        ids = motio.run_sequences("deepocsort", packed, d, frame_ids=frame_ids,
                                  tracker_kwargs=caps, resident=resident)
        assert ids["A"] == list(range(1, 31)) and ids["EMPTY"] == [] and len(ids["LAST"]) == 45
        out[resident] = files(d, packed)
        for nm in packed:
            assert out[resident][nm] == single[nm], (resident, nm)
    assert single["EMPTY"] == b"" and all(len(single[nm]) for nm in ("A", "C", "LAST"))
    # the frame without detections is skipped, not stepped: leaving it out of the image list
    # changes nothing, and no row carries its number
    for resident in (False, True):
        d = tmp / f"no12_{resident}"
        motio.run_sequences("deepocsort", packed, d, tracker_kwargs=caps, resident=resident)
        assert files(d, packed) == out[resident]
    frames = np.loadtxt(tmp / "single" / "A.txt", delimiter=",")[:, 0]
    assert 12 not in frames and frames.max() > 12
    last = np.loadtxt(tmp / "single" / "LAST.txt", delimiter=",")[:, 0]
    assert last.max() > 30  # rows from the frames only the last sequence has


# -------------------------------------------------------------------------- the feeder as an op
def ragged_set(F, seed):
    """Four sequences' packed rows and frame tables: different lengths, entries without
    detections, one sequence without any frame."""
    rng = np.random.default_rng([F, seed])
    counts = [[3, 0, 5, 1, 2], [], [4, 4, 0, 0, 7, 1, 2, 6, 3], [0, 2, 9, 0, 0, 1, 5]]
    dets, embs, tables = [], [], []
    for c in counts:
        c = np.array(c, np.int64)
        n = int(c.sum())
        order = rng.permutation(len(c))  # the frames' rows lie in another order than the table
        start = np.zeros(len(c), np.int64)
        pos = 0
        for j in order:
            start[j] = pos
            pos += c[j]
        dets.append(rng.uniform(-5, 1900, (n, 6)).astype(np.float32))
        embs.append(rng.standard_normal((n, F)))
        tables.append((start, c, 100 + np.arange(len(c))))
    return dets, embs, tables


def host_runs(tables, t):
    """run_sequences' runs of frame index t: [(k0, k1)]."""
    S = len(tables)
    has = [t < len(tb[1]) and tb[1][t] > 0 for tb in tables]
    runs, k = [], 0
    while k < S:
        if not has[k]:
            k += 1
            continue
        k1 = k
        while k1 < S and has[k1]:
            k1 += 1
        runs.append((k, k1))
        k = k1
    return runs


@pytest.mark.parametrize("F", [1, 20, 64, 130])
def test_feeder_gather_op(native, F):
    """Every frame index of a 4-sequence ragged set: the gathered dets, embs and det_off of every
    run against the numpy concatenation, bitwise.  F = 1 and 130 leave tails that are not a
    multiple of the 16-byte vector; odd F puts rows off the 16-byte phase."""
    from boxmot_amd.engine import SequenceFeeder

    dets, embs, tables = ragged_set(F, 1)
    feed = SequenceFeeder(dets, embs, tables, F)
    assert feed.n_frames == 9
    seen = 0
    for t in range(feed.n_frames):
        runs = host_runs(tables, t)
        assert [(r[0], r[0] + r[1]) for r in feed.schedule[t]] == runs
        feed.gather(t)
        for r, (k0, k1) in enumerate(runs):
            sl = [slice(int(tables[k][0][t]), int(tables[k][0][t] + tables[k][1][t]))
                  for k in range(k0, k1)]
            d, o, e = feed.read_run(t, r)
            np.testing.assert_array_equal(
                d.view(np.uint32),
                np.concatenate([dets[k][s] for k, s in zip(range(k0, k1), sl)]).view(np.uint32))
            np.testing.assert_array_equal(
                e.view(np.uint64),
                np.concatenate([embs[k][s] for k, s in zip(range(k0, k1), sl)]).view(np.uint64))
            off = np.concatenate([[0], np.cumsum([s.stop - s.start for s in sl])])
            np.testing.assert_array_equal(o, off.astype(np.int32))
            assert feed.schedule[t][r][2] == off[-1]
            seen += 1
    assert seen >= 9 and feed.status() == 0
    feed.close()


def random_outputs(rng, n, c):
    """c tracker output rows [x1, y1, x2, y2, id, conf, cls, det_ind] in an [n, 8] array (the
    rows past c are NaN), with exact halves for the half-to-even rounding."""
    out = np.full((n, 8), np.nan)
    x1 = rng.uniform(-50, 1900, c)
    y1 = rng.uniform(-50, 1000, c)
    w = rng.uniform(0.5, 300, c)
    x1[::3] = np.floor(x1[::3]) + 0.5
    w[1::3] = np.floor(w[1::3]) + 0.5
    out[:c] = np.column_stack([x1, y1, x1 + w, y1 + rng.uniform(1, 400, c),
                               rng.integers(1, 500, c), rng.uniform(0, 1, c),
                               rng.integers(0, 5, c), rng.integers(0, 99, c)])
    return out


def drive_appends(feed, tables, rng, full=False):
    """Gather, write random step outputs (out_count = the detections with `full`, otherwise often
    fewer) and append for every frame index; returns per sequence the list of (frame id, rows)
    handed to the append, in order."""
    fed = [[] for _ in tables]
    for t in range(feed.n_frames):
        feed.gather(t)
        for r, (k0, k1) in enumerate(host_runs(tables, t)):
            outs, cnts = [], []
            for k in range(k0, k1):
                n = int(tables[k][1][t])
                c = int(rng.integers(0, n + 1)) if (t + k) % 3 and not full else n
                outs.append(random_outputs(rng, n, c))
                cnts.append(c)
                fed[k].append((int(tables[k][2][t]), outs[-1][:c]))
            feed.write_run(t, r, np.concatenate(outs), cnts)
        feed.append(t)
    return fed


def test_feeder_mot_append_op(native):
    """The appended rows against convert_to_mot_format on the same rows, bitwise, per sequence in
    frame order; out_count below the detections leaves the rest of the step's rows out."""
    from boxmot_amd import motio
    from boxmot_amd.engine import SequenceFeeder

    dets, embs, tables = ragged_set(20, 2)
    feed = SequenceFeeder(dets, embs, tables, 20, guard_rows=3)
    fed = drive_appends(feed, tables, np.random.default_rng(77))
    res, base, cnt = feed.raw_results()
    assert feed.status() == 0
    got = feed.results()
    for k, rows in enumerate(fed):
        want = [motio.convert_to_mot_format(r, fid) for fid, r in rows if r.shape[0]]
        want = np.vstack(want) if want else np.empty((0, 9))
        np.testing.assert_array_equal(got[k].view(np.uint64), want.view(np.uint64))
        assert base[k + 1] - base[k] == tables[k][1].sum()  # sized from the detection count
        free = res[base[k] + cnt[k]: base[k + 1]]
        assert (free.view(np.uint64) == 0xFFFFFFFFFFFFFFFF).all()  # never written
    assert sum(len(g) for g in got) > 20
    assert (res[base[-1]:].view(np.uint64) == 0xFFFFFFFFFFFFFFFF).all() and len(res) == base[-1] + 3
    feed.close()


def test_feeder_overflow_latches(native):
    """Result buffers smaller than the rows: the sequence's append that does not fit writes
    nothing and latches the capacity status; its neighbours' rows, the rows it already had and
    the guard rows are untouched, and results() raises."""
    from boxmot_amd import _native as N
    from boxmot_amd import motio
    from boxmot_amd.engine import SequenceFeeder

    dets, embs, tables = ragged_set(20, 3)
    full = [int(tb[1].sum()) for tb in tables]
    cap = [4, 0, full[2], 1]  # sequence 0: 3 rows fit, then 5 do not; sequence 3: one 1-row frame
    feed = SequenceFeeder(dets, embs, tables, 20, res_cap=cap, guard_rows=4)
    fed = drive_appends(feed, tables, np.random.default_rng(5), full=True)
    assert feed.status() == 2 and N.STATUS[2] == "capacity exceeded"
    with pytest.raises(RuntimeError, match="overflow"):
        feed.results()
    res, base, cnt = feed.raw_results()
    assert list(np.diff(base)) == cap and len(res) == sum(cap) + 4
    # the rule: a frame's rows are appended whole when they fit behind the sequence's rows
    kept = {}
    for k in range(4):
        kept[k], have = [], 0
        for fid, r in fed[k]:
            if have + r.shape[0] <= cap[k]:
                kept[k].append((fid, r))
                have += r.shape[0]
    assert [len(kept[k]) < len(fed[k]) for k in range(4)] == [True, False, False, True]
    for k, rows in kept.items():
        want = [motio.convert_to_mot_format(r, fid) for fid, r in rows]
        want = np.vstack(want) if want else np.empty((0, 9))
        assert cnt[k] == want.shape[0] <= cap[k]
        np.testing.assert_array_equal(res[base[k]: base[k] + cnt[k]].view(np.uint64),
                                      want.view(np.uint64))
        free = res[base[k] + cnt[k]: base[k + 1]]
        assert (free.view(np.uint64) == 0xFFFFFFFFFFFFFFFF).all()
    assert 0 < cnt[0] <= 4 and cnt[3] == 1 and cnt[2] == full[2]
    assert (res[base[-1]:].view(np.uint64) == 0xFFFFFFFFFFFFFFFF).all()  # the guard rows
    feed.close()


# -------------------------------------------------------------------------------------------- GSI
@pytest.mark.parametrize("resident", [False, True], ids=["default", "resident"])
def test_flow_with_gsi(native, tmp_path, resident):
    from boxmot_amd import gsi, motio
    from boxmot_amd.synth import SyntheticScene

    packed = {}
    for s in (1, 2):
        sc = SyntheticScene(n_obj=8 + 4 * s, seed=60 + s, p_det=0.8, emb_dim=20,
                            emb_dtype="float64")
        packed[f"MOT-SYN-{s}"] = pack_text(tmp_path, f"MOT-SYN-{s}", *scene_rows(sc, 40))
    a, b = tmp_path / "two_steps", tmp_path / "one_call"
    motio.run_sequences("deepocsort", packed, a, resident=resident)
    plain = files(a, packed)
    gsi(a)
    motio.run_sequences("deepocsort", packed, b, gsi=True, resident=resident)
    for nm in packed:
        text = (b / f"{nm}.txt").read_bytes()
        assert text == (a / f"{nm}.txt").read_bytes() and text != plain[nm], nm
        assert b"," in plain[nm] and b"," not in text

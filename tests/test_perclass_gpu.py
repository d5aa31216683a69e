"""per_class=True for DeepOcSort and HybridSort on the GPU: the drop-ins against the
reference-captured fixtures (tests/golden/perclass_*.npz, written by
tests/golden/make_golden_perclass.py), ``step_classes`` over several sequences against one drop-in
per sequence bit for bit, HybridSort and the per_class mode in motio.run_sequences (default and
resident), and the error paths."""
import ast
from pathlib import Path

import numpy as np
import pytest

from tests.golden_util import compare_outputs
from tests.perclass_util import NR_CLASSES, fixture_frames

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = sorted(GOLDEN.glob("perclass_deepoc_*.npz")) + sorted(GOLDEN.glob("perclass_hybrid_*.npz"))
IMG = np.zeros((1080, 1920, 3), np.uint8)


@pytest.fixture(scope="module")
def native():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return torch


def make_dropin(kind, args, **kw):
    from boxmot_amd import DeepOcSortPerClass, HybridSortPerClass

    if kind == "deepocsort":
        return DeepOcSortPerClass(nr_classes=NR_CLASSES, **args, **kw)
    return HybridSortPerClass(reid_weights=None, device="cuda", half=False,
                              nr_classes=NR_CLASSES, **args, **kw)


def run_dropin(tr, frames):
    rows = []
    for t, d, e in frames:
        o = np.asarray(tr.update(d, IMG, e), np.float64).reshape(-1, 8)
        rows.append(np.concatenate([np.full((o.shape[0], 1), t, np.float64), o], 1))
    return np.concatenate(rows, 0)


def load(path):
    with np.load(path) as fx:
        return {k: fx[k] for k in fx.files}


def test_fixtures_exist():
    names = [p.stem for p in FIXTURES]
    assert any(n.startswith("perclass_deepoc") for n in names)
    assert sum(n.startswith("perclass_hybrid") for n in names) >= 2


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.stem)
def test_dropin_equals_reference(native, path):
    """Boxes within 1e-9 (the tolerance of these two trackers), ids, conf,
    cls, det_ind and the rows per frame exact."""
    fx = load(path)
    for k in ast.literal_eval(str(fx["needs"])):
        assert int(fx[k]) > 0, f"the fixture never reached {k}"
    assert int(fx["lap_degenerate"]) == 0 and int(fx["nr_classes"]) == NR_CLASSES
    kind, args = str(fx["kind"]), ast.literal_eval(str(fx["tracker_args"]))
    if kind == "hybridsort" and args.get("longterm_reid_weight"):
        assert int(fx["ref_corrections"]) > 0
    ref, nf = fx["outputs"], int(fx["n_frames"])
    tr = make_dropin(kind, args)
    got = run_dropin(tr, fixture_frames(fx))
    assert tr.engine.status() == 0 and tr.frame_count == nf
    np.testing.assert_array_equal(np.bincount(got[:, 0].astype(int), minlength=nf + 1),
                                  np.bincount(ref[:, 0].astype(int), minlength=nf + 1))
    compare_outputs(got, ref, box_atol=1e-9)
    # active_tracks: the last class's list (empty: class 2 is never populated); the per-class
    # lists carry the class-global ids of the rows
    assert tr.active_tracks == []
    lists = tr.per_class_active_tracks
    live = {t["id"] for c in range(NR_CLASSES) for t in lists[c]}
    assert set(got[got[:, 0] == nf][:, 5].astype(int)) <= live
    assert len(live) == sum(len(lists[c]) for c in range(NR_CLASSES))


@pytest.mark.parametrize("kind", ["deepocsort", "hybridsort"])
def test_id_counter_continues_across_instances(native, kind):
    """The class-level counter is shared: a second instance built WITHOUT resetting it (the
    constructor resets it, so it is set back by hand) goes on from the first one's ids."""
    from boxmot_amd import DeepOcSort, HybridSort

    fx = load(GOLDEN / ("perclass_deepoc_crowd24.npz" if kind == "deepocsort"
                        else "perclass_hybrid_crowd24.npz"))
    args = ast.literal_eval(str(fx["tracker_args"]))
    frames = fixture_frames(fx)[:3]
    cls = DeepOcSort if kind == "deepocsort" else HybridSort
    a = make_dropin(kind, args)
    run_dropin(a, frames)
    n = cls._id_count
    assert n > 1
    b = make_dropin(kind, args)
    assert cls._id_count == 1  # every constructor resets it, as the reference's does
    cls._id_count = n
    got = run_dropin(b, frames)
    assert got[:, 5].min() == n and cls._id_count == 2 * n - 1


@pytest.fixture(scope="module", params=["deepocsort", "hybridsort"])
def three(request, native):
    """The fixture scene at three seeds, the third starting four frames late: per frame the
    sequences' detections, and the rows of one per-class drop-in per sequence."""
    kind = request.param
    fx = load(GOLDEN / ("perclass_deepoc_crowd24.npz" if kind == "deepocsort"
                        else "perclass_hybrid_longterm.npz"))
    args = ast.literal_eval(str(fx["tracker_args"]))
    seqs = [fixture_frames(fx), fixture_frames(fx, seed=190), fixture_frames(fx, seed=191, start=4)]
    want = [run_dropin(make_dropin(kind, args), f) for f in seqs]
    return kind, args, seqs, want, int(fx["n_frames"])


def test_step_classes_equals_dropins_bitwise(three):
    """One engine of 3 x 3 class sequences: frames 1-4 step sequences [0, 2) only (the third has
    not started), later frames step sequence 0 and the chunk seq0 = 1, nseq = 2 in two calls."""
    import torch

    from boxmot_amd.engine import DeepOcsortEngine, HybridsortEngine

    kind, args, seqs, want, nf = three
    tr = make_dropin(kind, args)
    Eng = DeepOcsortEngine if kind == "deepocsort" else HybridsortEngine
    eng = Eng(n_seq=3 * NR_CLASSES, track_cap=256, det_cap=256, emb_dim=16, params=tr._params)
    by_t = [{t: (d, e) for t, d, e in f} for f in seqs]
    got = [[] for _ in seqs]

    def step(t, k0, k1):
        fr = [by_t[k][t] for k in range(k0, k1)]
        off = np.zeros(k1 - k0 + 1, np.int32)
        off[1:] = np.cumsum([d.shape[0] for d, _ in fr])
        d = torch.from_numpy(np.concatenate([x[0] for x in fr]).astype(np.float32)).cuda()
        e = torch.from_numpy(np.concatenate([x[1] for x in fr]).astype(np.float64)).cuda()
        o = torch.full((int(off[-1]), 8), np.nan, dtype=torch.float64, device="cuda")
        c = torch.zeros(k1 - k0, dtype=torch.int32, device="cuda")
        od = torch.from_numpy(off).cuda()
        if kind == "deepocsort":
            eng.step_classes(d, od, e, None, o, c, NR_CLASSES, seq0=k0, nseq=k1 - k0)
        else:
            eng.step_classes(d, od, e, o, c, NR_CLASSES, seq0=k0, nseq=k1 - k0)
        o, c = o.cpu().numpy(), c.cpu().numpy()
        for k in range(k0, k1):
            r = o[off[k - k0]: off[k - k0] + c[k - k0]]
            got[k].append(np.concatenate([np.full((r.shape[0], 1), t, np.float64), r], 1))

    for t in range(1, nf + 1):
        if t <= 4:
            step(t, 0, 2)
        else:
            step(t, 0, 1)
            step(t, 1, 3)
    assert eng.status() == 0
    for k in range(3):
        g = np.concatenate(got[k], 0)
        assert g.shape == want[k].shape and g.shape[0] > 50
        assert g.tobytes() == want[k].tobytes(), f"sequence {k} differs from its drop-in"
    eng.close()


def test_n_classes_is_fixed_by_the_first_call(native):
    torch = native
    from boxmot_amd.engine import DeepOcsortEngine, DeepOcsortParams

    eng = DeepOcsortEngine(n_seq=6, track_cap=16, det_cap=16, emb_dim=4, params=DeepOcsortParams())
    d = torch.zeros((2, 6), dtype=torch.float32, device="cuda")
    d[:, 2:4] = 10.0
    d[:, 4] = 0.9
    e = torch.ones((2, 4), dtype=torch.float64, device="cuda")
    off = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    o = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    c = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="multiple"):  # 6 sequences are no multiple of 4 classes
        eng.step_classes(d, off, e, None, o, c, 4, seq0=0, nseq=1)
    eng.step_classes(d, off, e, None, o, c, 3, seq0=0, nseq=1)
    with pytest.raises(ValueError, match="n_classes differs"):
        eng.step_classes(d, off, e, None, o, c, 2, seq0=0, nseq=1)
    with pytest.raises(ValueError):  # sequence 2 of an engine of two sequences of three classes
        eng.step_classes(d, off, e, None, o, c, 3, seq0=2, nseq=1)
    torch.cuda.synchronize()
    assert eng.status() == 0 and c.cpu().numpy().tolist() == [2]
    assert o.cpu().numpy()[:, 4].tolist() == [2.0, 1.0]  # both births of class 0, reversed list
    eng.close()


def test_id_map_capacity_latches(native):
    """An id map of 2 births per class sequence: the frame that brings the third birth of class 0
    latches BX_ERR_CAPACITY, reports no row and leaves the counter where it was."""
    from boxmot_amd.engine import HybridsortEngine, HybridsortParams

    eng = HybridsortEngine(n_seq=2, track_cap=16, det_cap=16, emb_dim=4, params=HybridsortParams())
    eng.classes_config(2, 2)
    d = np.zeros((2, 6), np.float32)
    d[:, 0] = [0, 500]
    d[:, 2] = [50, 550]
    d[:, 3] = 100
    d[:, 4] = 0.9
    e = np.eye(4)[:2]
    out, g = eng.update_classes_host(0, 2, d, e, 1)
    assert out.shape[0] == 2 and g == 3 and eng.status() == 0
    d3 = np.concatenate([d, d[:1] + np.array([1000, 0, 1000, 0, 0, 0], np.float32)])
    with pytest.raises(ValueError, match="capacity"):
        eng.update_classes_host(0, 2, d3, np.eye(4)[:3], g)
    assert eng.status() == 2 and eng.classes().id_count(0) == 3
    assert eng.classes().id_map(0, 0).tolist() == [1, 2]
    eng.close()


def test_map_grows_in_the_dropin(native):
    """ClassMapGuard moves the state into an engine with a larger id map before a class could pass
    it: a drop-in whose map holds 8 births equals one with the default map."""
    fx = load(GOLDEN / "perclass_hybrid_crowd24.npz")
    args = ast.literal_eval(str(fx["tracker_args"]))
    frames = fixture_frames(fx)[:12]
    a = make_dropin("hybridsort", args)
    want = run_dropin(a, frames)
    b = make_dropin("hybridsort", args)
    b._map.cap = 8
    d, e = frames[0][1], frames[0][2]
    b.engine = b._make_engine(e.shape[1])
    b.engine.classes_config(NR_CLASSES, 8)
    got = run_dropin(b, frames)
    assert b._map.cap > 8 and b.engine.classes().map_cap == b._map.cap
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------ the file flow
def dropin_file(kind, packed, fids, path, kw, n_classes):
    """process_sequence (val.py:337-353) with one fresh drop-in."""
    from boxmot_amd import (DeepOcSort, DeepOcSortPerClass, HybridSort, HybridSortPerClass,
                            motio)

    seq = motio.BinSequence(packed)
    if kind == "deepocsort":
        tr = DeepOcSortPerClass(nr_classes=n_classes, **kw) if n_classes else DeepOcSort(**kw)
    else:
        kw = dict(dict(reid_weights=None, device=None, half=False), **kw)
        tr = HybridSortPerClass(nr_classes=n_classes, **kw) if n_classes else HybridSort(**kw)
    out = []
    for fid in fids:
        d, e = seq.frame(fid)
        if not d.size:
            continue
        rows = np.asarray(tr.update(d, IMG, e), np.float64).reshape(-1, 8)
        if rows.shape[0]:
            out.append(motio.convert_to_mot_format(rows, int(fid)))
    motio.write_mot_results(path, np.vstack(out) if out else np.empty((0, 0)))
    assert tr.engine.status() == 0


def files(d, names):
    return {nm: (Path(d) / f"{nm}.txt").read_bytes() for nm in names}


@pytest.fixture(scope="module")
def packed3(native, tmp_path_factory):
    """Three small packed sequences (12, 20 and 16 frames, classes 0 / 1 / dropped 4), the second
    without detections in frames 7-9 (a frame gap)."""
    from boxmot_amd import motio
    from boxmot_amd.synth import SyntheticScene
    from tests.perclass_util import CLASSES

    tmp = tmp_path_factory.mktemp("packed3")
    packed = {}
    for q, nf in enumerate((12, 20, 16)):
        sc = SyntheticScene(n_obj=12 + 4 * q, seed=400 + q, emb_dim=16, emb_dtype="float64",
                            layout="crowded", conf_lo=0.31, jitter=3.0, p_det=0.8, classes=CLASSES)
        dets, embs = [], []
        for t in range(1, nf + 1):
            if q == 1 and t in (7, 8, 9):
                continue
            d, e, _ = sc.frame(t)
            dets.append(np.concatenate([np.full((d.shape[0], 1), t), d], 1))
            embs.append(e)
        packed[f"SEQ-{q}"] = motio.pack_arrays(np.concatenate(dets), np.concatenate(embs),
                                               tmp / f"SEQ-{q}.bxmot")
    return packed, tmp


@pytest.mark.parametrize("kind,per_class", [("hybridsort", False), ("hybridsort", True),
                                            ("deepocsort", True)])
def test_flow_equals_dropins_and_resident_equals_default(packed3, kind, per_class):
    from boxmot_amd import motio

    packed, tmp = packed3
    kw = dict(max_age=5, min_hits=2)
    if kind == "hybridsort":
        kw.update(det_thresh=0.3, longterm_reid_weight=0.3, TCM_first_step_weight=0.5)
    C = NR_CLASSES if per_class else 0
    tag = f"{kind}_{int(per_class)}"
    for nm, p in packed.items():
        dropin_file(kind, p, motio.BinSequence(p).frame_ids, tmp / tag / "single" / f"{nm}.txt", kw,
                    C)
    single = files(tmp / tag / "single", packed)
    ids = motio.run_sequences(kind, packed, tmp / tag / "default", tracker_kwargs=kw, n_classes=C)
    assert [len(v) for v in ids.values()] == [12, 17, 16]
    motio.run_sequences(kind, packed, tmp / tag / "resident", tracker_kwargs=kw, resident=True,
                        n_classes=C)
    a, b = files(tmp / tag / "default", packed), files(tmp / tag / "resident", packed)
    for nm in packed:
        assert len(single[nm]) > 0
        assert a[nm] == single[nm], f"{nm}: the batched flow differs from the drop-in"
        assert b[nm] == a[nm], f"{nm}: resident differs from the default path"
        rows = np.loadtxt(tmp / tag / "default" / f"{nm}.txt", delimiter=",")
        assert rows[:, 1].min() == 1  # every sequence's ids start at 1
        if per_class:
            assert set(rows[:, 7].astype(int)) == {0, 1}  # class 4 was dropped


def test_hybridsort_flow_frame_sizes_reach_centroid_mode(packed3):
    from boxmot_amd import motio

    packed, tmp = packed3
    kw = dict(det_thresh=0.3, asso_func="centroid", iou_threshold=0.7)
    # frames so small that every centre distance is many diagonals: nothing associates, while
    # the engine's default 1920 x 1080 does associate
    sizes = {nm: (64.0 + k, 48.0) for k, nm in enumerate(packed)}
    motio.run_sequences("hybridsort", packed, tmp / "cen_a", tracker_kwargs=kw, frame_sizes=sizes)
    motio.run_sequences("hybridsort", packed, tmp / "cen_b", tracker_kwargs=kw)
    motio.run_sequences("hybridsort", packed, tmp / "cen_c", tracker_kwargs=kw, frame_sizes=sizes,
                        resident=True)
    a, b, c = (files(tmp / d, packed) for d in ("cen_a", "cen_b", "cen_c"))
    assert a == c and any(a[nm] != b[nm] for nm in packed)

"""The device class split and id merge alone (include/bxclasses.h, engine.ClassSplit): the split
against a stable argsort bit for bit, the merge against a numpy restatement of the host
renumbering loop of bx_ocsort_update_classes_host, and the capacity / argument error paths."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def kept_class(cls, C):
    """cls_of: an integer in [0, C), else -1."""
    c = cls.astype(np.float32)
    ok = (c >= 0) & (c < C) & (c == np.floor(c))
    return np.where(ok, c, -1).astype(np.int64)


# S = 3, C = 4; every per-sequence row count of {0, 1, 37, 70} appears in some position
@pytest.mark.parametrize("F", [1, 5, 64])
@pytest.mark.parametrize("counts", [(0, 1, 37), (70, 0, 1), (37, 70, 0), (1, 37, 70)])
def test_split_equals_stable_argsort(native, F, counts):
    torch = native
    from boxmot_amd.engine import ClassSplit

    S, C = 3, 4
    rng = np.random.default_rng([F, *counts])
    n = sum(counts)
    dets = rng.uniform(0, 500, (n, 6)).astype(np.float32)
    dets[:, 5] = rng.choice([0, 1, 2, 3, -1, 4, 2.5], n).astype(np.float32)
    embs = rng.standard_normal((n, F))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    # the reference: per sequence a stable sort of the kept rows by class
    ro, rs, rd, re = [0], [], [], []
    for s in range(S):
        d = dets[off[s]: off[s + 1]]
        k = kept_class(d[:, 5], C)
        order = np.argsort(k, kind="stable")
        order = order[k[order] >= 0]
        rs.append(order)
        rd.append(d[order])
        re.append(embs[off[s]: off[s + 1]][order])
        for c in range(C):
            ro.append(ro[-1] + int((k == c).sum()))
    rs, rd, re = np.concatenate(rs), np.concatenate(rd), np.concatenate(re)
    m = ro[-1]
    assert m == rs.shape[0]
    cs = ClassSplit(S, C, emb_dim=F, row_cap=70)
    o_d = torch.full((n + 1, 6), -7.0, dtype=torch.float32, device="cuda")
    o_e = torch.full((n + 1, F), -7.0, dtype=torch.float64, device="cuda")
    o_o = torch.full((S * C + 1,), -7, dtype=torch.int32, device="cuda")
    o_s = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    cs.split(dev(torch, dets), dev(torch, off), dev(torch, embs), o_d, o_e, o_o, o_s)
    torch.cuda.synchronize()
    assert cs.status() == 0
    np.testing.assert_array_equal(o_o.cpu().numpy(), np.array(ro, np.int32))
    np.testing.assert_array_equal(o_s.cpu().numpy()[:m], rs.astype(np.int32))
    assert o_d.cpu().numpy()[:m].tobytes() == rd.tobytes()
    assert o_e.cpu().numpy()[:m].tobytes() == re.tobytes()
    # nothing behind the kept rows was written
    assert (o_d.cpu().numpy()[m:] == -7).all() and (o_e.cpu().numpy()[m:] == -7).all()
    assert (o_s.cpu().numpy()[m:] == -7).all()
    cs.close()


def test_split_odd_width_from_an_odd_row(native):
    """F = 5 with a call whose first row sits at an odd row of a larger array: source rows and
    destination rows differ in 16-byte phase for some rows and agree for others."""
    torch = native
    from boxmot_amd.engine import ClassSplit

    F, n = 5, 23
    rng = np.random.default_rng(5)
    dets = rng.uniform(0, 9, (n, 6)).astype(np.float32)
    dets[:, 5] = rng.choice([0, 1, 7], n)
    embs = rng.standard_normal((n + 1, F))
    big = dev(torch, embs)
    cs = ClassSplit(1, 2, emb_dim=F, row_cap=32)
    o_d = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    o_e = torch.zeros((n, F), dtype=torch.float64, device="cuda")
    o_o = torch.zeros(3, dtype=torch.int32, device="cuda")
    o_s = torch.zeros(n, dtype=torch.int32, device="cuda")
    cs.split(dev(torch, dets), dev(torch, np.array([0, n], np.int32)), big[1:], o_d, o_e, o_o, o_s)
    torch.cuda.synchronize()
    k = kept_class(dets[:, 5], 2)
    order = np.argsort(k, kind="stable")
    order = order[k[order] >= 0]
    m = order.shape[0]
    assert o_o.cpu().numpy().tolist() == [0, int((k == 0).sum()), m]
    assert o_e.cpu().numpy()[:m].tobytes() == embs[1:][order].tobytes()
    cs.close()


def test_split_row_cap_latches_and_stores_nothing(native):
    torch = native
    from boxmot_amd.engine import ClassSplit

    cs = ClassSplit(2, 2, emb_dim=0, row_cap=4)
    dets = np.zeros((7, 6), np.float32)
    dets[:, 5] = [0, 1, 0, 1, 0, 1, 1]
    o_d = torch.full((7, 6), -7.0, dtype=torch.float32, device="cuda")
    o_o = torch.zeros(5, dtype=torch.int32, device="cuda")
    o_s = torch.full((7,), -7, dtype=torch.int32, device="cuda")
    # sequence 0 has 5 rows > row_cap: split as if it had none; sequence 1 (2 rows) is kept
    cs.split(dev(torch, dets), dev(torch, np.array([0, 5, 7], np.int32)), None, o_d, None, o_o, o_s)
    torch.cuda.synchronize()
    assert cs.status() == 2  # BX_ERR_CAPACITY
    assert o_o.cpu().numpy().tolist() == [0, 0, 0, 0, 2]
    assert o_s.cpu().numpy().tolist() == [0, 1, -7, -7, -7, -7, -7]
    cs.close()


def merge_reference(frames, C, id0=1):
    """The gid loop of bx_ocsort_update_classes_host (bx_ocsort.hip:846-862) for one sequence:
    births in class order take the next class-global ids; rows are stacked in class order with
    column 4 sent through the map."""
    g, lids, gid, outs = id0, [id0] * C, [dict() for _ in range(C)], []
    for ids_now, rows in frames:
        for c in range(C):
            for l in range(lids[c], ids_now[c]):
                gid[c][l] = g
                g += 1
            lids[c] = ids_now[c]
        out = [r.copy() for c in range(C) for r in rows[c]]
        k = 0
        for c in range(C):
            for r in rows[c]:
                out[k][4] = gid[c][int(r[4])]
                k += 1
        outs.append(np.array(out).reshape(-1, 8))
    return outs, g


def test_merge_equals_host_renumbering(native):
    """Two sequences of C = 3 classes over three frames: births in several classes, a frame without
    births, a class whose out_count is 0, rows that name ids born in earlier frames."""
    torch = native
    from boxmot_amd.engine import ClassSplit

    S, C = 2, 3
    rng = np.random.default_rng(11)
    cs = ClassSplit(S, C, emb_dim=0, row_cap=16, map_cap=16)
    ids = np.ones((S, C), np.int32)  # the engines' next-id counters
    births = [  # per frame, per sequence, per class
        [[2, 0, 1], [0, 3, 0]],
        [[0, 0, 0], [1, 0, 2]],
        [[1, 2, 0], [0, 0, 0]],
    ]
    hist = [[], []]
    for f in range(3):
        c_off, c_out, c_cnt, det_off = [0], [], [], [0]
        per_seq = []
        for s in range(S):
            ids[s] += np.array(births[f][s], np.int32)
            rows = []
            for c in range(C):
                live = np.arange(1, ids[s, c])
                # class 1 of sequence 0 never reports a row (out_count 0); the rest report every
                # live id in reversed order, as the engines do
                n = 0 if (s, c) == (0, 1) else live.shape[0]
                r = rng.uniform(0, 100, (n, 8))
                r[:, 4] = live[::-1][:n]
                rows.append(r)
                cap = n + (c % 2)  # the class's region of the step's out may be larger
                c_out.append(np.concatenate([r, np.full((cap - n, 8), -1.0)]))
                c_off.append(c_off[-1] + cap)
                c_cnt.append(n)
            per_seq.append(rows)
            hist[s].append((ids[s].copy(), rows))
            det_off.append(c_off[-1])
        total = c_off[-1]
        out = torch.full((total + 1, 8), -7.0, dtype=torch.float64, device="cuda")
        cnt = torch.full((S,), -7, dtype=torch.int32, device="cuda")
        cs.merge(dev(torch, np.array(c_off, np.int32)), dev(torch, np.concatenate(c_out)),
                 dev(torch, np.array(c_cnt, np.int32)), dev(torch, ids.reshape(-1)),
                 dev(torch, np.array(det_off, np.int32)), out, cnt)
        torch.cuda.synchronize()
        assert cs.status() == 0
        o, k = out.cpu().numpy(), cnt.cpu().numpy()
        for s in range(S):
            want, g = merge_reference(hist[s], C)
            assert k[s] == want[-1].shape[0]
            assert o[det_off[s]: det_off[s] + k[s]].tobytes() == want[-1].tobytes()
            assert (o[det_off[s] + k[s]: det_off[s + 1]] == -7).all()
            assert cs.id_count(s) == g
    # the maps: local id -> class-global id
    assert cs.id_map(0, 0).tolist() == [1, 2, 4] and cs.id_map(0, 1).tolist() == [5, 6]
    assert cs.id_map(0, 2).tolist() == [3]
    cs.close()


def test_merge_chunk_and_map_capacity(native):
    """seq0 = 1 of S = 2 (the other sequence's state stays untouched); then births past map_cap:
    BX_ERR_CAPACITY, out_count 0, no row, counter and map unchanged."""
    torch = native
    from boxmot_amd.engine import ClassSplit

    cs = ClassSplit(2, 2, emb_dim=0, row_cap=8, map_cap=3)
    ids = np.array([1, 1, 3, 2], np.int32)  # sequence 1: two births in class 0, one in class 1
    rows = np.zeros((3, 8))
    rows[:, 4] = [2, 1, 1]
    out = torch.full((3, 8), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    args = (dev(torch, np.array([0, 2, 3], np.int32)), dev(torch, rows),
            dev(torch, np.array([2, 1], np.int32)))
    cs.merge(*args, dev(torch, ids), dev(torch, np.array([0, 3], np.int32)), out, cnt, seq0=1,
             nseq=1)
    torch.cuda.synchronize()
    assert cs.status() == 0 and cnt.cpu().numpy().tolist() == [3]
    assert out.cpu().numpy()[:, 4].tolist() == [2, 1, 3]
    assert cs.id_count(0) == 1 and cs.id_count(1) == 4 and cs.id_map(0, 0).size == 0
    ids[2] = 5  # class 0 of sequence 1 would hold 4 births > map_cap 3
    out.fill_(-7.0)
    cs.merge(*args, dev(torch, ids), dev(torch, np.array([0, 3], np.int32)), out, cnt, seq0=1,
             nseq=1)
    torch.cuda.synchronize()
    assert cs.status() == 2  # BX_ERR_CAPACITY
    assert cnt.cpu().numpy().tolist() == [0] and (out.cpu().numpy() == -7).all()
    assert cs.id_count(1) == 4 and cs.id_map(1, 0).tolist() == [1, 2]
    cs.close()


def test_argument_errors(native):
    torch = native
    from boxmot_amd.engine import ClassSplit

    with pytest.raises(ValueError):
        ClassSplit(1, 0)
    with pytest.raises(ValueError):
        ClassSplit(1, 2, row_cap=4096)  # > BX_CLASSES_ROW_MAX
    cs = ClassSplit(2, 2, emb_dim=4, row_cap=8)
    z = torch.zeros(64, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):  # more sequences than the state has
        cs.split(z, z, z, z, z, z, z, nseq=3)
    with pytest.raises(ValueError):  # emb_dim 4 needs embs
        cs.split(z, z, None, z, None, z, z)
    with pytest.raises(ValueError):
        cs.merge(z, z, z, z, z, z, z, seq0=1, nseq=2)
    cs.close()

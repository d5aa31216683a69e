"""The shared feeder's float64 / 10-column mode (bx_feed_create_shared_fmt) as an op, against a
numpy restatement: gathered dets compared as bytes with ``astype(float64)`` of the packed float32
rows, runs of 1, 31, 32 and 33 rows (around BX_FEED_ROW_ALIGN), a frame index with two runs
separated by an unstepped sequence, a shared source, appends from 10-column rows against the
8-column mode's, the guard rows, the latched BX_ERR_CAPACITY, and (0, 8) against
bx_feed_create_shared."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 3
# detections of sequences 0..3 at frame indices 0..4; sequences 2 and 3 read the rows of 0 and 1.
# t=0: one run of 1 row; t=1: 31 = 20 + 11; t=2: 32; t=3: 33 = 30 + 3 and, behind the unstepped
# sequence 2, a second run (sequence 3); t=4: nothing
COUNTS = np.array([[1, 0, 0, 0],
                   [20, 11, 0, 0],
                   [0, 32, 0, 0],
                   [30, 3, 0, 3],
                   [0, 0, 0, 0]])
SOURCE = [0, 1, 0, 1]
GUARD = 3


@pytest.fixture(scope="module")
def native():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return torch


def data():
    rng = np.random.default_rng(0xF64)
    dets, embs, tables = [], [], []
    for k in range(4):
        q = SOURCE[k]
        cnt = COUNTS[:, k]
        src_cnt = COUNTS[:, q]
        start = np.concatenate([[0], np.cumsum(src_cnt)[:-1]])
        assert all(cnt[t] <= src_cnt[t] for t in range(len(cnt)))
        tables.append((start.astype(np.int64), cnt.astype(np.int64),
                       np.arange(1, len(cnt) + 1, dtype=np.int64) * 10 + k))
        if q == k:
            n = int(src_cnt.sum())
            # values that are no float32 values before the cast, ids and classes as integers
            d = rng.uniform(0.0, 1000.0, (n, 6))
            dets.append(d.astype(np.float32))
            embs.append(rng.standard_normal((n, F)))
        else:
            dets.append(None)
            embs.append(None)
    return dets, embs, tables


def feeders(**kw):
    from boxmot_amd.engine import SharedSequenceFeeder

    dets, embs, tables = data()
    return SharedSequenceFeeder(dets, embs, tables, F, guard_rows=GUARD, source=SOURCE,
                                **kw), dets, embs, tables


def test_gather_float64_against_numpy(native):
    fd, dets, embs, tables = feeders(det_f64=True, out_cols=10)
    try:
        assert fd.det_f64 and fd.out_cols == 10
        assert [[r[:3] for r in runs] for runs in fd.schedule] == \
            [[(0, 1, 1)], [(0, 2, 31)], [(1, 1, 32)], [(0, 2, 33), (3, 1, 3)], []]
        for t, runs in enumerate(fd.schedule):
            fd.gather(t)
            for r, (k0, ns, rows, pd, po, pe, pout, pcnt) in enumerate(runs):
                assert pd % 256 == 0 and pe % 256 == 0 and pout % 256 == 0
                d, off, e = fd.read_run(t, r)
                assert d.dtype == np.float64 and d.shape == (rows, 6)
                want_d, want_e, want_off = [], [], [0]
                for k in range(k0, k0 + ns):
                    a, n = int(tables[k][0][t]), int(tables[k][1][t])
                    want_d.append(dets[SOURCE[k]][a: a + n].astype(np.float64))
                    want_e.append(embs[SOURCE[k]][a: a + n])
                    want_off.append(want_off[-1] + n)
                assert d.tobytes() == np.concatenate(want_d).tobytes()
                assert e.tobytes() == np.concatenate(want_e).tobytes()
                assert off.tolist() == want_off
    finally:
        fd.close()


def drive(fd, rng_seed=5, bad=None):
    """write_run + append of every frame index with random out rows of the feeder's width whose
    first 8 columns come from the same stream; ``bad``: (t, r, value) an out_count to poison."""
    rng = np.random.default_rng(rng_seed)
    for t, runs in enumerate(fd.schedule):
        fd.gather(t)  # (writes the det_off the append finds each sequence's rows by)
        for r, (k0, ns, rows, *_) in enumerate(runs):
            out8 = rng.uniform(-50.0, 2000.0, (rows, 8))
            out = np.full((rows, fd.out_cols), 7.25)
            out[:, :8] = out8
            cnt = np.array([int(c) for c in COUNTS[t, k0: k0 + ns]], np.int32)
            cnt[0] = max(cnt[0] - 1, 0)  # fewer rows than detections
            if bad and bad[:2] == (t, r):
                cnt[-1] = bad[2]
            fd.write_run(t, r, out, cnt)
        if runs:
            fd.append(t)


def test_append_stride_10_equals_8_and_guard(native):
    a, *_ = feeders(det_f64=True, out_cols=10)
    b, *_ = feeders()
    try:
        drive(a)
        drive(b)
        ra, rb = a.raw_results(), b.raw_results()
        for x, y in zip(ra, rb):
            assert x.tobytes() == y.tobytes()
        assert a.status() == 0 and ra[2].sum() > 80
        assert ra[0][-GUARD:].tobytes() == b"\xff" * (GUARD * 72)
        k = 1  # rows are frame, id, l, t, w, h, 1, cls, conf in append order
        assert set(ra[0][ra[1][k]: ra[1][k] + ra[2][k], 0].tolist()) == {21.0, 31.0, 41.0}
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("value", [-1, 4])
def test_out_count_outside_range_latches(native, value):
    fd, *_ = feeders(det_f64=True, out_cols=10)
    try:
        drive(fd, bad=(3, 1, value))  # sequence 3 has 3 detections there
        assert fd.status() == 2  # BX_ERR_CAPACITY
        res, base, n = fd.raw_results()
        assert n[3] == 0 and res[-GUARD:].tobytes() == b"\xff" * (GUARD * 72)
    finally:
        fd.close()


def test_plain_mode_through_new_entry_is_identical(native):
    """(0, 8) through bx_feed_create_shared_fmt against bx_feed_create_shared: the same device
    bytes, runs, gathers and results; other modes are refused."""
    from boxmot_amd import _native as N
    from boxmot_amd.engine import SharedSequenceFeeder

    class ViaFmt(SharedSequenceFeeder):
        def __init__(self, dets, embs, tables, emb_dim, guard_rows, source):
            self.source = list(source)
            self._build(dets, embs, tables, emb_dim, None, guard_rows, source, (0, 8))

    dets, embs, tables = data()
    a = ViaFmt(dets, embs, tables, F, GUARD, SOURCE)
    b, *_ = feeders()
    try:
        assert not a.det_f64 and a.out_cols == 8 and a.device_bytes == b.device_bytes
        assert [[r[:3] for r in runs] for runs in a.schedule] == \
            [[r[:3] for r in runs] for runs in b.schedule]
        for t, runs in enumerate(a.schedule):
            a.gather(t)
            b.gather(t)
            for r in range(len(runs)):
                for x, y in zip(a.read_run(t, r), b.read_run(t, r)):
                    assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        drive(a)
        drive(b)
        for x, y in zip(a.raw_results(), b.raw_results()):
            assert x.tobytes() == y.tobytes()
    finally:
        a.close()
        b.close()
    for fmt in ((0, 9), (2, 8), (1, 7), (0, 0)):
        with pytest.raises(ValueError):
            ViaFmt.__new__(ViaFmt)._build(dets, embs, tables, F, None, 0, SOURCE, fmt)
    h = C.c_void_p()
    assert N.load().bx_feed_create_shared_fmt(0, F, None, None, None, None, None, None, 0, None,
                                              0, 8, C.byref(h)) == 1

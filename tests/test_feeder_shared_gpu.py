"""The feeder whose sequences share packed rows (bx_feed_create_shared) as an op: a feeder with
source = [0, 1, 2, 0, 1, 2] against a plain six-sequence feeder with duplicated uploads — every
gathered run, the appends and the results, bitwise — and the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests.test_deepocsort_flow_gpu import drive_appends, host_runs, ragged_set

pytestmark = pytest.mark.gpu

SOURCE = [0, 1, 2, 0, 1, 2]


@pytest.fixture(scope="module")
def native():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return torch


def six(F, pick):
    """Three sequences of the ragged set twice.  The copies keep their own frame tables: copy 4
    is not stepped at its first frame index with detections and copy 5 iterates one frame index
    less, so the runs differ from the sources'."""
    dets, embs, tables = ragged_set(F, 1)
    dets, embs, tables = ([x[k] for k in pick] for x in (dets, embs, tables))
    copies = [tuple(np.array(c) for c in tb) for tb in tables]
    first = int(np.flatnonzero(copies[1][1])[0]) if copies[1][1].any() else None
    if first is not None:
        copies[1][1][first] = 0
    copies[2] = tuple(c[:-1] for c in copies[2])
    return dets, embs, tables + copies


@pytest.mark.parametrize("pick", [(0, 2, 3), (0, 1, 2)], ids=["ragged", "with-empty"])
@pytest.mark.parametrize("F", [1, 20, 130])
def test_shared_feeder_equals_duplicated_uploads(native, F, pick):
    """F = 1 and 130 leave tails that are no multiple of the 2-wide copy; odd F puts rows off the
    16-byte phase.  (0, 1, 2) has a source without any row."""
    from boxmot_amd.engine import SequenceFeeder, SharedSequenceFeeder

    dets, embs, tables = six(F, pick)
    plain = SequenceFeeder(dets * 2, embs * 2, tables, F, guard_rows=3)
    shared = SharedSequenceFeeder(dets + [None] * 3, embs + [None] * 3, tables, F, guard_rows=3,
                                  source=SOURCE)
    assert shared.source == SOURCE and shared.schedule != [] and shared.n_frames == plain.n_frames
    assert [[r[:3] for r in runs] for runs in shared.schedule] == \
        [[r[:3] for r in runs] for runs in plain.schedule]
    rows = sum(d.shape[0] for d in dets)
    # one copy of the packed rows less, one int32 map more
    assert plain.device_bytes - shared.device_bytes == rows * (24 + 8 * F) - 4 * len(SOURCE)
    seen = 0
    for t in range(plain.n_frames):
        assert [(r[0], r[0] + r[1]) for r in shared.schedule[t]] == host_runs(tables, t)
        plain.gather(t)
        shared.gather(t)
        for r in range(len(plain.schedule[t])):
            for a, b in zip(shared.read_run(t, r), plain.read_run(t, r)):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), \
                    (t, r)
            seen += 1
    assert seen >= 9
    fed = [drive_appends(f, tables, np.random.default_rng(7)) for f in (shared, plain)]
    assert all(len(a) == len(b) for a, b in zip(*fed))
    for a, b in zip(shared.raw_results(), plain.raw_results()):
        assert a.tobytes() == b.tobytes()
    assert shared.status() == 0 and plain.status() == 0
    assert sum(r.shape[0] for r in shared.results()) > 0
    shared.close()
    plain.close()


def test_shared_feeder_refusals(native):
    from boxmot_amd import _native as N
    from boxmot_amd.engine import SequenceFeeder, SharedSequenceFeeder

    dets, embs, tables = six(4, (0, 2, 3))
    args = (dets + [None] * 3, embs + [None] * 3, tables, 4)
    for bad in ([0, 1, 2, 4, 1, 2],      # src[k] > k
                [0, 0, 2, 1, 1, 2],      # src[src[3]] != src[3]: sequence 1 is no source
                [0, 1, 2, 0, -1, 2]):    # out of range
        with pytest.raises(ValueError, match="src"):
            SharedSequenceFeeder(*args, source=bad)
    # an entry of a copy that lies outside its source's rows: sequence 3 reads sequence 1's
    with pytest.raises(ValueError, match="outside"):
        big = list(tables)
        big[3] = (tables[3][0] + dets[1].shape[0], tables[3][1], tables[3][2])
        SharedSequenceFeeder(*args[:2], big, 4, source=[0, 1, 2, 1, 1, 2])
    f = SharedSequenceFeeder(*args, source=SOURCE)
    L = f._L
    d = np.zeros((dets[0].shape[0], 6), np.float32)
    e = np.zeros((dets[0].shape[0], 4), np.float64)
    assert L.bx_feed_upload_host(f._h, 3, d.ctypes.data, e.ctypes.data) == 1  # not a source
    assert b"source" in L.bx_last_error()
    assert L.bx_feed_upload_host(f._h, 0, d.ctypes.data, e.ctypes.data) == 0
    assert L.bx_feed_create_shared(6, 4, None, None, None, None, None, None, 0, None,
                                   C.byref(C.c_void_p())) == 1
    f.close()
    # source=None is the plain feeder, and bx_feed_create's layout is what it was
    a = SharedSequenceFeeder(dets * 2, embs * 2, tables, 4)
    b = SequenceFeeder(dets * 2, embs * 2, tables, 4)
    assert a.source is None and a.device_bytes == b.device_bytes
    assert isinstance(N.EXPORTS, list) and "bx_feed_create_shared" in N.EXPORTS
    a.close()
    b.close()

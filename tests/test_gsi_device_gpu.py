"""boxmot_amd.postprocessing.gsi_device on the GPU: GSI from result slots in device memory
(what ``SequenceFeeder.results_device`` hands out) to rows ``MotEvaluator.run_device`` takes.

One buffer with six slots, interval 5, tau 10, id 1 in every slot (equal ids in different slots
must not merge); slack rows between the slots and two guard rows hold NaN and must never reach a
result.  Expected per slot: ``gsi_batch([slot_rows], 5, 10)[0]`` (tests/test_gsi_gpu.py pins that
batching does not change bits), put through ``np.trunc(x) + 0.0`` when ``truncate`` is on: what
``np.savetxt(fmt="%d ...")`` followed by ``np.loadtxt`` makes of it.  Every comparison is on the
uint64 views.

The error path.  A NaN frame latches the pivot check (tests/test_gsi_paths_gpu.py) and raises
LinAlgError in the host path and here, with the same message content.  A duplicated (id, frame)
does NOT: with the reference's jitter the pivot of the second copy is 2e-10 (K + 1e-10 * I with two
equal rows: (1 + 1e-10) - 1 / (1 + 1e-10)), far above the rounding of the factorisation, so
``gaussian_smooth`` returns rows for it and ``gsi_device`` must return the same bits; the test
holds ``gsi_device`` to whatever ``gaussian_smooth`` does on those rows.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INTERVAL, TAU = 5, 10.0
SLACK, GUARD = 2, 2


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return t


def mot_rows(ident, frames, x=300.0, y=200.0, seed=0):
    """[n, 9] result rows of one id: a box drifting from (x, y) with a little jitter."""
    rng = np.random.default_rng([seed, int(ident)])
    f = np.asarray(frames, np.float64)
    r = np.empty((f.shape[0], 9))
    r[:, 0], r[:, 1] = f, ident
    r[:, 2] = x + 0.01 * f + rng.normal(0, 0.3, f.shape[0])
    r[:, 3] = y - 0.01 * f + rng.normal(0, 0.3, f.shape[0])
    r[:, 4] = 40 + rng.normal(0, 0.3, f.shape[0])
    r[:, 5] = 90 + rng.normal(0, 0.3, f.shape[0])
    r[:, 6], r[:, 7], r[:, 8] = 1.0, 0.0, 0.9
    return r


def make_slots():
    s1 = mot_rows(1, [1, 2, 5, 9, 14], seed=1)  # gaps of 3 and 4 are filled, the gap of 5 is not
    s3 = np.concatenate([mot_rows(3, [7], seed=3), mot_rows(1, [6, 4], seed=3)])  # descending
    s4 = mot_rows(1, [f for f in range(1, 201) if f % 7], seed=4)  # 200 rows after filling
    s5 = mot_rows(1, [2, 3, 4, 7, 8, 9], x=-3.6, y=-0.4, seed=5)   # trunc gives -3 and -0
    empty = np.empty((0, 9))
    return [s1, empty, s3, s4, s5, empty]


def layout(slots, stride):
    """(buffer [rows, stride], base, n): NaN everywhere but columns 0..8 of the slots' rows."""
    n = np.array([s.shape[0] for s in slots], np.int64)
    base = np.zeros(len(slots), np.int64)
    at = 1  # (a slack row in front: no slot starts at row 0)
    for q, s in enumerate(slots):
        base[q] = at
        at += s.shape[0] + SLACK
    buf = np.full((at + GUARD, stride), np.nan)
    for q, s in enumerate(slots):
        buf[base[q]: base[q] + n[q], :9] = s
    return buf, base, n


@pytest.fixture(scope="module")
def slots():
    return make_slots()


@pytest.fixture(scope="module")
def expected(torch, slots):
    """Per slot the float rows of the host path; computed once and left unchanged."""
    from boxmot_amd.postprocessing import gsi_batch

    out = [gsi_batch([s], INTERVAL, TAU)[0] if s.shape[0] else np.empty((0, 9)) for s in slots]
    for e in out:
        e.setflags(write=False)
    assert [e.shape[0] for e in out] == [10, 0, 4, 200, 8, 0]
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(torch, slots, stride, truncate, pointers=False):
    from boxmot_amd.postprocessing import gsi_device

    buf, base, n = layout(slots, stride)
    d = [torch.from_numpy(x).cuda() for x in (buf, base, n)]
    if pointers:
        out = gsi_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(slots),
                         interval=INTERVAL, tau=TAU, row_stride=stride, truncate=truncate)
    else:
        out = gsi_device(*d, interval=INTERVAL, tau=TAU, row_stride=stride, truncate=truncate)
    rows, ob, on = out
    assert rows.is_cuda and ob.is_cuda and on.is_cuda
    assert rows.dtype == torch.float64 and ob.dtype == torch.int64 and on.dtype == torch.int64
    assert rows.shape[1] == 9 and ob.shape == (len(slots),) and on.shape == (len(slots),)
    return rows.cpu().numpy(), ob.cpu().numpy(), on.cpu().numpy()


def check(rows, ob, on, expected, truncate):
    want = [np.trunc(e) + 0.0 if truncate else np.asarray(e) for e in expected]
    counts = [w.shape[0] for w in want]
    print("rows per slot", on.tolist(), "base", ob.tolist())
    assert on.tolist() == counts
    assert ob.tolist() == np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()  # consecutive
    assert rows.shape[0] == sum(counts)
    assert not np.isnan(rows).any()
    for q, w in enumerate(want):
        got = rows[ob[q]: ob[q] + on[q]]
        assert np.array_equal(bits(got), bits(w)), f"slot {q}"
    if truncate:
        assert not np.signbit(rows[rows == 0.0]).any()  # no -0.0
        assert np.array_equal(rows, np.trunc(rows))
        assert (rows[ob[4]: ob[4] + on[4], 3] == 0.0).any()  # the negative fraction was there


@pytest.mark.parametrize("stride,truncate", [(9, True), (10, True), (9, False), (10, False)],
                         ids=["stride9", "stride10", "stride9-float", "stride10-float"])
def test_slots_match_gsi_batch(torch, slots, expected, stride, truncate):
    check(*run(torch, slots, stride, truncate), expected, truncate)


def test_raw_pointers_need_n_seq(torch, slots, expected):
    from boxmot_amd.postprocessing import gsi_device

    check(*run(torch, slots, 9, True, pointers=True), expected, True)
    buf, base, n = (torch.from_numpy(x).cuda() for x in layout(slots, 9))
    with pytest.raises(ValueError, match="n_seq"):
        gsi_device(buf.data_ptr(), base.data_ptr(), n.data_ptr())


def test_untruncated_fraction_is_negative(expected):
    """Slot 5 is what it is for: some value truncates to a negative zero before the + 0.0."""
    assert np.signbit(np.trunc(expected[4])[np.trunc(expected[4]) == 0.0]).any()


def test_all_empty(torch, slots):
    rows, ob, on = run(torch, [s[:0] for s in slots], 9, True)
    assert rows.shape == (0, 9) and ob.tolist() == [0] * 6 and on.tolist() == [0] * 6


def test_arguments_are_validated(torch, slots):
    from boxmot_amd.postprocessing import gsi_device

    buf, base, n = (torch.from_numpy(x).cuda() for x in layout(slots, 9))
    with pytest.raises(ValueError, match="contiguous CUDA"):
        gsi_device(buf.cpu(), base, n)
    with pytest.raises(ValueError, match="contiguous CUDA"):
        gsi_device(buf, base.int(), n)
    with pytest.raises(ValueError, match="outside the rows tensor"):
        gsi_device(buf, base + buf.shape[0], n)
    with pytest.raises(ValueError, match="row_stride"):
        gsi_device(buf, base, n, row_stride=7)


def test_nan_frame_raises_linalgerror(torch):
    """The host path's error, with its message content: the id and 'not positive definite'."""
    from boxmot_amd.postprocessing import gaussian_smooth, gsi_device

    bad = mot_rows(1, [1, 2, 3, 4, 5, 6], seed=7)
    bad[3, 0] = np.nan
    with pytest.raises(np.linalg.LinAlgError, match=r"id 1 \(.*not positive definite"):
        gaussian_smooth(bad, TAU)
    buf, base, n = (torch.from_numpy(x).cuda()
                    for x in layout([np.empty((0, 9)), bad], 9))
    with pytest.raises(np.linalg.LinAlgError, match=r"id 1 \(.*not positive definite"):
        gsi_device(buf, base, n, interval=INTERVAL, tau=TAU)


def test_duplicate_frame_as_gaussian_smooth(torch):
    """An id twice in a frame: gsi_device does what gaussian_smooth does on those rows (module
    docstring: the jitter keeps the pivot positive, so that is rows, not LinAlgError)."""
    from boxmot_amd.postprocessing import gaussian_smooth, gsi_batch, gsi_device

    dup = mot_rows(1, [1, 2, 2, 3, 4], seed=8)
    assert np.isfinite(gaussian_smooth(dup, TAU)).all()  # (no LinAlgError: measured on the GPU)
    buf, base, n = (torch.from_numpy(x).cuda() for x in layout([dup], 9))
    rows, ob, on = (x.cpu().numpy() for x in gsi_device(buf, base, n, interval=INTERVAL, tau=TAU))
    want = np.trunc(gsi_batch([dup], INTERVAL, TAU)[0]) + 0.0
    assert ob.tolist() == [0] and on.tolist() == [want.shape[0]]
    assert np.array_equal(bits(rows), bits(want))

"""GPU checks of the GSI smoothing paths no fixture reaches (siblings of test_gsi_gpu.py, whose
tolerance rule ``min(4 * solver_spread, 1e-3)`` and ``check_smoothed`` are reused unchanged).

* Slot reuse of the persistent blocked kernel: more blocked tracklets than its 512 slots, and
  more than its 1 GiB slot budget holds.  The kernel promises bits that depend only on a
  tracklet's length and path, so a tracklet must return the same bits wherever it lands.
* BX_GSI_MAX_N: 4096 rows are factored, 4097 are refused before any launch.
* The pivot latch: a NaN frame makes a later pivot NaN, ``!(d > 0)`` latches BX_ERR_INVALID for
  that tracklet alone (an ordinary error return), its rows come out unsmoothed, and Python raises
  LinAlgError as the reference does.
* The argument checks of the ``bx_gsi_*`` entry points: status code and ``bx_last_error`` text.

Where no fixture exists the reference is ``cpu_smooth``: scikit-learn's formula restated in
float64 (lower Cholesky of K + 1e-10*I, mean = K @ alpha), with its spread against the three
solvers of ``make_golden_gsi.solver_spread`` measured on the CPU alone.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gsi_gpu import GOLDEN, check_smoothed

pytestmark = pytest.mark.gpu

OK, INVALID, CAPACITY = 0, 1, 2  # bx_status (include/bxassoc.h)
LDS_N, MAX_N, MAX_SLOTS, SLOT_BUDGET = 176, 4096, 512, 1 << 30  # include/bxgsi.h, bx_gsi.hip
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def lib():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    return _native.load()


def last_error(lib):
    return lib.bx_last_error().decode(errors="replace")


def tracklet(rng, ident, n, start=1):
    """n rows on dense frames: a random walk of the box, 2 px per frame (as the fixtures')."""
    box = np.array([rng.uniform(100, 1500), rng.uniform(100, 800), rng.uniform(40, 120),
                    rng.uniform(80, 260)]) + np.cumsum(rng.normal(0.0, 2.0, (n, 4)), 0)
    return np.concatenate([start + np.arange(n, dtype=float)[:, None], np.full((n, 1), float(ident)),
                           box, rng.uniform(0.3, 1.0, (n, 1)), np.zeros((n, 1))], 1)


def cpu_smooth(tr, tau, rng):
    """(mean [n, 4], spread) of one tracklet: the reference's formula in float64, and the largest
    difference of the mean between it and three other float64 solves of the same system."""
    from scipy.linalg import cho_factor, cho_solve

    n = tr.shape[0]
    ls = np.clip(tau * np.log(tau**3 / n), tau**-1, tau**2)
    t = tr[:, 0] / ls
    K = np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2)
    Kj = K + 1e-10 * np.eye(n)
    y = tr[:, 2:6]
    mean = K @ cho_solve(cho_factor(Kj, lower=True), y)
    p = rng.permutation(n)
    inv = np.argsort(p)
    alphas = [np.linalg.solve(Kj, y), cho_solve(cho_factor(Kj, lower=False), y),
              cho_solve(cho_factor(Kj[p][:, p], lower=True), y[p])[inv]]
    return mean, max(float(np.abs(K @ a - mean).max()) for a in alphas)


def cpu_reference(rows, tau, seed):
    """{"smoothed", "solver_spread"} for rows grouped by ascending id: what check_smoothed takes."""
    rng = np.random.default_rng(seed)
    out = np.concatenate([rows[:, :2], np.zeros((rows.shape[0], 4)), rows[:, 6:8],
                          np.full((rows.shape[0], 1), -1.0)], 1)
    worst = 0.0
    for ident in np.unique(rows[:, 1]):
        m = rows[:, 1] == ident
        out[m, 2:6], spread = cpu_smooth(rows[m], tau, rng)
        worst = max(worst, spread)
    return {"smoothed": out, "solver_spread": worst}


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def offsets(lens):
    return np.r_[0, np.cumsum(lens)].astype(np.int32)


def smooth_direct(lib, rows, off, tau, force=0, ncol=None, short=0):
    """bx_gsi_smooth on host rows -> (rc, out [n, 9] prefilled with SENTINEL, status prefilled
    with -7).  `short`: bytes to understate the workspace by (it is allocated in full)."""
    import torch

    off = np.ascontiguousarray(off, np.int32)
    nt = off.shape[0] - 1
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    nbytes = C.c_size_t(0)
    lib.bx_gsi_workspace_bytes(off.ctypes.data, nt, force, C.byref(nbytes))
    ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device="cuda")
    out = torch.full((rows.shape[0], 9), SENTINEL, dtype=torch.float64, device="cuda")
    status = torch.full((max(nt, 1),), -7, dtype=torch.int32, device="cuda")
    rc = lib.bx_gsi_smooth(d_rows.data_ptr(), rows.shape[1] if ncol is None else ncol,
                           off.ctypes.data, nt, float(tau), force, ws.data_ptr(),
                           nbytes.value - short, out.data_ptr(), status.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), status.cpu().numpy()[:nt]


# ------------------------------------------------------------------------------- slot reuse
def test_slot_reuse_beyond_512_blocked_tracklets(lib):
    """600 tracklets of 1..40 rows, all forced onto the blocked path: 512 persistent workgroups,
    so 88 of them factor a second tracklet (of another length) in the same slot and LDS.  The
    same tracklets with reversed ids land in other slots behind other predecessors, and 20 of
    them run alone; all three return the same bits, and they match the CPU restatement."""
    from boxmot_amd.postprocessing import _gaussian_smooth

    rng = np.random.default_rng(601)
    T, tau = 600, 10.0
    assert T > MAX_SLOTS
    lens = [k % 40 + 1 for k in range(T)]
    off = offsets(lens)
    rows = np.concatenate([tracklet(rng, k + 1, n, int(rng.integers(1, 50)))
                           for k, n in enumerate(lens)])
    a = _gaussian_smooth(rows, tau, force_blocked=True)
    assert np.array_equal(a[:, 1], rows[:, 1])

    rev = rows.copy()
    rev[:, 1] = T + 1 - rows[:, 1]
    b = _gaussian_smooth(rev, tau, force_blocked=True)
    cols = [0, 2, 3, 4, 5, 6, 7, 8]
    for k in range(T):
        bk = b[b.shape[0] - off[k + 1]: b.shape[0] - off[k]]
        assert np.all(bk[:, 1] == T - k)
        assert same_bits(a[off[k]: off[k + 1]][:, cols], bk[:, cols]), f"tracklet {k}, reversed"

    sample = sorted({0, T - 1, MAX_SLOTS, MAX_SLOTS + 1, 555} | set(range(7, T, 41)))
    assert len(sample) == 20 and sum(k >= MAX_SLOTS for k in sample) >= 3
    for k in sample:
        alone = _gaussian_smooth(rows[off[k]: off[k + 1]], tau, force_blocked=True)
        assert same_bits(a[off[k]: off[k + 1]], alone), f"tracklet {k}, alone"
    check_smoothed(a, cpu_reference(rows, tau, 602), "600 blocked tracklets of 1..40 rows")


def test_slot_reuse_through_the_budget(lib):
    """One 2049-row tracklet (the `deep` fixture's) sizes every slot at 16.9 MB, so the 1 GiB
    budget holds 63 slots for 71 blocked tracklets: the workspace size proves the reuse.  Every
    tracklet returns the bits of its own single call, and the long one matches the reference."""
    from boxmot_amd import gaussian_smooth

    z = dict(np.load(GOLDEN / "gsi_deep.npz"))
    tau = float(z["tau"])
    deep = z["interpolated"][z["interpolated"][:, 1] == 2]
    assert deep.shape[0] == 2049
    rng = np.random.default_rng(71)
    lens = [2049] + [177 + k % 24 for k in range(70)]
    assert min(lens) > LDS_N  # the default launch sends every one to the blocked path
    off = offsets(lens)
    rows = np.concatenate([deep] + [tracklet(rng, 3 + k, n) for k, n in enumerate(lens[1:])])

    slot_bytes = 8 * ((2049 * 2050 // 2 + 4 * 2049 + 31) & ~31)
    nbytes = C.c_size_t(0)
    assert lib.bx_gsi_workspace_bytes(off.ctypes.data, len(lens), 0, C.byref(nbytes)) == OK
    n_slots = SLOT_BUDGET // slot_bytes
    assert n_slots == 63 and nbytes.value < 71 * slot_bytes
    assert n_slots * slot_bytes <= nbytes.value < (n_slots + 1) * slot_bytes

    got = gaussian_smooth(rows, tau)
    for k in range(len(lens)):
        alone = gaussian_smooth(rows[off[k]: off[k + 1]], tau)
        assert same_bits(got[off[k]: off[k + 1]], alone), f"tracklet {k} ({lens[k]} rows)"
    ref = {"smoothed": z["smoothed"][z["smoothed"][:, 1] == 2], "solver_spread": z["solver_spread"]}
    check_smoothed(got[:2049], ref, "deep's 2049 rows among 70 tracklets sharing 63 slots")


# ----------------------------------------------------------------------------- BX_GSI_MAX_N
def test_max_n_rows_are_admitted(lib):
    """A tracklet of BX_GSI_MAX_N = 4096 rows at tau = 20 (length scale 13.4: the factor's
    off-diagonal is ~1) is factored, stays finite and matches the CPU restatement within
    min(4 * spread, 1e-3), the spread measured here from the three CPU solvers."""
    import time

    from boxmot_amd import gaussian_smooth

    rows = tracklet(np.random.default_rng(4096), 5, MAX_N)
    ref = cpu_reference(rows, 20.0, 4097)
    t0 = time.perf_counter()
    got = gaussian_smooth(rows, 20.0)
    print(f"4096 rows: gaussian_smooth took {time.perf_counter() - t0:.3f} s")
    moved = float(np.abs(ref["smoothed"][:, 2:6] - rows[:, 2:6]).max())
    assert moved > 1.0  # the smoothing is not the identity here
    check_smoothed(got, ref, "4096 rows at tau = 20")


def test_more_than_max_n_rows_are_refused(lib):
    from boxmot_amd import gaussian_smooth

    rows = tracklet(np.random.default_rng(4097), 5, MAX_N + 1)
    nbytes = C.c_size_t(77)
    off = offsets([3, MAX_N + 1])
    assert lib.bx_gsi_workspace_bytes(off.ctypes.data, 2, 0, C.byref(nbytes)) == CAPACITY
    assert "4097 rows exceeds BX_GSI_MAX_N" in last_error(lib) and nbytes.value == 77
    both = np.concatenate([tracklet(np.random.default_rng(3), 4, 3), rows])
    rc, out, status = smooth_direct(lib, both, off, 10.0)
    assert rc == CAPACITY and "4097 rows exceeds BX_GSI_MAX_N" in last_error(lib)
    assert np.all(out == SENTINEL) and np.all(status == -7)  # nothing was launched
    with pytest.raises(ValueError, match="exceeds BX_GSI_MAX_N"):
        gaussian_smooth(rows, 10.0)


# ------------------------------------------------------------------------------ pivot latch
@pytest.mark.parametrize("lens,bad_row,force", [((20, 30, 25), 7, 0), ((50, 70, 45), 40, 1),
                                                ((30, 200, 180), 0, 0)],
                         ids=["lds", "blocked-second-panel", "both-paths-first-row"])
def test_nan_frame_latches_the_pivot(lib, lens, bad_row, force):
    """Three tracklets, the middle one with one NaN frame: its status is BX_ERR_INVALID and its
    rows carry columns 2..5 of the input; the other two carry the bits of a call without it.
    Python raises LinAlgError naming the id, and bx_gsi_run_host returns BX_ERR_INVALID."""
    from boxmot_amd.postprocessing import _gaussian_smooth

    rng = np.random.default_rng(sum(lens))
    tr = [tracklet(rng, ident, n, 100) for ident, n in zip((3, 11, 12), lens)]
    tr[1][bad_row, 0] = np.nan
    rows, off = np.concatenate(tr), offsets(lens)
    rc, out, status = smooth_direct(lib, rows, off, 10.0, force)
    assert rc == OK and status.tolist() == [OK, INVALID, OK]
    bad = out[off[1]: off[2]]
    assert same_bits(bad[:, [0, 1, 2, 3, 4, 5, 6, 7]], tr[1]) and np.all(bad[:, 8] == -1.0)

    rc, healthy, status = smooth_direct(lib, np.concatenate([tr[0], tr[2]]),
                                        offsets([lens[0], lens[2]]), 10.0, force)
    assert rc == OK and status.tolist() == [OK, OK] and np.isfinite(healthy).all()
    assert same_bits(out[: off[1]], healthy[: lens[0]])
    assert same_bits(out[off[2]:], healthy[lens[0]:])

    with pytest.raises(np.linalg.LinAlgError, match=rf"id 11 \({lens[1]} rows\)"):
        _gaussian_smooth(rows, 10.0, force_blocked=bool(force))

    host_out = np.full((rows.shape[0] + 64, 9), SENTINEL)
    n_out = C.c_int64(-1)
    rc = lib.bx_gsi_run_host(rows.ctypes.data, rows.shape[0], 8, 20, 10.0, host_out.ctypes.data,
                             host_out.shape[0], C.byref(n_out), None)
    assert rc == INVALID and "not positive definite" in last_error(lib)


# -------------------------------------------------------------------------- argument checks
def test_smooth_argument_checks(lib):
    rng = np.random.default_rng(8)
    lens = [5, 200]
    rows, off = np.concatenate([tracklet(rng, 1, 5), tracklet(rng, 2, 200)]), offsets(lens)
    untouched = lambda out, status: np.all(out == SENTINEL) and np.all(status == -7)  # noqa: E731

    for tau in (0.0, -1.0, float("nan")):
        rc, out, status = smooth_direct(lib, rows, off, tau)
        assert rc == INVALID and "tau must be positive" in last_error(lib), tau
        assert untouched(out, status)
    rc, out, status = smooth_direct(lib, rows, off, 10.0, ncol=7)
    assert rc == INVALID and "at least 8 columns" in last_error(lib) and untouched(out, status)

    down = np.array([0, 5, 3], np.int32)
    nbytes = C.c_size_t(77)
    assert lib.bx_gsi_workspace_bytes(down.ctypes.data, 2, 0, C.byref(nbytes)) == INVALID
    assert "must not decrease" in last_error(lib) and nbytes.value == 77
    rc, out, status = smooth_direct(lib, rows, down, 10.0)
    assert rc == INVALID and "must not decrease" in last_error(lib) and untouched(out, status)

    rc, out, status = smooth_direct(lib, rows, off, 10.0, short=1)
    assert rc == CAPACITY and "smoothing workspace too small" in last_error(lib)
    assert untouched(out, status)

    # no tracklets: nothing to do, no pointer is read
    assert lib.bx_gsi_smooth(None, 8, None, 0, 10.0, 0, None, 0, None, None, None) == OK
    assert lib.bx_gsi_workspace_bytes(None, 0, 0, C.byref(nbytes)) == OK and nbytes.value < 4096

    rc, out, status = smooth_direct(lib, rows, off, 10.0)  # and the same call, well-formed
    assert rc == OK and status.tolist() == [OK, OK] and np.isfinite(out).all()


def test_interpolation_argument_checks(lib):
    import torch

    z = np.load(GOLDEN / "gsi_gaps.npz")
    inp, ref, interval = np.ascontiguousarray(z["input"]), z["interpolated"], int(z["interval"])
    R, ncol = inp.shape
    st = torch.cuda.current_stream().cuda_stream
    d_rows = torch.from_numpy(inp).cuda()
    nbytes = C.c_size_t(0)
    assert lib.bx_gsi_plan_workspace_bytes(R, C.byref(nbytes)) == OK
    plan = torch.zeros(nbytes.value, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -5, dtype=torch.int64, device="cuda")

    rc = lib.bx_gsi_interpolate_plan(d_rows.data_ptr(), None, R, ncol, interval, plan.data_ptr(),
                                     nbytes.value - 1, counts.data_ptr(), st)
    assert rc == CAPACITY and "interpolation workspace too small" in last_error(lib)
    torch.cuda.synchronize()
    assert counts.tolist() == [-5, -5] and not plan.any().item()

    assert lib.bx_gsi_interpolate_plan(d_rows.data_ptr(), None, R, ncol, interval, plan.data_ptr(),
                                       nbytes.value, counts.data_ptr(), st) == OK
    n_out, n_tracks = counts.tolist()
    assert n_out == ref.shape[0] and n_tracks == np.unique(ref[:, 1]).size

    # cap below the output: the rows past it are not written (a cap inside a filled gap, one on
    # an input row, none at all, the whole output)
    key = lambda a: a[:, 1] * 1e6 + a[:, 0]  # noqa: E731
    filled = ~np.isin(key(ref), key(inp))
    inside = int(np.flatnonzero(filled[:-1] & filled[1:])[0]) + 1
    on_row = int(np.flatnonzero(~filled[:-1] & ~filled[1:])[3]) + 1
    for cap in (inside, on_row, 0, n_out):
        out = torch.full((n_out, ncol), SENTINEL, dtype=torch.float64, device="cuda")
        off = torch.full((n_tracks + 1,), -1, dtype=torch.int32, device="cuda")
        assert lib.bx_gsi_interpolate(d_rows.data_ptr(), R, ncol, plan.data_ptr(), out.data_ptr(),
                                      None, cap, off.data_ptr(), st) == OK
        got = out.cpu().numpy()
        assert same_bits(got[:cap], ref[:cap]) and np.all(got[cap:] == SENTINEL), cap
        starts = np.flatnonzero(np.r_[True, ref[1:, 1] != ref[:-1, 1]])
        assert off.cpu().tolist() == starts.tolist() + [n_out], cap

    rc = lib.bx_gsi_interpolate(d_rows.data_ptr(), R, ncol, plan.data_ptr(), out.data_ptr(), None,
                                -1, off.data_ptr(), st)
    assert rc == INVALID and "bad interpolation arguments" in last_error(lib)

    # no rows: both passes and the host path return OK with nothing to write
    counts.fill_(-5)
    assert lib.bx_gsi_interpolate_plan(None, None, 0, ncol, interval, plan.data_ptr(),
                                       nbytes.value, counts.data_ptr(), st) == OK
    assert counts.tolist() == [0, 0]
    assert lib.bx_gsi_interpolate(None, 0, ncol, plan.data_ptr(), None, None, 0, off.data_ptr(),
                                  st) == OK
    n = C.c_int64(-1)
    assert lib.bx_gsi_run_host(None, 0, 8, interval, 10.0, None, 0, C.byref(n), None) == OK
    assert n.value == 0
    rc = lib.bx_gsi_run_host(inp.ctypes.data, R, 7, interval, 10.0, None, 0, C.byref(n), None)
    assert rc == INVALID and "bad arguments" in last_error(lib)

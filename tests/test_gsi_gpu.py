"""GPU checks of the GSI post-processing against the reference's captures
(tests/golden/gsi_*.npz, written by tests/golden/make_golden_gsi.py).

Interpolation is plain float64 arithmetic in a written order: bitwise.  Smoothing solves K +
1e-10*I, conditioned at ~1e12, where correct float64 solvers disagree; each fixture carries the
reference's own spread against three restated solvers (``solver_spread``) and the smoothed
columns must match within 4x that spread (one more summation order; the device exp an ulp from
libm in K), capped at 1e-3 px.  The smoothing itself moves boxes by 4 to 7 px.

Fixtures beyond the default pair (interval 20, tau 10): ``tiles`` (lengths around the blocked
path's tile edges), ``deep`` (1201 and 2049 rows at tau = 15, where the factor's off-diagonal is
~1 — at tau = 10 a tracklet of more than 1000 rows factors the identity), ``params`` (three other
(interval, tau) pairs, both clips of the length scale), ``wide`` (10-column rows) and ``rows``
(interpolation only: row counts at the sort's padding and the scan's chunk, duplicate (id, frame)
rows).  The pivot latch, slot reuse, BX_GSI_MAX_N and the argument checks are in
test_gsi_paths_gpu.py.
"""
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
NAMES = ["tiny", "gaps", "mixed", "long", "unsorted"]
MORE = ["tiles", "deep", "wide"]  # same keys as NAMES
N_PARAMS, N_ROWS = 3, 6  # sub-cases of gsi_params.npz and gsi_rows.npz (keys suffixed _k)
FMT = "%d %d %d %d %d %d %d %d %d"
EXACT = [0, 1, 6, 7, 8]


@pytest.fixture(scope="module")
def fx():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return {n: dict(np.load(GOLDEN / f"gsi_{n}.npz")) for n in NAMES + MORE + ["params", "rows"]}


@pytest.fixture(scope="module")
def ours(fx):
    """This implementation's two steps on every fixture, computed once."""
    from boxmot_amd import gaussian_smooth, linear_interpolation

    out = {}
    for n in NAMES + MORE:
        z = fx[n]
        itp = linear_interpolation(z["input"], int(z["interval"]))
        out[n] = (itp, gaussian_smooth(itp, float(z["tau"])))
    return out


def tol(z):
    return min(4.0 * float(z["solver_spread"]), 1e-3)


def check_smoothed(got, z, what):
    ref = z["smoothed"]
    assert got.shape == ref.shape, what
    assert np.array_equal(got[:, EXACT], ref[:, EXACT]), f"{what}: frame/id/conf/cls/-1 or row order"
    err = float(np.abs(got[:, 2:6] - ref[:, 2:6]).max())
    print(f"{what}: max |smoothed - reference| = {err:.3g} (bound {tol(z):.3g})")
    assert np.isfinite(got).all() and err <= tol(z), (what, err, tol(z))


@pytest.mark.parametrize("name", NAMES + MORE)
def test_interpolation_is_bitwise(fx, ours, name):
    got, ref = ours[name][0], fx[name]["interpolated"]
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


@pytest.mark.parametrize("name", NAMES + MORE)
def test_smoothing_matches_the_reference(fx, ours, name):
    check_smoothed(ours[name][1], fx[name], name)


def test_tracks_of_one_and_two_rows(fx, ours):
    got, ref = ours["tiny"][1], fx["tiny"]["smoothed"]
    n_rows = {i: int((ref[:, 1] == i).sum()) for i in np.unique(ref[:, 1])}
    short = np.isin(ref[:, 1], [i for i, n in n_rows.items() if n <= 2])
    assert sorted(n_rows.values()) == [1, 2, 3] and short.sum() == 3
    err = float(np.abs(got[short] - ref[short]).max())
    print(f"tracks of 1 and 2 rows: max error {err:.3g}")
    assert err <= 1e-9


def test_batched_equals_single(fx, ours):
    from boxmot_amd.postprocessing import gsi_batch

    z0 = fx[NAMES[0]]
    batch = gsi_batch([fx[n]["input"] for n in NAMES], int(z0["interval"]), float(z0["tau"]))
    assert len(batch) == len(NAMES)
    for n, b in zip(NAMES, batch):
        single = ours[n][1]
        assert b.shape == single.shape, n
        assert np.array_equal(b.view(np.uint64), single.view(np.uint64)), n


def test_lds_and_blocked_paths_agree(fx, ours):
    from boxmot_amd.postprocessing import _gaussian_smooth

    z = fx["mixed"]
    lens = np.unique(z["interpolated"][:, 1], return_counts=True)[1]
    assert (lens <= 176).any() and (lens > 176).any()  # both paths run in the default launch
    forced = _gaussian_smooth(ours["mixed"][0], float(z["tau"]), force_blocked=True)
    check_smoothed(forced, z, "mixed, every tracklet on the blocked path")
    dflt = ours["mixed"][1]
    assert np.array_equal(forced[:, EXACT], dflt[:, EXACT])
    err = float(np.abs(forced[:, 2:6] - dflt[:, 2:6]).max())
    print(f"LDS vs blocked on mixed: {err:.3g}")
    assert err <= tol(z)
    tiny = _gaussian_smooth(ours["tiny"][0], float(fx["tiny"]["tau"]), force_blocked=True)
    check_smoothed(tiny, fx["tiny"], "tiny, blocked path")


def test_tile_edge_lengths_on_the_blocked_path(fx, ours):
    """`tiles` with every tracklet forced through the blocked factorisation: lengths 93..97 (the
    right-hand-side rows straddle a trailing tile's edge, or form a tile of their own), 128, 160,
    208, 224 +-1 (a trailing tile of exactly 64 rows, or one row more or less)."""
    from boxmot_amd.postprocessing import _gaussian_smooth

    z = fx["tiles"]
    lens = np.unique(z["interpolated"][:, 1], return_counts=True)[1]
    assert {93, 94, 95, 96, 97, 128, 160, 208, 224} <= set(lens.tolist())
    forced = _gaussian_smooth(ours["tiles"][0], float(z["tau"]), force_blocked=True)
    check_smoothed(forced, z, "tiles, every tracklet on the blocked path")


@pytest.mark.parametrize("k", range(N_PARAMS))
def test_other_intervals_and_taus(fx, k):
    """(interval, tau) = (2, 2): nothing fillable, the length scale of a 1-row tracklet clipped
    to tau^2; (5, 3): gaps of 3 filled and of 4 not, 30 rows clipped to 1/tau; (50, 10): a
    48-frame gap filled."""
    from boxmot_amd import gaussian_smooth, linear_interpolation

    p = fx["params"]
    z = {key: p[f"{key}_{k}"] for key in ("input", "interval", "tau", "interpolated", "smoothed",
                                           "solver_spread")}
    assert (int(z["interval"]), float(z["tau"])) == [(2, 2.0), (5, 3.0), (50, 10.0)][k]
    itp = linear_interpolation(z["input"], int(z["interval"]))
    assert itp.shape == z["interpolated"].shape
    assert np.array_equal(itp.view(np.uint64), z["interpolated"].view(np.uint64))
    check_smoothed(gaussian_smooth(itp, float(z["tau"])), z, f"params {k}")


def test_ten_column_rows(fx, ours):
    """MOT result rows are 10 wide: interpolation on all 10 columns (bitwise, parametrised above),
    smoothing reads them at stride 10, and a batch of a 10- and an 8-column array works on the
    shared 8 columns and returns the bits of the single calls."""
    from boxmot_amd.postprocessing import gsi_batch

    z, u = fx["wide"], fx["unsorted"]
    assert z["input"].shape[1] == 10 and ours["wide"][0].shape[1] == 10
    assert ours["wide"][1].shape == (z["interpolated"].shape[0], 9)
    assert (int(z["interval"]), float(z["tau"])) == (int(u["interval"]), float(u["tau"]))
    batch = gsi_batch([z["input"], u["input"]], int(z["interval"]), float(z["tau"]))
    for n, b in zip(["wide", "unsorted"], batch):
        assert b.shape == ours[n][1].shape, n
        assert np.array_equal(b.view(np.uint64), ours[n][1].view(np.uint64)), n


@pytest.mark.parametrize("k", range(N_ROWS))
def test_interpolation_row_counts_and_duplicates(fx, k):
    """1, 1023, 1024, 1025 and 2048 input rows (the bitonic network's padding; the scan's
    1024-row chunks and the carry between them, with filled gaps in every chunk), and duplicate
    (id, frame) rows with different boxes, whose order is np.lexsort's stable one."""
    from boxmot_amd import linear_interpolation

    r = fx["rows"]
    inp, ref = r[f"input_{k}"], r[f"interpolated_{k}"]
    if k < 5:
        assert inp.shape[0] == [1, 1023, 1024, 1025, 2048][k]
    got = linear_interpolation(inp, int(r[f"interval_{k}"]))
    assert got.shape == ref.shape and (k == 0 or ref.shape[0] > inp.shape[0])
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def test_gsi_on_a_folder(fx, tmp_path):
    from boxmot_amd import gaussian_smooth, gsi, linear_interpolation

    files = {"MOT17-02-FRCNN.txt": "gaps", "MOT17-04-FRCNN.txt": "unsorted"}
    for f, n in files.items():
        np.savetxt(tmp_path / f, fx[n]["input"], delimiter=",", fmt="%.6f")
    (tmp_path / "MOT17-05-FRCNN.txt").write_text("")
    (tmp_path / "seqmap.txt").write_text("name\n")
    loaded = {f: np.loadtxt(tmp_path / f, delimiter=",") for f in files}
    gsi(tmp_path)
    assert (tmp_path / "MOT17-05-FRCNN.txt").read_text() == ""
    assert (tmp_path / "seqmap.txt").read_text() == "name\n"
    for f, n in files.items():
        own = gaussian_smooth(linear_interpolation(loaded[f], 20), 10)
        want = tmp_path / "want.txt"
        np.savetxt(want, own, fmt=FMT)
        assert (tmp_path / f).read_text() == want.read_text(), f
        got = np.loadtxt(tmp_path / f)
        ref = fx[n]["smoothed"]
        assert got.shape == ref.shape
        assert np.array_equal(got[:, EXACT], ref[:, EXACT].astype(np.int64)), f


def test_run_sequences_with_gsi(fx, tmp_path):
    from boxmot_amd import gsi, motio
    from boxmot_amd.synth import SyntheticScene

    packed = {}
    for s in (1, 2):
        sc = SyntheticScene(n_obj=8 + 4 * s, seed=60 + s, p_det=0.8)
        fr = []
        for t in range(1, 41):
            d = sc.frame(t)[0]
            fr.append(np.concatenate([np.full((d.shape[0], 1), t), d], 1))
        dp = tmp_path / f"MOT-SYN-{s}.dets.txt"
        np.savetxt(dp, np.concatenate(fr), fmt="%f", header="synthetic")
        packed[f"MOT-SYN-{s}"] = motio.pack_sequence(dp, None, tmp_path / f"MOT-SYN-{s}.bxmot")
    a, b = tmp_path / "two_steps", tmp_path / "one_call"
    motio.run_sequences("bytetrack", packed, a)
    plain = {nm: (a / f"{nm}.txt").read_text() for nm in packed}
    gsi(a)
    motio.run_sequences("bytetrack", packed, b, gsi=True)
    for nm in packed:
        text = (b / f"{nm}.txt").read_text()
        assert text == (a / f"{nm}.txt").read_text() and text != plain[nm], nm
        assert "," in plain[nm] and "," not in text  # the reference writes GSI rows space-separated


def test_run_host_matches_the_two_steps(fx, ours):
    """bx_gsi_run_host (host memory in and out, one file's rows) returns the bits of the two
    Python steps, and reports an output that is too small."""
    import ctypes as C

    from boxmot_amd import _native as N

    L = N.load()
    z = fx["unsorted"]
    inp = np.ascontiguousarray(z["input"])
    want = ours["unsorted"][1]
    out = np.full((want.shape[0] + 3, 9), np.nan)
    n_out = C.c_int64(-1)
    N.check(L.bx_gsi_run_host(inp.ctypes.data, inp.shape[0], inp.shape[1], int(z["interval"]),
                              float(z["tau"]), out.ctypes.data, out.shape[0], C.byref(n_out), None),
            "bx_gsi_run_host")
    assert n_out.value == want.shape[0] and np.isnan(out[n_out.value:]).all()
    assert np.array_equal(out[: n_out.value].view(np.uint64), want.view(np.uint64))
    with pytest.raises(ValueError, match="fewer rows"):
        N.check(L.bx_gsi_run_host(inp.ctypes.data, inp.shape[0], inp.shape[1], 20, 10.0,
                                  out.ctypes.data, 5, C.byref(n_out), None), "bx_gsi_run_host")
    assert n_out.value == want.shape[0]

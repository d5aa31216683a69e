#!/usr/bin/env python
"""Generate the GSI fixtures tests/golden/gsi_<name>.npz from the Python reference
(boxmot/postprocessing/gsi.py: linear_interpolation, gaussian_smooth), on the CPU.

Same shim as make_golden.py (imported, not edited).  Inputs are seeded random walks (2 px jitter
per frame) with frames removed to open gaps; rows are ``frame, id, x, y, w, h, conf, cls``.  Each
file holds ``input``, ``interval``, ``tau``, the reference's ``interpolated`` and ``smoothed``
arrays and ``solver_spread``: the largest absolute difference of the predicted mean between
scikit-learn and three restatements of its solve on the same kernel matrix (np.linalg.solve, an
upper Cholesky, a Cholesky of a randomly permuted system) — the reference's own solver spread on
a system conditioned at ~1e12, which the GPU tests derive their tolerance from.  It never
involves the code under test.  A case is written only if it reaches the branch it is there for,
and only if 4x its spread stays below the tests' 1e-3 px cap.

``params`` and ``rows`` hold several inputs in one file, every key suffixed ``_k``; ``rows`` is
interpolation only (no ``tau``, ``smoothed`` or ``solver_spread``).  ``wide`` has 10-column rows.
``deep`` runs at tau = 15: at tau = 10 a tracklet of more than 1000 rows factors the identity,
at tau = 20 the reference's own spread breaks the cap.

Files are named ``gsi_*`` (not ``trk_*`` / ``deepoc_*``: other suites glob those).

Usage: ``python tests/golden/make_golden_gsi.py [name ...]`` (no argument = all).
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

from make_golden import install_shim  # noqa: E402

LDS_N, NB = 176, 32  # BX_GSI_LDS_N, BX_GSI_NB (include/bxgsi.h): the kernel's path boundary


def stub_missing():
    try:
        import tqdm  # noqa: F401
    except ImportError:
        m = types.ModuleType("tqdm")
        m.tqdm = lambda it, **k: it
        sys.modules["tqdm"] = m


def walk(rng, ident, frames):
    """One track: a random walk of the box (2 px jitter per frame) observed at `frames`."""
    frames = np.asarray(frames)
    span = int(frames[-1] - frames[0]) + 1
    steps = rng.normal(0.0, 2.0, (span, 4))
    path = np.array([rng.uniform(100, 1500), rng.uniform(100, 800), rng.uniform(40, 120),
                     rng.uniform(80, 260)]) + np.cumsum(steps, 0)
    box = path[frames - frames[0]]
    conf = rng.uniform(0.3, 1.0, (len(frames), 1))
    return np.concatenate([frames[:, None].astype(float), np.full((len(frames), 1), float(ident)),
                           box, conf, np.zeros((len(frames), 1))], 1)


def with_gaps(rng, start, n, interval, n_gaps):
    """Frames start..start+n-1 with n_gaps interior runs (shorter than interval - 1) removed, so
    the interpolation restores exactly n rows."""
    keep = np.ones(n, bool)
    for _ in range(n_gaps):
        if n < 8:
            break
        g = int(rng.integers(1, min(interval - 1, n // 3)))
        a = int(rng.integers(1, n - g - 1))
        if keep[a - 1: a + g + 1].all():
            keep[a: a + g] = False
    return start + np.flatnonzero(keep)


def case_tiny(rng, interval):
    return np.concatenate([walk(rng, 1, [5]), walk(rng, 2, [3, 4]), walk(rng, 3, [7, 8, 9])])


def case_gaps(rng, interval):
    rows = []
    for ident, gap in enumerate([1, interval - 2, interval - 1, interval], start=1):
        # frames 1..4, then `gap` missing frames, then 4 more
        f = np.r_[np.arange(1, 5), np.arange(5 + gap, 9 + gap)]
        rows.append(walk(rng, ident, f))
    f = np.r_[np.arange(2, 6), 7, np.arange(7 + interval, 7 + interval + 4)]  # both kinds
    rows.append(walk(rng, 9, f))
    return np.concatenate(rows)


MIXED = [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 20, 24, 31, 32, 33, 40, 47, 55, 63, 64, 65,
         80, 96, 100, 141, LDS_N - 1, LDS_N, LDS_N + 1, 192, 200, 225, 300, 400, 15, 18, 21, 27]


def case_mixed(rng, interval):
    rows = []
    for ident, n in enumerate(MIXED, start=1):
        rows.append(walk(rng, ident, with_gaps(rng, int(rng.integers(1, 50)), n, interval,
                                               n // 25)))
    return np.concatenate(rows)


def case_long(rng, interval):
    return np.concatenate([walk(rng, 1, with_gaps(rng, 1, 1200, interval, 12)),
                           walk(rng, 2, with_gaps(rng, 30, 700, interval, 8))])


def case_unsorted(rng, interval):
    rows = [walk(rng, ident, with_gaps(rng, int(rng.integers(1, 30)), n, interval, 3))
            for ident, n in [(1000, 37), (3, 90), (42, 12), (17, 61), (7, 1), (256, 45)]]
    rows = np.concatenate(rows)
    return rows[rng.permutation(rows.shape[0])]


TILES = [15, 16, 17, 34, 93, 94, 95, 96, 97, 127, 128, 129, 159, 160, 161, 207, 208, 209, 223, 224,
         225]


def case_tiles(rng, interval):
    """Lengths around the blocked path's tile edges: trailing tiles start at row 32 and step by 64
    and the right-hand sides sit in rows n..n+3, so 93..95 straddle a tile boundary with them and
    96 puts them in a tile of their own."""
    rows = []
    for ident, n in enumerate(TILES, start=1):
        rows.append(walk(rng, ident, with_gaps(rng, int(rng.integers(1, 50)), n, interval,
                                               max(1, n // 25))))
    return np.concatenate(rows)


DEEP = [1201, 2049]  # at tau = 15: at tau = 20 the reference's own 4 x spread is over the 1e-3 cap


def case_deep(rng, interval):
    return np.concatenate([walk(rng, 1, with_gaps(rng, 1, DEEP[0], interval, 12)),
                           walk(rng, 2, with_gaps(rng, 40, DEEP[1], interval, 20))])


def case_params(rng, interval):
    """Three (input, interval, tau) sub-cases off the default pair."""
    a = np.concatenate([walk(rng, 4, [9]), walk(rng, 6, [3, 5]),  # a gap of 1: not filled at 2
                        walk(rng, 11, np.r_[np.arange(1, 6), np.arange(7, 12)])])
    f = np.r_[np.arange(1, 9), np.arange(12, 20), np.arange(24, 35)]  # gaps of 3 and of 4
    b = np.concatenate([walk(rng, 2, f), walk(rng, 5, np.r_[1, 5, 6]), walk(rng, 8, np.r_[1, 6])])
    c = np.concatenate([walk(rng, 3, np.r_[np.arange(1, 6), np.arange(54, 60)]),  # 48 missing
                        walk(rng, 7, np.r_[np.arange(2, 5), np.arange(54, 57)]),  # 49, 50 missing:
                        walk(rng, 9, np.r_[np.arange(2, 5), np.arange(55, 58)])])  # not filled
    return [(a, 2, 2), (b, 5, 3), (c, 50, 10)]


def case_wide(rng, interval):
    """10-column MOT rows (frame, id, x, y, w, h, conf, -1, -1, -1), shuffled, sparse ids, both
    smoothing paths."""
    rows = [walk(rng, ident, with_gaps(rng, int(rng.integers(1, 30)), n, interval, 3))
            for ident, n in [(1000, 37), (3, 190), (42, 12), (17, 61), (7, 1), (256, 45)]]
    rows = np.concatenate(rows)
    rows = np.concatenate([rows[:, :7], np.full((rows.shape[0], 3), -1.0)], 1)
    return rows[rng.permutation(rows.shape[0])]


ROWS = [1, 1023, 1024, 1025, 2048]
CHUNK = 1024  # rows one pass of gsi_scan_kernel covers


def short_tracklets(rng, total, interval):
    """Exactly `total` shuffled rows of 6..10-row tracklets (sparse ids), each with one fillable
    gap, so gap rows come before and after every scan chunk."""
    rows, ident = [], 3
    while total:
        n = min(total, int(rng.integers(6, 11)))
        if total - n < 3:
            n = total
        f = int(rng.integers(1, 200)) + np.arange(n + 4)
        if n >= 2:  # the last tracklet's gap sits before its last row: the last chunk has one too
            a = int(rng.integers(1, n)) if total > n else n - 1
            f = np.r_[f[:a], f[a + int(rng.integers(1, 5)):]]
        rows.append(walk(rng, ident, f[:n]))
        ident += int(rng.integers(1, 4))
        total -= n
    rows = np.concatenate(rows)
    return rows[rng.permutation(rows.shape[0])]


def case_rows(rng, interval):
    """Interpolation only: row counts at the bitonic padding and the scan chunk, and duplicate
    (id, frame) rows with different boxes (one pair directly before a fillable gap)."""
    out = [short_tracklets(rng, r, interval) for r in ROWS]
    dup = [walk(rng, 5, [1, 2, 3, 6, 7]), walk(rng, 5, [3]), walk(rng, 5, [7]),
           walk(rng, 2, [4, 9]), walk(rng, 2, [4]), walk(rng, 2, [4]), walk(rng, 9, [1, 2, 5]),
           walk(rng, 9, [1, 2])]
    dup = np.concatenate(dup)
    out.append(dup[rng.permutation(dup.shape[0])])
    return out


CASES = [("tiny", case_tiny, 20, 10, 101), ("gaps", case_gaps, 20, 10, 102),
         ("mixed", case_mixed, 20, 10, 103), ("long", case_long, 20, 10, 104),
         ("unsorted", case_unsorted, 20, 10, 105), ("tiles", case_tiles, 20, 10, 106),
         ("deep", case_deep, 20, 15, 107), ("params", case_params, None, None, 108),
         ("wide", case_wide, 20, 10, 109), ("rows", case_rows, 20, None, 110)]


def length_scale(tau, n):
    return np.clip(tau * np.log(tau**3 / n), tau**-1, tau**2)


def solver_spread(interp, smoothed, tau, rng):
    """max |scikit-learn's mean - a restated solve's mean| over the tracks of one fixture."""
    from scipy.linalg import cho_factor, cho_solve
    from sklearn.gaussian_process.kernels import RBF

    worst = 0.0
    for ident in np.unique(interp[:, 1]):
        tr = interp[interp[:, 1] == ident]
        ref = smoothed[smoothed[:, 1] == ident][:, 2:6]
        n = len(tr)
        t = tr[:, 0].reshape(-1, 1)
        kern = RBF(length_scale(tau, n), length_scale_bounds="fixed")
        K = kern(t)
        Kt = kern(t, t)
        Kj = K.copy()
        Kj[np.diag_indices_from(Kj)] += 1e-10
        y = tr[:, 2:6]
        p = rng.permutation(n)
        inv = np.argsort(p)
        alphas = [np.linalg.solve(Kj, y), cho_solve(cho_factor(Kj, lower=False), y),
                  cho_solve(cho_factor(Kj[p][:, p], lower=True), y[p])[inv]]
        for a in alphas:
            worst = max(worst, float(np.abs(Kt @ a - ref).max()))
    return worst


def check_branch(name, inp, interp, interval, tau):
    lens = {int(i): int((interp[:, 1] == i).sum()) for i in np.unique(interp[:, 1])}
    if name == "tiny":
        assert sorted(lens.values()) == [1, 2, 3]
    elif name == "gaps":
        # ids 1, 2: gaps of 1 and interval - 2 rows are filled; ids 3, 4: interval - 1 and
        # interval are not
        assert lens[1] == 8 + 1 and lens[2] == 8 + interval - 2, lens
        assert lens[3] == 8 and lens[4] == 8, lens
        assert lens[9] == 9 + 1, lens
    elif name == "mixed":
        got = sorted(lens.values())
        assert got == sorted(MIXED), got
        assert LDS_N in got and LDS_N + 1 in got and any(n > LDS_N and n % NB for n in got)
        assert min(got) == 5 and max(got) == 400 and interp.shape[0] > inp.shape[0]
    elif name == "long":
        assert sorted(lens.values()) == [700, 1200]
        assert length_scale(tau, 1200) == 1 / tau and length_scale(tau, 700) > 1 / tau
        assert interp.shape[0] > inp.shape[0]
    elif name == "unsorted":
        order = np.lexsort((inp[:, 0], inp[:, 1]))
        assert not np.array_equal(order, np.arange(inp.shape[0]))
        ids = np.unique(inp[:, 1])
        assert not np.array_equal(ids, np.arange(ids[0], ids[0] + len(ids)))
        assert interp.shape[0] > inp.shape[0]


def gap_counts(inp, interval):
    """Rows the reference inserts before each row of `inp` in np.lexsort order."""
    s = inp[np.lexsort((inp[:, 0], inp[:, 1]))]
    f, i = s[:, 0].astype(np.int64), s[:, 1].astype(np.int64)
    d = f[1:] - f[:-1]
    return np.r_[0, np.where((i[1:] == i[:-1]) & (d > 1) & (d < interval), d - 1, 0)]


def factor_offdiag(frames, tau):
    """Largest off-diagonal entry of the Cholesky factor of K + 1e-10*I: ~0 when the clipped
    length scale makes K the identity, ~1 when the factorisation has work to do."""
    t = frames / length_scale(tau, len(frames))
    K = np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2)
    L = np.linalg.cholesky(K + 1e-10 * np.eye(len(t)))
    return float(np.abs(L - np.diag(np.diag(L))).max())


def check_new_branch(name, inp, interp, interval, tau, smoothed=None):
    lens = {int(i): int((interp[:, 1] == i).sum()) for i in np.unique(interp[:, 1])}
    n_in = {int(i): int((inp[:, 1] == i).sum()) for i in np.unique(inp[:, 1])}
    if name == "tiles":
        assert [lens[i] for i in sorted(lens)] == TILES, lens
        assert all(n_in[i] < lens[i] for i in lens), (n_in, lens)  # every tracklet has a gap
        assert {93, 94, 95, 96, 97, 128, 160, 208, 224} <= set(TILES)
    elif name == "deep":
        assert [lens[i] for i in sorted(lens)] == DEEP and all(n_in[i] < lens[i] for i in lens)
        assert all(n > 1000 and n % NB and (n - NB) % 64 for n in DEEP)
        for i in lens:
            tr = interp[interp[:, 1] == i]
            off = factor_offdiag(tr[:, 0], tau)
            moved = float(np.abs(smoothed[smoothed[:, 1] == i][:, 2:6] - tr[:, 2:6]).max())
            print(f"deep: {lens[i]} rows: length scale {length_scale(tau, lens[i]):.3g}, largest "
                  f"off-diagonal of the factor {off:.3g}, boxes move {moved:.3g} px")
            assert off > 0.5 and moved > 1.0, (i, off, moved)
        # the recorded contrast: the 1200-row tracklet of `long` (tau = 10) factors the identity
        z = np.load(HERE / "gsi_long.npz")
        tr = z["interpolated"][z["interpolated"][:, 1] == 1]
        off = factor_offdiag(tr[:, 0], float(z["tau"]))
        print(f"deep: contrast, long's {len(tr)} rows at tau={float(z['tau']):g}: {off:.3g}")
        assert len(tr) == 1200 and off < 1e-12, off
    elif name == "params0":
        assert (interval, tau) == (2, 2) and interp.shape[0] == inp.shape[0]  # nothing fillable
        assert sorted(lens.values()) == [1, 2, 10] and (gap_counts(inp, 3) > 0).any()
        assert length_scale(tau, 1) == tau**2
    elif name == "params1":
        assert (interval, tau) == (5, 3)
        d = np.diff(interp[interp[:, 1] == 2][:, 0])
        assert lens[2] == 30 and n_in[2] == 27 and sorted(set(d)) == [1, 5], (lens, d)
        assert lens[5] == 3 + 3 and lens[8] == 2, lens  # 1 -> 5: filled, 1 -> 6: not
        assert length_scale(tau, lens[2]) == 1 / tau
    elif name == "params2":
        assert (interval, tau) == (50, 10)
        assert lens[3] == 11 + 48 and lens[7] == 6 and lens[9] == 6, lens
    elif name == "wide":
        assert inp.shape[1] == 10 and np.all(inp[:, 7:] == -1) and np.all(interp[:, 7:] == -1)
        order = np.lexsort((inp[:, 0], inp[:, 1]))
        assert not np.array_equal(order, np.arange(inp.shape[0]))
        ids = np.unique(inp[:, 1])
        assert not np.array_equal(ids, np.arange(ids[0], ids[0] + len(ids)))
        assert interp.shape[0] > inp.shape[0]
        assert min(lens.values()) == 1 and max(lens.values()) > LDS_N
    elif name.startswith("rows"):
        k = int(name[4:])
        cnt = gap_counts(inp, interval)
        assert interp.shape[0] == inp.shape[0] + cnt.sum()
        if k < len(ROWS):
            assert inp.shape[0] == ROWS[k]
            for base in range(0, inp.shape[0] if inp.shape[0] > 1 else 0, CHUNK):
                assert cnt[base: base + CHUNK].sum() > 0, (name, base)
            if inp.shape[0] > CHUNK:  # filled rows on both sides of the first chunk's end
                assert cnt[CHUNK - 32: CHUNK].sum() > 0 and cnt[CHUNK: CHUNK + 32].sum() > 0
        else:
            s = inp[np.lexsort((inp[:, 0], inp[:, 1]))]
            same = (s[1:, :2] == s[:-1, :2]).all(1)
            assert same.sum() >= 5 and not (s[1:, 2:6][same] == s[:-1, 2:6][same]).any()
            assert (same[:-1] & (cnt[2:] > 0)).any()  # a duplicate pair directly before a filled gap
            assert not np.array_equal(np.lexsort((inp[:, 0], inp[:, 1])), np.arange(inp.shape[0]))


def reference(inp, interval, tau, seed, name):
    """The reference's two steps on one input, and its solver spread (tau None: step one only)."""
    from boxmot.postprocessing.gsi import gaussian_smooth, linear_interpolation

    interp = linear_interpolation(inp.copy(), interval)
    if tau is None:
        return interp, None, None
    smoothed = gaussian_smooth(interp.copy(), tau)
    assert np.isfinite(smoothed).all() and smoothed.shape == (interp.shape[0], 9)
    spread = solver_spread(interp, smoothed, tau, np.random.default_rng(seed + 1000))
    print(f"{name}: rows={inp.shape[0]} interpolated={interp.shape[0]} solver_spread={spread:.3g}")
    assert 4 * spread < 1e-3, f"{name}: the reference's own spread breaks the 1e-3 cap"
    return interp, smoothed, spread


def main():
    only = set(sys.argv[1:])
    install_shim()
    stub_missing()

    for name, make, interval, tau, seed in CASES:
        if only and name not in only:
            continue
        rng = np.random.default_rng(seed)
        inp = make(rng, interval)
        if name in ("params", "rows"):  # several inputs in one file, keys suffixed _k
            subs = inp if name == "params" else [(a, interval, None) for a in inp]
            keys = {}
            for k, (a, iv, ta) in enumerate(subs):
                interp, smoothed, spread = reference(a, iv, ta, seed + 10 * k, f"{name}{k}")
                check_new_branch(f"{name}{k}", a, interp, iv, ta, smoothed)
                keys.update({f"input_{k}": a, f"interval_{k}": iv, f"interpolated_{k}": interp})
                if ta is not None:
                    keys.update({f"tau_{k}": ta, f"smoothed_{k}": smoothed,
                                 f"solver_spread_{k}": spread})
                else:
                    print(f"{name}{k}: rows={a.shape[0]} interpolated={interp.shape[0]}")
            np.savez_compressed(HERE / f"gsi_{name}.npz", **keys)
            continue
        interp, smoothed, spread = reference(inp, interval, tau, seed, name)
        check_branch(name, inp, interp, interval, tau)
        check_new_branch(name, inp, interp, interval, tau, smoothed)
        np.savez_compressed(HERE / f"gsi_{name}.npz", input=inp, interval=interval, tau=tau,
                            interpolated=interp, smoothed=smoothed, solver_spread=spread)


if __name__ == "__main__":
    main()

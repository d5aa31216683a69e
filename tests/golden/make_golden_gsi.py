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
involves the code under test.  A case is written only if it reaches the branch it is there for.

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


CASES = [("tiny", case_tiny, 20, 10, 101), ("gaps", case_gaps, 20, 10, 102),
         ("mixed", case_mixed, 20, 10, 103), ("long", case_long, 20, 10, 104),
         ("unsorted", case_unsorted, 20, 10, 105)]


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


def main():
    only = set(sys.argv[1:])
    install_shim()
    stub_missing()
    from boxmot.postprocessing.gsi import gaussian_smooth, linear_interpolation

    for name, make, interval, tau, seed in CASES:
        if only and name not in only:
            continue
        rng = np.random.default_rng(seed)
        inp = make(rng, interval)
        interp = linear_interpolation(inp.copy(), interval)
        smoothed = gaussian_smooth(interp.copy(), tau)
        check_branch(name, inp, interp, interval, tau)
        assert np.isfinite(smoothed).all() and smoothed.shape == (interp.shape[0], 9)
        spread = solver_spread(interp, smoothed, tau, np.random.default_rng(seed + 1000))
        print(f"{name}: rows={inp.shape[0]} interpolated={interp.shape[0]} "
              f"solver_spread={spread:.3g}")
        np.savez_compressed(HERE / f"gsi_{name}.npz", input=inp, interval=interval, tau=tau,
                            interpolated=interp, smoothed=smoothed, solver_spread=spread)


if __name__ == "__main__":
    main()

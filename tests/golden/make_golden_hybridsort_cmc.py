#!/usr/bin/env python
"""Generate the HybridSort camera-motion fixtures tests/golden/hybcmc_<name>.npz from the
Python reference with ``tracker.ECC = True`` (hybridsort.py:417, 448-451;
KalmanBoxTracker.camera_update :237-249), on the CPU.

The shim, the patches H1-H3, the counters, the snapshot and the frame loop are
make_golden_hybridsort.py's, imported, not edited.  The reference's ``ECC = True`` path needed no further run-time patch:
``camera_update`` runs as published on every state these scenes reach (no state score is exactly
0, where ``convert_bbox_to_z`` would return four rows and the assignment into ``x[:5]`` raise).

The module's ``get_cmc_method`` is replaced, so OpenCV is never touched: ``tracker.cmc.apply``
returns the seeded similarity warp ``boxmot_amd.synth.synth_warp(seed, t)`` of the frame (the one
``make_golden.py warp`` uses for the other trackers) as a float32 2x3, the type the reference's
estimator returns, or the float32 identity.  The warps are stored in the fixture (``warps
[n_frames, 2, 3]`` float64 holding the float32 values, frame t at row t-1).

    hybcmc_crowd40    crowd40_dense's scene and arguments under shake warps
    hybcmc_noisy40    noisy40_motion's, so that motion decides the association
    hybcmc_identity   grid24_f20's with ECC = True and identity warps: the state -> corner
                          box -> state round trip alone

No per-class fixture is written: on perclass_hybrid_crowd24's scene warps of 6 and of 40 px
changed no output row (appearance decides, the OCR round recovers the rest, and the per-class
fixtures keep no state), and with emb_noise 3 and GIoU a LAP call ties.

A case is written only if the reference's outputs under its warps differ from its outputs with
``ECC = False`` (for noisy40: the ids too) - except crowd40, see STATE_ONLY below - and, for
every case, the identity one included, only if the captured ``kf.x`` differs from the ``ECC =
False`` run's in at least one bit.  The plain fixtures keep the four state
snapshots of make_golden_hybridsort.py, and ``cam_before`` / ``cam_after``: kf.x of every track
right before and right after the reference's ``camera_update`` of the last frame (under
``warps[-1]``), the phase alone, which tests/test_hybridsort_cmc_host.py holds the numpy
restatement to bit for bit.

The bits of ``warp @ [x, y, 1]`` are BLAS's: these files were written with numpy 2.2.6 over
OpenBLAS 0.3.29 (Haswell kernels), whose row sum is fma(m0, x, m1 * y) + m2; the device phase
spells that order out.  ``check_blas_order`` asserts it on random rows before
anything is written, so a regeneration over another BLAS fails loudly instead of changing bits.

Usage: ``python tests/golden/make_golden_hybridsort_cmc.py [name ...]`` (no argument = all).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

import make_golden_hybridsort as mgh  # noqa: E402
from make_golden import install_shim, synth_frames, use_restated_lapx_jv  # noqa: E402

from boxmot_amd.synth import SyntheticScene, synth_warp  # noqa: E402
from tests.hybcmc_util import fma  # noqa: E402

BASE = {name: (skw, tkw, nf) for name, skw, tkw, nf, _ in mgh.CASES}
# name, the make_golden_hybridsort.py case it follows, the warps' shift in px (None: identity)
CASES = [
    ("crowd40", "crowd40_dense", 6.0),
    ("noisy40", "noisy40_motion", 6.0),
    ("identity", "grid24_f20", None),
]
# crowd40_dense is decided by its appearance term and its output boxes are observations: shifts
# of 6, 12 and 24 px all left every output row as it is without warps.  Its fixture is written on
# the state alone (kf.x at the four snapshots differs) and says so in ``outputs_differ``.
STATE_ONLY = ("crowd40",)


def frame_warps(seed: int, nf: int, shift) -> np.ndarray:
    """[nf, 2, 3] float32: frame t's warp at row t-1."""
    if shift is None:
        return np.tile(np.eye(2, 3, dtype=np.float32), (nf, 1, 1))
    return np.stack([synth_warp(seed, t, shift=shift) for t in range(1, nf + 1)]).astype(np.float32)


class FrameCMC:
    """``tracker.cmc``: the warp of the frame the caller set in ``t``, as float32."""

    def __init__(self, warps):
        self.warps, self.t, self.calls = warps, 0, 0

    def apply(self, img, dets=None):
        self.calls += 1
        return self.warps[self.t - 1].copy()


def with_frame(frames, cmc):
    for fno, dets, embs in frames:
        cmc.t = fno
        yield fno, dets, embs


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_blas_order(n=200):
    """numpy's ``warp @ [x, y, 1]`` here is fma(m0, x, m1 * y) + m2, the order the device phase
    and tests/hybcmc_util.py spell out."""
    rng = np.random.default_rng(0)
    for k in range(n):
        m = synth_warp(1, k, shift=30.0).astype(np.float32)
        x, y = rng.uniform(-50, 2000, 2)
        got = m @ np.array([x, y, 1]).T
        md = m.astype(np.float64)
        for r in range(2):
            want = fma(md[r, 0], x, md[r, 1] * y) + md[r, 2]
            assert got[r] == want, "this BLAS sums the 2x3 product in another order: the " \
                                   "fixtures' bits would change (DESIGN.md 2.28)"


def capture_phase(mod, last):
    """Wrap KalmanBoxTracker.camera_update: kf.x before and after every call of frame `last`."""
    KBT = mod.KalmanBoxTracker
    ref, rec = KBT.camera_update, {"t": 0, "before": [], "after": []}

    def camera_update(self, warp):
        b = self.kf.x[:, 0].copy()
        ref(self, warp)
        if rec["t"] == last:
            rec["before"].append(b)
            rec["after"].append(self.kf.x[:, 0].copy())

    KBT.camera_update = camera_update
    return rec, lambda: setattr(KBT, "camera_update", ref)


def plain_case(mod, count, name, base, shift):
    skw, tkw, nf = BASE[base]
    scene = SyntheticScene(**skw)
    snap_at = [nf // 4, nf // 2, 3 * nf // 4, nf]
    warps = frame_warps(skw["seed"], nf, shift)

    def capture(ecc):
        for k in count:
            count[k] = 0
        tracker = mod.HybridSort(reid_weights=None, device="cpu", half=False, **tkw)
        tracker.ECC = ecc
        tracker.cmc = FrameCMC(warps)
        rec, undo = capture_phase(mod, nf)

        def frames():
            for f in with_frame(synth_frames(scene, nf), tracker.cmc):
                rec["t"] = f[0]
                yield f

        try:
            o, st, snaps = mgh.run(tracker, frames(), count, snap_at)
        finally:
            undo()
        assert tracker.cmc.calls == (nf if ecc else 0)
        state = {f"state_{k}": np.concatenate([snaps[f][k] for f in snap_at], 0)
                 for k in snaps[nf]}
        state["state_frames"] = np.array(snap_at, np.int32)
        state["state_off"] = np.concatenate(
            [[0], np.cumsum([snaps[f]["id"].shape[0] for f in snap_at])]).astype(np.int32)
        if ecc:
            state["cam_before"] = np.array(rec["before"], np.float64).reshape(-1, 9)
            state["cam_after"] = np.array(rec["after"], np.float64).reshape(-1, 9)
            assert state["cam_before"].shape[0] >= 20
        return o, st, state

    off, _, off_state = capture(False)
    outs, stats, state = capture(True)
    x_differs = not same_bits(state["state_x"], off_state["state_x"])
    out_differs = not same_bits(outs, off)
    ids_differ = outs.shape != off.shape or not np.array_equal(outs[:, 5], off[:, 5])
    print(f"hybcmc_{name}: rows={outs.shape[0]} (ECC off: {off.shape[0]}) lap={stats} "
          f"outputs differ: {out_differs} ids differ: {ids_differ} kf.x differs: {x_differs}")
    assert stats["degenerate"] == 0, f"{name}: a LAP call ties: change the warps"
    assert x_differs, f"{name}: kf.x is the ECC = False run's bit for bit"
    if shift is not None and name not in STATE_ONLY:
        assert out_differs, f"{name}: the warps change no output"
    if name == "noisy40":
        assert ids_differ, f"{name}: the warps change no id"
    path = HERE / f"hybcmc_{name}.npz"
    if path.exists():  # a regeneration adds to a fixture and replaces nothing
        with np.load(path) as old:
            for k, v in dict(state, outputs=outs).items():
                assert k not in old.files or same_bits(old[k], v) or \
                    np.array_equal(old[k], v), f"{name}: {k} changed"
    np.savez_compressed(
        path, outputs=outs, n_frames=nf, kind="hybridsort",
        scene=repr(skw), tracker_args=repr(tkw), base=base, warps=warps.astype(np.float64),
        lap_calls=stats["calls"], lap_degenerate=stats["degenerate"],
        rows_without_ecc=off.shape[0], outputs_differ=out_differs, ids_differ=ids_differ,
        **count, **state)


def main():
    only = set(sys.argv[1:])
    install_shim()
    use_restated_lapx_jv()
    import boxmot.motion.cmc  # noqa: F401  (so that the replacement below is not overwritten)

    mgh.install_h1()
    count = dict.fromkeys(mgh.COUNTERS, 0)
    import boxmot.trackers.hybridsort.hybridsort as mod

    mod.get_cmc_method = lambda name: (lambda: None)  # (every run assigns tracker.cmc)
    mgh.instrument(count)
    check_blas_order()
    for name, base, shift in CASES:
        if not only or name in only or f"hybcmc_{name}" in only:
            plain_case(mod, count, name, base, shift)


if __name__ == "__main__":
    main()

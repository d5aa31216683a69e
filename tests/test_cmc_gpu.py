"""ECC camera-motion compensation on the device against the numpy restatement
(tests/ecc_ref.py): preprocessing bit for bit, the solve within the tolerance DESIGN.md 2.14
records, batches, capacity and errors, and the warp's way into a tracker."""

import numpy as np
import pytest

from tests import ecc_ref as R

pytestmark = pytest.mark.gpu

# Ten times the largest device-minus-restatement difference measured over every case below
# (7.8e-15 in a warp entry, 6.9e-15 in rho); the contract's caps are 1e-4 / 1e-6.
TOL_WARP = 7.8e-14
TOL_RHO = 6.9e-14
assert TOL_WARP <= 1e-4 and TOL_RHO <= 1e-6

EYE = np.eye(2, 3)


@pytest.fixture(scope="module")
def cmc():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from boxmot_amd import cmc as m

    return m


def device_case(cmc, name):
    h, w, seed, mode, A, init, max_iter = R.CASES[name]
    a, b = R.case_frames(name)
    e = cmc.ECC(warp_mode=mode, max_iter=max_iter, scale=None)
    first = e.apply(a)
    assert first.dtype == np.float32 and np.array_equal(first, EYE) and e.last["code"] == 1
    out = e.apply(b, init_warp=init)
    assert out.dtype == np.float32 and out.shape == (2, 3)
    assert np.array_equal(out, e.last["warp"].astype(np.float32))
    return e.last


def compare(got, ref, what):
    M, rho, it, code = ref
    dw = np.abs(got["warp"] - M).max()
    dr = 0.0 if np.isnan(rho) and np.isnan(got["rho"]) else abs(got["rho"] - rho)
    print(f"{what}: code {got['code']}/{code} iterations {got['iterations']}/{it} "
          f"max |d warp| {dw:.3e} |d rho| {dr:.3e}")
    assert got["code"] == code and got["iterations"] == it
    assert dw <= TOL_WARP
    assert dr <= TOL_RHO


# ------------------------------------------------------------------------------ preprocessing
@pytest.mark.parametrize("scale", [0.15, 0.5, None])
def test_prep_is_bit_equal(cmc, scale):
    img = np.random.default_rng(7).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    e = cmc.ECC(scale=scale)
    e.apply(img)
    has, g, gx, gy = e._handle.state(0)
    rg, rgx, rgy = R.prep(img, scale)
    assert has and g.shape == R.work_size(37, 53, scale)
    assert np.array_equal(g, rg) and np.array_equal(e.prev_img, rg)
    assert np.array_equal(gx, rgx) and np.array_equal(gy, rgy)
    grey = R.grey(img).astype(np.uint8)  # a grey frame skips the conversion only
    e2 = cmc.ECC(scale=scale)
    e2.apply(grey)
    assert np.array_equal(e2.prev_img, rg)


# -------------------------------------------------------------------------------------- solve
@pytest.mark.parametrize("name", list(R.CASES))
def test_solve_matches_restatement(cmc, name):
    compare(device_case(cmc, name), R.solve_case(name), name)


def test_constant_image(cmc):
    a = R.texture(48, 64, 1)
    c = np.full((48, 64), 77, np.uint8)
    e = cmc.ECC(scale=None)
    e.apply(a)
    assert np.array_equal(e.apply(c), EYE)
    assert e.last["code"] == 2 and e.last["iterations"] == 1 and np.isnan(e.last["rho"])
    assert np.array_equal(e.prev_img, c)


def test_scaled_translation(cmc):
    a = R.texture(96, 128, 1)
    b = R.texture(96, 128, 1, R.shift_warp(2.6, -1.4))
    ref = R.EccRef(scale=0.5)
    ref.apply(a)
    e = cmc.ECC(scale=0.5)
    e.apply(a)
    e.apply(b)
    compare(e.last, ref.apply(b), "scale 0.5")
    # BGR input through the whole path
    bgr = lambda g: np.stack([g, g, g], -1)  # noqa: E731
    ref = R.EccRef(scale=0.5)
    ref.apply(bgr(a))
    e = cmc.ECC(scale=0.5)
    e.apply(bgr(a))
    e.apply(bgr(b))
    compare(e.last, ref.apply(bgr(b)), "scale 0.5 bgr")


# -------------------------------------------------------------------------------------- batch
SHIFTS2 = [(1.3, -0.7), (-0.4, 0.15), (0.6, 1.1), (6.0, -4.0), (0.2, 0.2)]  # stream 3: too far
SHIFTS3 = [(0.5, 0.3), (0.8, -0.2), (-0.3, 0.4), (0.4, 0.1), (-0.6, 0.5)]


def batch_frames():
    f1 = np.stack([R.texture(48, 64, s + 1) for s in range(5)])
    f2 = np.stack([R.texture(48, 64, s + 1, R.shift_warp(*SHIFTS2[s])) for s in range(5)])
    f3 = np.stack([R.texture(48, 64, s + 1, R.shift_warp(*SHIFTS3[s])) for s in range(5)])
    return f1, f2, f3


def run_batch(cmc):
    f1, f2, f3 = batch_frames()
    b = cmc.EccBatch(5, scale=None)
    outs = [b.apply(f1)]
    order = [3, 0, 2, 1]  # stream 4 gets no frame at the second step
    outs.append(b.apply(f2[order], streams=order))
    outs.append(b.apply(f3))
    res = [[t.cpu().numpy() for t in o] for o in outs]
    assert b.status() == 0
    return res


def test_batch_equals_single_streams(cmc):
    import torch

    res = run_batch(cmc)
    f1, f2, f3 = batch_frames()
    for s in range(5):
        e = cmc.ECC(scale=None)
        steps = [f1[s], f2[s], f3[s]] if s != 4 else [f1[s], None, f3[s]]
        for k, fr in enumerate(steps):
            w, rho, it, code = (a[s] for a in res[k])
            if fr is None:  # not listed: identity, NO_FRAME
                assert code == cmc.NO_FRAME and np.array_equal(w.reshape(2, 3), EYE)
                continue
            e.apply(fr)
            assert np.array_equal(w.reshape(2, 3), e.last["warp"])
            assert (rho == e.last["rho"] or (np.isnan(rho) and np.isnan(e.last["rho"])))
            assert it == e.last["iterations"] and code == e.last["code"]
    codes = np.stack([r[3] for r in res])
    assert codes[0].tolist() == [1] * 5
    assert codes[1].tolist() == [0, 0, 0, 2, 3]
    # stream 4 kept its first image over the step it sat out: its third step aligns frame 3 to
    # frame 1, like the restatement; stream 3 goes on from the frame that did not converge
    ref = R.EccRef(scale=None)
    ref.apply(f1[4])
    M, rho, it, code = ref.apply(f3[4])
    assert code == R.OK and res[2][3][4] == 0 and res[2][2][4] == it
    assert np.abs(res[2][0][4].reshape(2, 3) - M).max() <= TOL_WARP
    assert np.abs(M[:, 2] - SHIFTS3[4]).max() < 0.02
    # a CUDA tensor in gives the same bits
    b = cmc.EccBatch(5, scale=None)
    b.apply(torch.from_numpy(f1).cuda())
    w = b.apply(torch.from_numpy(f3).cuda())[0].cpu().numpy()
    b2 = cmc.EccBatch(5, scale=None)
    b2.apply(f1)
    assert np.array_equal(w, b2.apply(f3)[0].cpu().numpy())
    assert w.dtype == np.float64 and w.shape == (5, 6)


def test_device_path_does_not_synchronise(cmc):
    """With device inputs EccBatch.apply only enqueues: torch's sync debug mode turns every
    synchronising torch call (a copy from host values among them) into an error."""
    import torch

    f1, f2, f3 = (torch.from_numpy(f).cuda() for f in batch_frames())
    order = torch.tensor([3, 0, 2, 1], device="cuda", dtype=torch.int32)
    f2o = f2[order.long()].contiguous()
    iw = torch.zeros(5, 6, dtype=torch.float64, device="cuda")
    iw[:, 0] = 1.0
    iw[:, 4] = 1.0
    b = cmc.EccBatch(5, scale=None)
    b.apply(f1)  # builds the handle and the cached tensors (allocations may synchronise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # the probe sees a host-to-device copy
            torch.tensor([1.0, 0.0], dtype=torch.float64, device="cuda")
        out2 = b.apply(f2o, streams=order)
        out3 = b.apply(f3, init_warps=iw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = run_batch(cmc)
    for got, want in ((out2, ref[1]), (out3, ref[2])):
        for x, y in zip(got, want):
            assert np.array_equal(x.cpu().numpy(), y, equal_nan=True)


def test_batch_runs_are_bit_identical(cmc):
    r1, r2 = run_batch(cmc), run_batch(cmc)
    for a, b in zip(r1, r2):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)


# ------------------------------------------------------------------------ capacity and errors
def test_capacity_leaves_state_unchanged(cmc):
    a, b = R.case_frames("shift_a")
    batch = cmc.EccBatch(2, scale=None, max_h=48, max_w=64)
    batch.apply(a[None], streams=[0])
    with pytest.raises(ValueError, match="capacity exceeded"):
        batch.apply(np.zeros((1, 50, 64), np.uint8), streams=[0])
    with pytest.raises(ValueError, match="capacity exceeded"):
        batch.apply(np.zeros((1, 48, 65), np.uint8), streams=[0])
    with pytest.raises(ValueError, match="capacity exceeded"):
        batch.apply(np.zeros((3, 48, 64), np.uint8))
    has, g, _, _ = batch.state(0)
    assert has and np.array_equal(g, a) and not batch.state(1)[0]
    w, rho, it, code = (t.cpu().numpy() for t in batch.apply(b[None], streams=[0]))
    M, rrho, rit, rcode = R.solve_case("shift_a")
    assert code[0] == rcode == 0 and it[0] == rit and np.abs(w[0].reshape(2, 3) - M).max() <= TOL_WARP
    assert code[1] == cmc.NO_FRAME
    # a smaller image fits; the stream's size changed, so it starts over (and says so)
    w, rho, it, code = batch.apply(np.zeros((1, 20, 30), np.uint8), streams=[0])
    assert code.cpu().numpy()[0] == 1 and batch.status() == 6
    batch.reset()
    assert not batch.state(0)[0]


def test_bad_stream_index(cmc):
    import torch

    from boxmot_amd import _native as N

    a = R.texture(48, 64, 1)
    batch = cmc.EccBatch(2, scale=None)
    with pytest.raises(ValueError, match="invalid argument"):
        batch.apply(a[None], streams=[2])
    with pytest.raises(ValueError, match="invalid argument"):
        batch.apply(np.stack([a, a]), streams=[1, 1])
    # the C entry's own check (BX_ERR_INVALID = 1), nothing launched
    with pytest.raises(ValueError, match="invalid argument"):  # BX_ECC_MAX_STREAMS
        cmc._Handle(65536, 1, 1)
    h = cmc._Handle(2, 48, 64)
    streams = np.array([5], np.int32)
    out = [np.zeros(12), np.zeros(2), np.zeros(2, np.int32), np.zeros(2, np.int32)]
    rc = h._L.bx_ecc_apply_host(h._h, 1, 48, 64, 1, a.ctypes.data, streams.ctypes.data, 0, 1e-5,
                                100, 0.0, None, *[o.ctypes.data for o in out], None)
    assert rc == 1 and b"stream index" in h._L.bx_last_error()
    assert not h.state(0, planes=False)[0] and h.status() == 0
    rc = h._L.bx_ecc_apply_host(h._h, 1, 48, 64, 1, a.ctypes.data, streams.ctypes.data, 3, 1e-5,
                                100, 0.0, None, *[o.ctypes.data for o in out], None)
    assert rc == 1 and b"HOMOGRAPHY" in h._L.bx_last_error()
    with pytest.raises(ValueError):
        N.check(rc, "bx_ecc_apply_host")
    h.close()
    # device-resident indices cannot be checked on the host: the frame is skipped, the status
    # latched, the other stream served
    w, rho, it, code = batch.apply(np.stack([a, a]), streams=torch.tensor([0, 9], device="cuda"))
    assert code.cpu().numpy().tolist() == [1, cmc.NO_FRAME] and batch.status() == 1


# ----------------------------------------------------------------------------- into a tracker
class StubCMC:
    def __init__(self, warps):
        self.warps, self.k = warps, 0

    def apply(self, img, dets=None):
        self.k += 1
        return self.warps[self.k - 1]


def pan_scene(n_frames=12):
    """A texture panned by a known sub-pixel amount per frame, boxes panning with it."""
    rng = np.random.default_rng(3)
    boxes = np.array([[6, 5, 16, 19], [24, 8, 33, 22], [42, 4, 52, 18], [10, 26, 21, 41],
                      [34, 27, 44, 43], [50, 24, 60, 40]], np.float64)
    frames, dets = [], []
    for t in range(n_frames):
        c = np.array([1.5 * np.sin(0.9 * t) + 0.35 * t, 1.0 * np.cos(0.7 * t) - 0.2 * t])
        frames.append(np.stack([R.texture(48, 64, 9, R.shift_warp(*c))] * 3, -1))
        d = np.zeros((len(boxes), 6))
        d[:, :4] = boxes + np.tile(c, 2) + rng.normal(0, 0.05, boxes.shape)
        d[:, 4] = 0.9
        dets.append(d)
    return frames, dets


def run_tracker(cmc_obj, frames, dets):
    import boxmot_amd

    t = boxmot_amd.BotSort(with_reid=False)
    if cmc_obj is not None:
        t.cmc = cmc_obj
    return [np.asarray(t.update(d, f)).copy() for f, d in zip(frames, dets)]


def test_ecc_drives_botsort(cmc):
    frames, dets = pan_scene()
    ref = R.EccRef(scale=None)
    ref_out = [ref.apply(f) for f in frames]
    assert [o[3] for o in ref_out] == [1] + [0] * (len(frames) - 1)
    ecc = cmc.ECC(scale=None)
    with_ecc = run_tracker(ecc, frames, dets)
    with_ref = run_tracker(StubCMC([o[0].astype(np.float32) for o in ref_out]), frames, dets)
    identity = run_tracker(None, frames, dets)
    assert sum(o.shape[0] for o in with_ecc) >= 6 * (len(frames) - 3)
    for a, b in zip(with_ecc, with_ref):
        assert np.array_equal(a, b)
    assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(with_ecc, identity))
    assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(with_ref, identity))

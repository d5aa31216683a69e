"""Sparse-optical-flow camera-motion compensation on the device against the numpy restatement
(tests/sof_ref.py): pyramid, lambda plane and keypoints bit for bit, tracking and fit within the
tolerance DESIGN.md 2.17 records, batches, capacity and errors, and the warp's way into a
tracker."""

import numpy as np
import pytest

from tests import sof_ref as R

pytestmark = pytest.mark.gpu

# Ten times the largest device-minus-restatement difference measured over every case below
# (DESIGN.md 2.17); the contract's cap is 1e-6 px (anything near it would mean float32 somewhere).
# Measured: 9.0e-9 px in a tracked position (one point of the scale 0.5 case whose iteration
# amplifies the reduction-order difference; every other case stays under 7e-13) and 3.6e-14 in a
# warp entry.
TOL_POS = 9.0e-8
TOL_WARP = 3.6e-13
assert TOL_POS <= 1e-6 and TOL_WARP <= 1e-6

EYE = np.eye(2, 3)
H, W = 96, 128
SHIFT = np.array([[1, 0, 1.3], [0, 1, -0.7]])
BIG = np.array([[1, 0, 6.0], [0, 1, -4.0]])
worst = {"pos": 0.0, "warp": 0.0}


@pytest.fixture(scope="module")
def cmc():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from boxmot_amd import cmc as m

    return m


def make(cmc, scale=None, **kw):
    """A device SOF and the restatement with the same settings."""
    s = cmc.SOF(scale=scale)
    ref_kw = {}
    for k, v in kw.items():
        if k == "criteria":
            s.criteria = v
            ref_kw["max_iter"], ref_kw["eps"] = v
        else:
            setattr(s, k, v)
            ref_kw[k] = v
    return s, R.SofRef(scale=scale, **ref_kw)


def check_state(s, r):
    """Pyramid, lambda plane (given the last frame's level 0) and keypoints, bit for bit."""
    st = s._handle.state(0)
    if r.levels is None:
        assert not st["has_prev"]
        return
    assert st["has_prev"] and len(st["levels"]) == len(r.levels)
    for a, b in zip(st["levels"], r.levels):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert np.array_equal(st["lam"], R.lam_plane(r.levels[0]))
    # detected keypoints are pixel centres (exact); kept tracked points carry the tracking's bits
    assert st["keypoints"].shape == r.kp.shape
    if np.array_equal(r.kp, np.floor(r.kp)):
        assert np.array_equal(st["keypoints"], r.kp)
    else:
        assert np.abs(st["keypoints"] - r.kp).max() <= TOL_POS


def check_step(s, r, img, what):
    """One frame through both; everything compared."""
    out = s.apply(img)
    M, code, nk, nt, ni = r.apply(img)
    got = s.last
    assert out.dtype == np.float32 and np.array_equal(out, got["warp"].astype(np.float32))
    assert (got["code"], got["n_keypoints"], got["n_tracked"], got["n_inliers"]) == (code, nk, nt, ni)
    dw = np.abs(got["warp"] - M).max()
    dp = 0.0
    if r.record is not None and code not in (R.FIRST_FRAME, R.NO_KEYPOINTS):
        p, rec = s._handle.points(0), r.record
        assert np.array_equal(p["prev"], rec["prev"])
        assert np.array_equal(p["tracked"], rec["tracked"])
        assert np.array_equal(p["iterations"], rec["iterations"])
        fin = np.isfinite(rec["next"]).all(1)
        if fin.any():
            dp = np.abs(p["next"][fin] - rec["next"][fin]).max()
        if code == R.OK:
            assert p["winner"] == rec["winner"] and np.array_equal(p["inlier"], rec["inlier"])
    worst["pos"], worst["warp"] = max(worst["pos"], dp), max(worst["warp"], dw)
    print(f"{what}: code {code} keypoints {nk} tracked {nt} inliers {ni} "
          f"max |d pos| {dp:.3e} max |d warp| {dw:.3e}")
    assert dp <= TOL_POS and dw <= TOL_WARP
    check_state(s, r)
    return got


# ------------------------------------------------------------- pyramid, lambda and keypoints
def test_pyramid_lambda_keypoints_bit_equal(cmc):
    img = np.random.default_rng(7).integers(0, 256, (37, 53), dtype=np.uint8)
    s, r = make(cmc, win_size=9, max_corners=50)  # 37x53 -> 19x27 -> 10x14; more candidates than 50
    got = check_step(s, r, img, "37x53")
    assert got["code"] == R.FIRST_FRAME and got["n_keypoints"] == 50
    assert [a.shape for a in s._handle.state(0)["levels"]] == [(37, 53), (19, 27), (10, 14)]
    assert np.count_nonzero(R.candidates(R.lam_plane(r.levels[0]), 0.01)) > 50
    # the level rule stops early: 22x30 at win 21 keeps level 0 only
    s, r = make(cmc)
    check_step(s, r, img[:22, :30], "22x30")
    assert [a.shape for a in s._handle.state(0)["levels"]] == [(22, 30)]
    # BGR and a resize in front (ECC's rule): 37x53 at 0.5 is 18x26
    bgr = np.random.default_rng(8).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    s, r = make(cmc, scale=0.5, win_size=5)
    check_step(s, r, bgr, "bgr 0.5")
    assert s._handle.state(0)["levels"][0].shape == (18, 26)


def test_selection_many_candidates_and_ties(cmc):
    # candidates spread over many waves, all kept
    s, r = make(cmc, win_size=9)
    got = check_step(s, r, R.texture(H, W, 1), "texture, 1000")
    assert 64 < got["n_keypoints"] < 1000
    # a periodic integer texture: exactly equal lambdas, the pixel index decides, also where the
    # cut at max_corners falls inside a tie
    ys, xs = np.mgrid[0:24, 0:32]
    g = (((xs % 8 < 4) ^ (ys % 8 < 4)) * 100).astype(np.uint8)
    for k in (20, 7, 1000):
        s, r = make(cmc, win_size=5, max_corners=k)
        check_step(s, r, g, f"periodic, {k}")
    assert len(np.unique(R.lam_plane(r.levels[0])[R.candidates(R.lam_plane(r.levels[0]), 0.01)])) \
        < len(r.kp)


# ----------------------------------------------------------------------------------- tracking
@pytest.mark.parametrize("name,A,kw", [
    ("four levels", SHIFT, dict(win_size=9)),
    ("one level", SHIFT, dict(win_size=9, max_level=0)),
    ("large shift", BIG, dict(win_size=9)),
    ("rotation", R.sim_warp(0.4, 1.01, 0.5, -0.3, 64, 48), dict(win_size=9)),
    ("max_iter 1", SHIFT, dict(win_size=9, criteria=(1, 0.01))),
    ("win 21", SHIFT, dict()),
])
def test_tracking_matches_restatement(cmc, name, A, kw):
    s, r = make(cmc, max_corners=200, **kw)
    check_step(s, r, R.texture(H, W, 1), name + " first")
    got = check_step(s, r, R.texture(H, W, 1, A), name)
    assert got["code"] == R.OK
    rec = r.record
    # the keypoints near the border lose their window: at level 0 (lost) or only higher up
    assert (~rec["tracked"]).any() and rec["tracked"].sum() >= 4
    if name == "max_iter 1":
        assert rec["iterations"].max() <= len(r.levels)
    if name == "four levels":
        assert len(r.levels) == 4
        half = 4
        p = rec["prev"]
        inside0 = (p[:, 0] >= half) & (p[:, 0] + half + 1 <= W - 1) & (p[:, 1] >= half) & \
            (p[:, 1] + half + 1 <= H - 1)
        p3 = p / 8
        inside3 = (np.floor(p3[:, 0] - half) >= 0) & (np.floor(p3[:, 0] - half) + 9 <= 15) & \
            (np.floor(p3[:, 1] - half) >= 0) & (np.floor(p3[:, 1] - half) + 9 <= 11)
        assert (~inside0).any() and not rec["tracked"][~inside0].any()  # out at level 0: lost
        assert (inside0 & ~inside3 & rec["tracked"]).any()               # out at level 3: skipped
    got = check_step(s, r, R.texture(H, W, 1), name + " back")  # a third frame: the state moved on
    assert got["code"] == R.OK


def test_flat_region_too_few_and_no_keypoints(cmc):
    flat = np.full((H, W), 77, np.uint8)
    # a constant image has no corner: the stream stays uninitialised, the next frame is a first one
    s, r = make(cmc, win_size=9)
    assert check_step(s, r, flat, "flat")["code"] == R.NO_KEYPOINTS
    assert check_step(s, r, R.texture(H, W, 1), "after flat")["code"] == R.FIRST_FRAME
    # faint dots: corners by their 3x3 block, but the 9x9 window fails the eigenvalue test
    faint = flat.copy()
    for x, y in [(30, 30), (60, 50), (90, 40), (40, 70), (100, 80)]:
        faint[y, x] += 1
    s, r = make(cmc, win_size=9)
    assert check_step(s, r, faint, "faint first")["n_keypoints"] >= 5
    got = check_step(s, r, faint, "faint")
    assert got["code"] == R.TOO_FEW and got["n_tracked"] == 0
    assert r.record["iterations"].max() == 0
    # three trackable points
    dots = flat.copy()
    for x, y in [(30, 30), (60, 50), (90, 40)]:
        dots[y - 1: y + 2, x - 1: x + 2] = 200
    s, r = make(cmc, win_size=9, max_corners=3)
    assert check_step(s, r, dots, "dots first")["n_keypoints"] == 3
    got = check_step(s, r, np.roll(dots, 1, axis=1), "dots")
    assert got["code"] == R.TOO_FEW and got["n_tracked"] == 3
    assert np.array_equal(got["warp"], EYE)
    # no corner on the new frame: the tracked points are kept
    s, r = make(cmc, win_size=9, max_corners=8)
    check_step(s, r, dots, "dots first")
    got = check_step(s, r, flat, "dots to flat")
    assert got["n_keypoints"] == got["n_tracked"]


def test_fit_ignores_a_moving_foreground(cmc):
    B = np.array([[1, 0, -7.0], [0, 1, 6.0]])
    s, r = make(cmc, win_size=9, max_corners=200)
    check_step(s, r, R.texture(H, W, 1), "two first")
    got = check_step(s, r, R.two_motion_frame(H, W, 1, SHIFT, B, (40, 30, 104, 78)), "two motions")
    assert got["code"] == R.OK and 4 <= got["n_inliers"] < got["n_tracked"]
    assert np.abs(got["warp"] - SHIFT).max() < 0.25


# -------------------------------------------------------------------------------------- batch
def batch_frames():
    flat = np.full((H, W), 77, np.uint8)
    t = [R.texture(H, W, k + 1) for k in range(8)]
    f1 = np.stack(t[:7] + [flat])  # stream 7: no keypoints
    mv = [SHIFT, BIG, R.sim_warp(0.4, 1.01, 0.5, -0.3, 64, 48), SHIFT, BIG, SHIFT, SHIFT]
    f2 = np.stack([R.texture(H, W, k + 1, mv[k]) for k in range(7)] + [t[7]])
    f2[5] = flat  # stream 5 sees a flat frame
    return f1, f2


def new_batch(cmc, n=8, **kw):
    b = cmc.SofBatch(n, scale=None, **kw)
    b.win_size, b.max_corners = 9, 100
    return b


def run_batch(cmc):
    f1, f2 = batch_frames()
    b = new_batch(cmc)
    outs = [b.apply(f1)]
    order = [3, 0, 7, 2, 1, 5, 6]  # stream 4 gets no frame at the second step
    outs.append(b.apply(f2[order], streams=order))
    res = [[t.cpu().numpy() for t in o] for o in outs]
    assert b.status() == 0
    return res, b


def test_batch_equals_single_streams(cmc):
    import torch

    res, b = run_batch(cmc)
    f1, f2 = batch_frames()
    assert res[0][1].tolist() == [1] * 7 + [4]
    assert res[1][1][4] == cmc.SOF_NO_FRAME and np.array_equal(res[1][0][4].reshape(2, 3), EYE)
    assert res[1][1][7] == 1  # the stream without keypoints starts over
    assert set(res[1][1].tolist()) >= {0, 1, cmc.SOF_NO_FRAME}
    for k in range(8):
        s = cmc.SOF(scale=None)
        s.win_size, s.max_corners = 9, 100
        for step, fr in enumerate([f1[k], f2[k]]):
            if step == 1 and k == 4:
                continue
            s.apply(fr)
            w, code, nk, nt, ni = (a[k] for a in res[step])
            assert np.array_equal(w.reshape(2, 3), s.last["warp"])
            assert (code, nk, nt, ni) == (s.last["code"], s.last["n_keypoints"],
                                          s.last["n_tracked"], s.last["n_inliers"])
        if k != 4:
            st1, stb = s._handle.state(0), b.state(k)
            assert np.array_equal(st1["keypoints"], stb["keypoints"])
            assert all(np.array_equal(x, y) for x, y in zip(st1["levels"], stb["levels"]))
    # the unlisted stream kept its first frame
    assert np.array_equal(b.state(4)["levels"][0], f1[4])
    # a CUDA tensor in gives the same bits
    b2 = new_batch(cmc)
    b2.apply(torch.from_numpy(f1).cuda())
    out = b2.apply(torch.from_numpy(f2).cuda())
    b3 = new_batch(cmc)
    b3.apply(f1)
    for x, y in zip(out, b3.apply(f2)):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert out[0].dtype == torch.float64 and tuple(out[0].shape) == (8, 6)


def test_batch_runs_are_bit_identical(cmc):
    r1, r2 = run_batch(cmc)[0], run_batch(cmc)[0]
    for a, b in zip(r1, r2):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_device_path_does_not_synchronise(cmc):
    """With device inputs SofBatch.apply only enqueues: torch's sync debug mode turns every
    synchronising torch call into an error."""
    import torch

    f1, f2 = (torch.from_numpy(f).cuda() for f in batch_frames())
    order = torch.tensor([3, 0, 7, 2, 1, 5, 6], device="cuda", dtype=torch.int32)
    f2o = f2[order.long()].contiguous()
    b = new_batch(cmc)
    b.apply(f1)  # builds the handle and the cached tensors (allocations may synchronise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # the probe sees a host-to-device copy
            torch.tensor([1.0, 0.0], dtype=torch.float64, device="cuda")
        out = b.apply(f2o, streams=order)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = run_batch(cmc)[0][1]
    for x, y in zip(out, ref):
        assert np.array_equal(x.cpu().numpy(), y)


def test_scale_divides_the_translation(cmc):
    a = R.texture(192, 256, 1)
    b = R.texture(192, 256, 1, np.array([[1, 0, 2.6], [0, 1, -1.4]]))
    s, r = make(cmc, scale=0.5, win_size=9, max_corners=100)
    check_step(s, r, a, "scale 0.5 first")
    got = check_step(s, r, b, "scale 0.5")
    assert got["code"] == R.OK and np.abs(got["warp"][:, 2] - [2.6, -1.4]).max() < 0.1
    s1 = cmc.SOF(scale=None)
    s1.win_size, s1.max_corners = 9, 100
    s1.apply(R.prep(a, 0.5).astype(np.uint8))
    s1.apply(R.prep(b, 0.5).astype(np.uint8))
    assert np.array_equal(got["warp"][:, 2], s1.last["warp"][:, 2] / 0.5)
    assert np.array_equal(got["warp"][:, :2], s1.last["warp"][:, :2])


# ------------------------------------------------------------------------ capacity and errors
def test_capacity_leaves_state_unchanged(cmc):
    a, c = R.texture(H, W, 1), R.texture(H, W, 1, SHIFT)
    batch = new_batch(cmc, 2, max_h=H, max_w=W)
    batch.apply(a[None], streams=[0])
    before = batch.state(0)
    with pytest.raises(ValueError, match="capacity exceeded"):
        batch.apply(np.zeros((1, H + 2, W), np.uint8), streams=[0])
    with pytest.raises(ValueError, match="capacity exceeded"):
        batch.apply(np.zeros((1, H, W + 1), np.uint8), streams=[0])
    with pytest.raises(ValueError, match="capacity exceeded"):
        batch.apply(np.zeros((3, H, W), np.uint8))
    after = batch.state(0)
    assert after["has_prev"] and np.array_equal(after["levels"][0], a)
    assert np.array_equal(after["keypoints"], before["keypoints"]) and not batch.state(1)["has_prev"]
    w, code, nk, nt, ni = (t.cpu().numpy() for t in batch.apply(c[None], streams=[0]))
    ref = R.SofRef(scale=None, win_size=9, max_corners=100)
    ref.apply(a)
    M, rcode, rnk, rnt, rni = ref.apply(c)
    assert (code[0], nk[0], nt[0], ni[0]) == (rcode, rnk, rnt, rni) and rcode == R.OK
    assert np.abs(w[0].reshape(2, 3) - M).max() <= TOL_WARP and code[1] == cmc.SOF_NO_FRAME
    # a smaller image fits; the stream's size changed, so it starts over (and says so)
    out = batch.apply(R.texture(40, 50, 2)[None], streams=[0])
    assert out[1].cpu().numpy()[0] == 1 and batch.status() == 6
    batch.reset()
    assert not batch.state(0)["has_prev"]


def test_bad_stream_index(cmc):
    import torch

    a = R.texture(H, W, 1)
    batch = new_batch(cmc, 2)
    with pytest.raises(ValueError, match="invalid argument"):
        batch.apply(a[None], streams=[2])
    with pytest.raises(ValueError, match="invalid argument"):
        batch.apply(np.stack([a, a]), streams=[1, 1])
    with pytest.raises(ValueError, match="invalid argument"):  # BX_SOF_MAX_STREAMS
        cmc._SofHandle(65536, 8, 8)
    # device-resident indices cannot be checked on the host: the frame is skipped, the status
    # latched, the other stream served
    out = batch.apply(np.stack([a, a]), streams=torch.tensor([0, 9], device="cuda"))
    assert out[1].cpu().numpy().tolist() == [1, cmc.SOF_NO_FRAME] and batch.status() == 1


# ----------------------------------------------------------------------------- into a tracker
class StubCMC:
    def __init__(self, warps):
        self.warps, self.k = warps, 0

    def apply(self, img, dets=None):
        self.k += 1
        return self.warps[self.k - 1]


def pan_scene(n_frames=10):
    """A texture panned back and forth by 7 px per frame (more than the 10 px wide boxes'
    overlap gate bridges without a warp), boxes panning with it."""
    rng = np.random.default_rng(3)
    boxes = np.array([[12, 10, 22, 24], [44, 16, 54, 30], [74, 8, 84, 22], [20, 52, 30, 66],
                      [58, 54, 68, 68], [86, 48, 96, 62]], np.float64)
    frames, dets = [], []
    for t in range(n_frames):
        c = np.array([7.0 * (t % 2) + 0.3 * t, 1.5 * np.cos(0.7 * t) - 0.4 * t])
        frames.append(np.stack([R.texture(H, W, 9, np.array([[1, 0, c[0]], [0, 1, c[1]]]))] * 3, -1))
        d = np.zeros((len(boxes), 6))
        d[:, :4] = boxes + np.tile(c, 2) + rng.normal(0, 0.05, boxes.shape)
        d[:, 4] = 0.9
        dets.append(d)
    return frames, dets


def run_tracker(cmc_obj, frames, dets):
    import boxmot_amd

    t = boxmot_amd.DeepOcSort(embedding_off=True)
    if cmc_obj is not None:
        t.cmc = cmc_obj
    return [np.asarray(t.update(d, f)).copy() for f, d in zip(frames, dets)]


def test_sof_drives_deepocsort(cmc):
    frames, dets = pan_scene()
    ref = R.SofRef(scale=None, win_size=9, max_corners=100)
    ref_out = [ref.apply(f) for f in frames]
    assert [o[1] for o in ref_out] == [1] + [0] * (len(frames) - 1)
    sof = cmc.SOF(scale=None)
    sof.win_size, sof.max_corners = 9, 100
    with_sof = run_tracker(sof, frames, dets)
    with_ref = run_tracker(StubCMC([o[0].astype(np.float32) for o in ref_out]), frames, dets)
    identity = run_tracker(None, frames, dets)
    assert sum(o.shape[0] for o in with_sof) >= 6 * (len(frames) - 4)
    for a, b in zip(with_sof, with_ref):
        assert np.array_equal(a, b)
    assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(with_sof, identity))


def test_zz_report_measured_differences(cmc):
    """Prints the largest device-minus-restatement differences of this module's cases."""
    print(f"largest |d pos| {worst['pos']:.3e} px, largest |d warp| {worst['warp']:.3e}")
    assert worst["pos"] <= TOL_POS and worst["warp"] <= TOL_WARP

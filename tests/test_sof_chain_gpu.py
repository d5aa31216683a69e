"""The chained sparse optical flow (bx_sof_apply_chain, cmc.SofChain) and the warp table built
from it.  The oracle is SofBatch.apply called one frame at a time on a second
handle; every comparison is bit equality of the warps, the codes, the three counts and the streams'
state (pyramid, keypoints, lambda plane, levels, has_prev) and tracking record."""
import functools

import numpy as np
import pytest

from tests import sof_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
# name -> (H, W, scale, settings, expected level sizes)
SIZES = {
    "24x32w5": (24, 32, None, dict(win_size=5), [(24, 32), (12, 16), (6, 8)]),
    "37x53s": (37, 53, 0.5, dict(win_size=5), [(18, 26), (9, 13)]),  # half-to-even: 18 x 26
    "96x128w21": (96, 128, None, dict(win_size=21), [(96, 128), (48, 64), (24, 32)]),
}
FIELDS = ("prev", "next", "tracked", "iterations", "inlier")


@pytest.fixture(scope="module")
def cmc():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from boxmot_amd import cmc as m

    return m


@functools.lru_cache(maxsize=None)
def clip(H, W, seed, n, t0=0):
    """n grey frames of one analytic texture seen through small known shifts."""
    out = []
    for t in range(t0, t0 + n):
        dx = 0.9 * np.sin(0.9 * t) + 0.2 * t
        dy = 0.7 * np.cos(0.7 * t) - 0.15 * t
        out.append(R.texture(H, W, seed, np.array([[1, 0, dx], [0, 1, dy]])))
    return np.stack(out)  # (shared: the tests copy before they change a frame)


def settle(obj, settings):
    for k, v in settings.items():
        setattr(obj, k, v)
    return obj


def new_chain(cmc, n_streams, max_frames, scale, settings, **kw):
    return settle(cmc.SofChain(n_streams, max_frames=max_frames, scale=scale, **kw), settings)


def stepwise(cmc, n_streams, frames, streams, scale, settings, before=None, **kw):
    """The oracle: one plain apply per frame.  Returns the five result arrays with one row per
    frame, in call order, and the batch (for its state)."""
    b = settle(cmc.SofBatch(n_streams, scale=scale, **kw), settings)
    if before is not None:
        before(b)
    rows = [[], [], [], [], []]
    for f, s in zip(frames, streams):
        out = b.apply(f[None], streams=[int(s)])
        for acc, t in zip(rows, out):
            acc.append(t.cpu().numpy()[int(s)])
    return [np.stack(r) for r in rows], b


def same_rows(got, want):
    return all(np.array_equal(np.asarray(g).reshape(np.asarray(w).shape), w)
               for g, w in zip(got, want))


def host(out):
    return [t.cpu().numpy() for t in out]


def same_state(a, b, s):
    """state() and points() of stream s of two objects, bit for bit."""
    x, y = a.state(s), b.state(s)
    if x["has_prev"] != y["has_prev"] or len(x["levels"]) != len(y["levels"]):
        return False
    if not all(np.array_equal(p, q) for p, q in zip(x["levels"], y["levels"])):
        return False
    if not np.array_equal(x["keypoints"], y["keypoints"]):
        return False
    if (x["lam"] is None) != (y["lam"] is None):
        return False
    if x["lam"] is not None and not np.array_equal(x["lam"], y["lam"]):
        return False
    p, q = a.points(s), b.points(s)
    return p["winner"] == q["winner"] and all(np.array_equal(p[k], q[k]) for k in FIELDS)


def sentinels(rows):
    import torch

    return (torch.full((rows, 6), SENTINEL, dtype=torch.float64, device="cuda"),
            *(torch.full((rows,), -7, dtype=torch.int32, device="cuda") for _ in range(4)))


# ------------------------------------------------------------ sizes, settings, the layout
@pytest.mark.parametrize("max_iter", [1, 30])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_chain_equals_stepwise(cmc, size, max_iter):
    """Streams [0, 0, 0, 1, 2, 2] in one call on a handle of 4 streams, the rows scattered into a
    larger buffer: the listed rows are the oracle's, every other row and stream 3 untouched."""
    import torch

    H, W, scale, st, levels = SIZES[size]
    st = dict(st, criteria=(max_iter, 0.01), max_corners=200)
    streams = [0, 0, 0, 1, 2, 2]
    frames = np.concatenate([clip(H, W, 1, 3), clip(H, W, 2, 1), clip(H, W, 3, 2)])
    want, oracle = stepwise(cmc, 4, frames, streams, scale, st)
    print(size, max_iter, "codes", want[1].tolist(), "keypoints", want[2].tolist(), "tracked",
          want[3].tolist(), "inliers", want[4].tolist())
    assert [want[1][k] for k in (0, 3, 4)] == [1, 1, 1]  # first frames
    assert want[1][1] == want[1][2] == want[1][5] == 0   # ordinary pairs give an estimate
    assert [a.shape for a in oracle.state(0)["levels"]] == levels

    dst = [7, 1, 4, 0, 9, 2]
    ch = new_chain(cmc, 4, 6, scale, st)
    got = host(ch.apply(frames, streams, dst=dst, out=sentinels(10)))
    assert same_rows([g[dst] for g in got], want)
    rest = [r for r in range(10) if r not in dst]
    assert np.all(got[0][rest] == SENTINEL) and all(np.all(g[rest] == -7) for g in got[1:])
    assert ch.status() == 0 == oracle.status()
    for s in range(4):
        assert same_state(ch, oracle, s), s
    assert not ch.state(3)["has_prev"]

    # a null dst is arange(n); so is a device arange
    ch2 = new_chain(cmc, 4, 6, scale, st)
    fresh = host(ch2.apply(frames, streams))
    assert same_rows(fresh, want)
    ch3 = new_chain(cmc, 4, 6, scale, st)
    out3 = ch3.apply(frames, torch.tensor(streams, device="cuda"),
                     dst=torch.arange(6, device="cuda"), out=sentinels(6))
    assert same_rows(host(out3), want)
    for c in (ch, ch2, ch3, oracle):
        c.close()


def test_cut_inside_a_lambda_tie(cmc):
    """A periodic integer texture has exactly equal lambdas: the cut at max_corners falls inside
    a tie and the pixel index decides, in every slot as in the plain apply."""
    ys, xs = np.mgrid[0:24, 0:32]
    g = (((xs % 8 < 4) ^ (ys % 8 < 4)) * 100).astype(np.uint8)
    frames = np.stack([g, np.roll(g, 1, axis=1), np.roll(g, 1, axis=0), g])
    st = dict(win_size=5, max_corners=7)
    want, oracle = stepwise(cmc, 1, frames, [0] * 4, None, st)
    lam = oracle.state(0)["lam"]
    ranked = np.sort(lam[R.candidates(lam, 0.01)])[::-1]
    assert want[2].tolist() == [7] * 4 and ranked[6] == ranked[7]
    ch = new_chain(cmc, 1, 4, None, st)
    assert same_rows(host(ch.apply(frames, [0] * 4)), want)
    assert same_state(ch, oracle, 0)


# ------------------------------------------------------------------------ lengths and cuts
def test_one_and_two_frames_equal_plain_applies(cmc):
    H, W, scale, st, _ = SIZES["24x32w5"]
    f = clip(H, W, 4, 3)
    plain = settle(cmc.SofBatch(1, scale=scale), st)
    ch = new_chain(cmc, 1, 2, scale, st)
    for k in range(3):  # n = 1, three times: the second and third read the stored state
        want = [t[0] for t in host(plain.apply(f[k][None]))]
        got = [t[0] for t in host(ch.apply(f[k][None], [0]))]
        assert same_rows(got, want), k
        assert same_state(ch, plain, 0)
    assert want[1] == 0
    want, oracle = stepwise(cmc, 1, f[:2], [0, 0], scale, st)
    ch2 = new_chain(cmc, 1, 2, scale, st)
    assert same_rows(host(ch2.apply(f[:2], [0, 0])), want)
    assert same_state(ch2, oracle, 0)


@pytest.mark.parametrize("size", ["24x32w5", "96x128w21"])
def test_chunking_is_invisible(cmc, size):
    """7 frames of one stream as one call, as 3 + 4 and as 7 chained calls of one frame."""
    H, W, scale, st, _ = SIZES[size]
    f = clip(H, W, 5, 7)
    want, oracle = stepwise(cmc, 1, f, [0] * 7, scale, st)
    assert want[1].tolist() == [1] + [0] * 6
    assert np.abs(want[0][1:, [2, 5]]).max() > 0.3  # the warps are real estimates
    for cuts in ([7], [3, 4], [1] * 7):
        ch = new_chain(cmc, 1, 7, scale, st)
        rows, a = [], 0
        for n in cuts:
            rows.append(host(ch.apply(f[a: a + n], [0] * n)))
            a += n
        got = [np.concatenate([r[q] for r in rows]) for q in range(5)]
        assert same_rows(got, want), cuts
        assert same_state(ch, oracle, 0), cuts
        ch.close()


def test_plain_apply_before_and_after_a_chain(cmc):
    """The first frame of a stream's group is tracked from what an earlier plain apply stored,
    and a plain apply after the chain reads what the chain handed over."""
    H, W, scale, st, _ = SIZES["24x32w5"]
    f0, f1 = clip(H, W, 6, 4), clip(H, W, 7, 3)
    ch = new_chain(cmc, 2, 5, scale, st)
    ch.batch.apply(np.stack([f0[0], f1[0]]))
    frames, streams = np.concatenate([f1[1:], f0[1:]]), [1, 1, 0, 0, 0]
    got = host(ch.apply(frames, streams))
    want, oracle = stepwise(cmc, 2, frames, streams, scale, st,
                            before=lambda b: b.apply(np.stack([f0[0], f1[0]])))
    assert same_rows(got, want) and want[1].tolist() == [0] * 5
    nxt = np.stack([clip(H, W, 6, 1, t0=4)[0], clip(H, W, 7, 1, t0=3)[0]])
    assert same_rows(host(ch.batch.apply(nxt)), host(oracle.apply(nxt)))
    for s in range(2):
        assert same_state(ch, oracle, s)


def test_back_to_back_calls_do_not_race(cmc):
    """Two chained calls on one stream with nothing between them: the first pair of the second
    call reads the pyramid and the keypoints that the first call's hand-over stored."""
    import torch

    H, W, scale, st, _ = SIZES["24x32w5"]
    f = clip(H, W, 10, 12)
    want, oracle = stepwise(cmc, 1, f, [0] * 12, scale, st)
    dev = torch.from_numpy(f).cuda()
    zeros = torch.zeros(6, dtype=torch.int32, device="cuda")
    ch = new_chain(cmc, 1, 6, scale, st)
    ch.apply(dev[:1], zeros[:1])  # builds the handle (allocations may synchronise)
    ch.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = ch.apply(dev[:6], zeros)
        b = ch.apply(dev[6:], zeros)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = [np.concatenate([x, y]) for x, y in zip(host(a), host(b))]
    assert same_rows(got, want)
    assert same_state(ch, oracle, 0)


# --------------------------------------------------------------- degenerate frames in mid-chain
H0, W0 = 96, 128
FLAT = np.full((H0, W0), 77, np.uint8)


def dots_image():
    d = FLAT.copy()
    for x, y in [(30, 30), (60, 50), (90, 40)]:
        d[y - 1: y + 2, x - 1: x + 2] = 200
    return d


def check_chain(cmc, frames, st, cuts):
    """One stream's frames through the oracle and through chained calls of the given lengths."""
    n = len(frames)
    want, oracle = stepwise(cmc, 1, frames, [0] * n, None, st)
    ch = new_chain(cmc, 1, max(cuts), None, st)
    rows, a = [], 0
    for k in cuts:
        rows.append(host(ch.apply(frames[a: a + k], [0] * k)))
        a += k
    got = [np.concatenate([r[q] for r in rows]) for q in range(5)]
    assert same_rows(got, want), (cuts, [g.tolist() for g in got[1:]], [w.tolist() for w in want[1:]])
    assert same_state(ch, oracle, 0), cuts
    assert ch.status() == oracle.status() == 0
    ch.close()
    return want


@pytest.mark.parametrize("cuts", [[5], [2, 3], [3, 2], [1, 4]])
def test_kept_points_and_deferred_pairs(cmc, cuts):
    """texture, dots, flat, flat, texture: the first flat frame keeps the tracked points, the
    second is tracked from them (a deferred pair, and a run of two), the texture after it too."""
    tex = R.texture(H0, W0, 1)
    frames = np.stack([tex, dots_image(), FLAT, FLAT, tex])
    want = check_chain(cmc, frames, dict(win_size=9, max_corners=8), cuts)
    code, nkp, ntrk = want[1].tolist(), want[2].tolist(), want[3].tolist()
    print("codes", code, "keypoints", nkp, "tracked", ntrk)
    assert code[0] == R.FIRST_FRAME and R.NO_KEYPOINTS not in code
    assert nkp[1] > 0 and nkp[2] == ntrk[2] and nkp[3] == ntrk[3]  # no corner: the tracked are kept
    assert code[3] == R.TOO_FEW and code[4] == R.TOO_FEW and nkp[4] > 0


@pytest.mark.parametrize("cuts", [[4], [1, 3], [2, 2]])
def test_no_keypoints_at_a_groups_start(cmc, cuts):
    """flat, flat, texture, texture: the stream stays uninitialised, then starts."""
    frames = np.stack([FLAT, FLAT, R.texture(H0, W0, 1), R.texture(H0, W0, 1, np.array(
        [[1, 0, 1.3], [0, 1, -0.7]]))])
    want = check_chain(cmc, frames, dict(win_size=9, max_corners=100), cuts)
    assert want[1].tolist() == [R.NO_KEYPOINTS, R.NO_KEYPOINTS, R.FIRST_FRAME, R.OK]
    # a whole call without a corner leaves the stream as it was: uninitialised
    ch = new_chain(cmc, 1, 2, None, dict(win_size=9))
    ch.apply(frames[:2], [0, 0])
    assert not ch.state(0)["has_prev"] and ch.points(0)["winner"] == -1


def test_too_few_in_mid_chain(cmc):
    d = dots_image()
    frames = np.stack([d, np.roll(d, 1, axis=1), d, np.roll(d, 1, axis=0)])
    want = check_chain(cmc, frames, dict(win_size=9, max_corners=3), [4])
    assert want[1].tolist() == [R.FIRST_FRAME] + [R.TOO_FEW] * 3 and want[3].tolist() == [0, 3, 3, 3]
    assert np.array_equal(want[0], np.tile(np.eye(2, 3).reshape(6), (4, 1)))


# ------------------------------------------------------------------------ capacity and errors
def test_other_working_size_is_a_first_frame(cmc):
    st = dict(win_size=5)
    big, small = clip(33, 65, 9, 2), clip(20, 30, 9, 2)
    ch = new_chain(cmc, 1, 2, None, st, max_h=33, max_w=65)
    ch.apply(big, [0, 0])
    assert ch.status() == 0
    got = host(ch.apply(small, [0, 0]))
    want, b = stepwise(cmc, 1, list(big) + list(small), [0] * 4, None, st, max_h=33, max_w=65)
    assert want[1].tolist()[2] == R.FIRST_FRAME and ch.status() == 6 == b.status()
    assert same_rows(got, [w[2:] for w in want])
    assert same_state(ch, b, 0) and ch.state(0)["levels"][0].shape == (20, 30)


def test_capacity_and_refusals(cmc):
    import torch

    H, W, scale, st, _ = SIZES["24x32w5"]
    f = clip(H, W, 11, 4)
    ch = new_chain(cmc, 2, 2, scale, st)
    ch.apply(f[:2], [0, 0])
    twin = new_chain(cmc, 2, 2, scale, st)
    twin.apply(f[:2], [0, 0])
    with pytest.raises(ValueError, match="capacity exceeded"):
        ch.apply(f[:3], [0, 0, 1])
    with pytest.raises(ValueError, match="capacity exceeded"):
        ch.apply_host(f[:3], [0, 0, 1])
    assert all(same_state(ch, twin, s) for s in range(2)) and not ch.state(1)["has_prev"]
    # the host entry itself refuses what a device call cannot check
    ch.reserve(3)
    with pytest.raises(ValueError, match="not adjacent"):
        ch.apply_host(f[:3], [0, 1, 0])
    with pytest.raises(ValueError, match="stream index out of range"):
        ch.apply_host(f[:1], [2])
    with pytest.raises(ValueError, match="not adjacent"):
        ch.apply(f[:3], [0, 1, 0])
    assert all(same_state(ch, twin, s) for s in range(2)) and ch.status() == 0
    # reserve grew the slots: three frames fit now, through either entry
    want, oracle = stepwise(cmc, 2, f, [0, 0, 0, 1], scale, st)
    got = ch.apply_host(f[2:], [0, 1])
    assert same_rows(got, [w[2:] for w in want])
    assert all(same_state(ch, oracle, s) for s in range(2))
    # a device-resident index out of range: the frame is skipped, the status latched
    ch2 = new_chain(cmc, 2, 3, scale, st)
    out = host(ch2.apply(f[:3], torch.tensor([0, 5, 1], device="cuda")))
    assert out[1].tolist() == [1, cmc.SOF_NO_FRAME, 1] and ch2.status() == 1
    assert ch2.state(0)["has_prev"] and ch2.state(1)["has_prev"]


# --------------------------------------------------------------------------------- the table
def test_sof_warp_table_equals_one_sof_per_sequence(cmc):
    """Two sequences of different frame sizes, masks with gaps, chunk 4."""
    imgs = [np.stack([np.stack([g] * 3, -1) for g in clip(48, 64, 12, 11)]),  # BGR
            clip(40, 56, 13, 9)]
    masks = [np.ones(11, bool), np.ones(9, bool)]
    masks[0][[0, 4, 5]] = False
    masks[1][[3, 8]] = False
    sof = cmc.SOF(scale=None)
    sof.win_size, sof.max_corners = 9, 100
    tab = cmc.sof_warp_table([imgs[0], lambda t: imgs[1][t]], masks, sof=sof, chunk=4)
    assert sof._handle is None and sof.last is None  # only its settings were read
    got = tab.host()
    assert set(got) == {"warps", "rho", "iterations", "code", "n_keypoints", "n_tracked",
                        "n_inliers"}
    assert got["warps"].shape == (11, 2, 6) and got["n_inliers"].shape == (11, 2)
    assert tab.warps.is_cuda and isinstance(tab, cmc.WarpTable)
    assert not got["rho"].any() and not got["iterations"].any()
    eye = np.eye(2, 3).reshape(6)
    n_ok = 0
    for s in range(2):
        e = cmc.SOF(scale=None)
        e.win_size, e.max_corners = 9, 100
        for t in range(11):
            if t >= masks[s].size or not masks[s][t]:
                assert np.array_equal(got["warps"][t, s], eye) and got["code"][t, s] == -1
                assert got["n_keypoints"][t, s] == got["n_tracked"][t, s] == 0
                continue
            w32 = e.apply(imgs[s][t])
            assert np.array_equal(got["warps"][t, s], e.last["warp"].reshape(6)), (s, t)
            assert np.array_equal(got["warps"][t, s].astype(np.float32), w32.reshape(6))
            assert (got["code"][t, s], got["n_keypoints"][t, s], got["n_tracked"][t, s],
                    got["n_inliers"][t, s]) == (e.last["code"], e.last["n_keypoints"],
                                                e.last["n_tracked"], e.last["n_inliers"])
            n_ok += e.last["code"] == 0
    assert n_ok == sum(int(m.sum()) - 1 for m in masks)  # every pair but the first frames
    same = cmc.sof_warp_table(imgs, masks, sof=sof, chunk=64).host()
    assert all(np.array_equal(same[k], got[k]) for k in got)
    tab.close()
    assert tab.warps is None and tab.n_tracked is None

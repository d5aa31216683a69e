"""The chained ECC apply (bx_ecc_apply_chain, cmc.EccChain) and the warp table built from it
(DESIGN.md 2.19).  The oracle is EccBatch.apply called one frame at a time on a second handle;
every comparison is bit equality of warps, rho, iterations, codes and the streams' state."""
import functools

import numpy as np
import pytest

from tests import ecc_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
# (H, W, scale): fewer pixels than the 1024 threads; several pixels per thread and no multiple of
# 64; a working size from half-to-even rounding (18 x 26)
SIZES = {"5x7": (5, 7, None), "33x65": (33, 65, None), "37x53s": (37, 53, 0.5)}


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
        out.append(R.texture(H, W, seed, R.shift_warp(dx, dy)))
    return np.stack(out)  # (shared: the tests copy before they change a frame)


def states(obj, n_streams):
    return [obj.state(s) for s in range(n_streams)]


def same_state(a, b):
    if a[0] != b[0]:
        return False
    return not a[0] or all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def stepwise(cmc, n_streams, frames, streams, kw, before=None):
    """The oracle: one plain apply per frame.  Returns ([n, 6], rho, iterations, code) rows in
    call order, the batch (for its state) and its latched status."""
    b = cmc.EccBatch(n_streams, **kw)
    if before is not None:
        before(b)
    rows = [[], [], [], []]
    for f, s in zip(frames, streams):
        out = b.apply(f[None], streams=[int(s)])
        for acc, t in zip(rows, out):
            acc.append(t.cpu().numpy()[int(s)])
    return [np.stack(r) for r in rows], b


def same_rows(got, want):
    return all(np.array_equal(np.asarray(g).reshape(np.asarray(w).shape), w, equal_nan=True)
               for g, w in zip(got, want))


def host(out):
    return [t.cpu().numpy() for t in out]


# --------------------------------------------------------------- sizes, models, iteration caps
@pytest.mark.parametrize("max_iter", [1, 3])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["translation", "euclidean", "affine"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_chain_equals_stepwise(cmc, size, mode, max_iter):
    """Streams [0, 0, 0, 1, 2, 2] in one call on a handle of 4 streams, the rows scattered into a
    larger buffer: the listed rows are the oracle's, every other row and stream 3 untouched."""
    import torch

    H, W, scale = SIZES[size]
    kw = dict(warp_mode=mode, max_iter=max_iter, scale=scale)
    streams = [0, 0, 0, 1, 2, 2]
    frames = np.concatenate([clip(H, W, 1, 3), clip(H, W, 2, 1), clip(H, W, 3, 2)])
    want, oracle = stepwise(cmc, 4, frames, streams, kw)
    assert want[3].tolist() == [1, want[3][1], want[3][2], 1, 1, want[3][5]]  # first frames
    assert np.array_equal(want[0][0], np.eye(2, 3).reshape(6))

    dst = [7, 1, 4, 0, 9, 2]
    out = (torch.full((10, 6), SENTINEL, dtype=torch.float64, device="cuda"),
           torch.full((10,), SENTINEL, dtype=torch.float64, device="cuda"),
           torch.full((10,), -7, dtype=torch.int32, device="cuda"),
           torch.full((10,), -7, dtype=torch.int32, device="cuda"))
    ch = cmc.EccChain(4, max_frames=6, **kw)
    got = host(ch.apply(frames, streams, dst=dst, out=out))
    assert same_rows([g[dst] for g in got], want)
    rest = [r for r in range(10) if r not in dst]
    assert np.all(got[0][rest] == SENTINEL) and np.all(got[1][rest] == SENTINEL)
    assert np.all(got[2][rest] == -7) and np.all(got[3][rest] == -7)
    assert ch.status() == 0 == oracle.status()
    for s in range(4):
        assert same_state(ch.state(s), oracle.state(s)), s
    assert not ch.state(3)[0]

    # a null dst is arange(n)
    ch2 = cmc.EccChain(4, max_frames=6, **kw)
    assert same_rows(host(ch2.apply(frames, streams)), want)
    ch3 = cmc.EccChain(4, max_frames=6, **kw)
    out3 = ch3.apply(frames, streams, dst=torch.arange(6, device="cuda"),
                     out=(torch.zeros(6, 6, dtype=torch.float64, device="cuda"),
                          torch.zeros(6, dtype=torch.float64, device="cuda"),
                          torch.zeros(6, dtype=torch.int32, device="cuda"),
                          torch.zeros(6, dtype=torch.int32, device="cuda")))
    assert same_rows(host(out3), want)
    for c in (ch, ch2, ch3, oracle):
        c.close()


@pytest.mark.parametrize("size", sorted(SIZES))
def test_one_and_two_frames_equal_plain_applies(cmc, size):
    H, W, scale = SIZES[size]
    kw = dict(scale=scale)
    f = clip(H, W, 4, 3)
    plain = cmc.EccBatch(1, **kw)
    ch = cmc.EccChain(1, max_frames=2, **kw)
    for k in range(3):  # n = 1, three times: the second and third read the stored previous
        want = [t[0] for t in host(plain.apply(f[k][None]))]
        got = [t[0] for t in host(ch.apply(f[k][None], [0]))]
        assert same_rows(got, want), k
        assert same_state(ch.state(0), plain.state(0))
    assert want[3] == 0 or size == "5x7"  # an ordinary pair converges
    want, oracle = stepwise(cmc, 1, f[:2], [0, 0], kw)
    ch2 = cmc.EccChain(1, max_frames=2, **kw)
    assert same_rows(host(ch2.apply(f[:2], [0, 0])), want)
    assert same_state(ch2.state(0), oracle.state(0))


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["translation", "euclidean", "affine"])
def test_chunking_is_invisible(cmc, mode):
    """7 frames of one stream as one call, as 3 + 4 and as 7 chained calls of one frame."""
    kw = dict(warp_mode=mode, scale=None)
    f = clip(33, 65, 5, 7)
    want, oracle = stepwise(cmc, 1, f, [0] * 7, kw)
    assert want[3].tolist() == [1] + [0] * 6 and np.all(want[2][1:] >= 2)
    shifts = want[0][1:, [2, 5]]
    assert np.abs(shifts).max() > 0.3  # the warps are real estimates, not identities
    for cuts in ([7], [3, 4], [1] * 7):
        ch = cmc.EccChain(1, max_frames=7, **kw)
        rows, a = [], 0
        for n in cuts:
            rows.append(host(ch.apply(f[a: a + n], [0] * n)))
            a += n
        got = [np.concatenate([r[q] for r in rows]) for q in range(4)]
        assert same_rows(got, want), cuts
        assert same_state(ch.state(0), oracle.state(0)), cuts
        ch.close()


def test_plain_apply_then_chain(cmc):
    """The first frame of a stream's group is aligned to what an earlier plain apply stored."""
    kw = dict(scale=None)
    f0, f1 = clip(33, 65, 6, 4), clip(33, 65, 7, 3)
    ch = cmc.EccChain(2, max_frames=5, **kw)
    ch.batch.apply(np.stack([f0[0], f1[0]]))
    got = host(ch.apply(np.concatenate([f1[1:], f0[1:]]), [1, 1, 0, 0, 0]))
    want, oracle = stepwise(cmc, 2, np.concatenate([f1[1:], f0[1:]]), [1, 1, 0, 0, 0], kw,
                            before=lambda b: b.apply(np.stack([f0[0], f1[0]])))
    assert same_rows(got, want) and want[3].tolist() == [0] * 5
    # and a plain apply after the chain reads what the chain handed over
    nxt = np.stack([clip(33, 65, 6, 1, t0=4)[0], clip(33, 65, 7, 1, t0=3)[0]])
    assert same_rows(host(ch.batch.apply(nxt)), host(oracle.apply(nxt)))
    for s in range(2):
        assert same_state(ch.state(s), oracle.state(s))


# -------------------------------------------------------------------------------------- codes
def test_constant_frame_in_a_chain(cmc):
    """A constant image gives NaN rho and code 2; the next pair has it as its template."""
    kw = dict(scale=None)
    f = clip(33, 65, 8, 5).copy()
    f[2] = 77
    want, oracle = stepwise(cmc, 1, f, [0] * 5, kw)
    assert want[3][0] == 1 and want[3][1] == 0 and want[3][2] == 2 and np.isnan(want[1][2])
    assert want[3][3] == 2  # (template constant: NaN again, as the oracle has it)
    ch = cmc.EccChain(1, max_frames=5, **kw)
    got = host(ch.apply(f, [0] * 5))
    assert same_rows(got, want)
    assert np.array_equal(got[0][2], np.eye(2, 3).reshape(6))
    assert same_state(ch.state(0), oracle.state(0))


def test_other_working_size_is_a_first_frame(cmc):
    kw = dict(scale=None, max_h=33, max_w=65)
    big, small = clip(33, 65, 9, 2), clip(20, 30, 9, 2)
    ch = cmc.EccChain(1, max_frames=2, **kw)
    ch.apply(big, [0, 0])
    assert ch.status() == 0
    got = host(ch.apply(small, [0, 0]))
    b = cmc.EccBatch(1, **kw)
    rows = []
    for fr in (big[0], big[1], small[0], small[1]):
        rows.append([t[0] for t in host(b.apply(fr[None]))])
    assert got[3].tolist() == [1, rows[3][3]] and ch.status() == 6 == b.status()
    assert same_rows([g[0] for g in got], rows[2]) and same_rows([g[1] for g in got], rows[3])
    assert same_state(ch.state(0), b.state(0)) and ch.state(0)[1].shape == (20, 30)


# -------------------------------------------------------------------------------- the hazard
def test_back_to_back_calls_do_not_race(cmc):
    """Two chained calls on one stream with nothing between them: the first frame of the second
    call reads, for its whole loop, the image the first call's hand-over stored."""
    import torch

    kw = dict(scale=None)
    f = clip(33, 65, 10, 12)
    want, oracle = stepwise(cmc, 1, f, [0] * 12, kw)
    dev = torch.from_numpy(f).cuda()
    zeros = torch.zeros(6, dtype=torch.int32, device="cuda")
    ch = cmc.EccChain(1, max_frames=6, **kw)
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
    assert same_state(ch.state(0), oracle.state(0))


# ------------------------------------------------------------------------ capacity and errors
def test_capacity_and_refusals(cmc):
    import torch

    kw = dict(scale=None)
    f = clip(33, 65, 11, 4)
    ch = cmc.EccChain(2, max_frames=2, **kw)
    ch.apply(f[:2], [0, 0])
    before = states(ch, 2)
    with pytest.raises(ValueError, match="capacity exceeded"):
        ch.apply(f[:3], [0, 0, 1])
    with pytest.raises(ValueError, match="capacity exceeded"):
        ch.apply_host(f[:3], [0, 0, 1])
    after = states(ch, 2)
    assert all(same_state(a, b) for a, b in zip(before, after)) and not after[1][0]
    # the host entry itself refuses what a device call cannot check
    ch.reserve(3)
    with pytest.raises(ValueError, match="not adjacent"):
        ch.apply_host(f[:3], [0, 1, 0])
    with pytest.raises(ValueError, match="stream index out of range"):
        ch.apply_host(f[:1], [2])
    with pytest.raises(ValueError, match="not adjacent"):
        ch.apply(f[:3], [0, 1, 0])
    assert all(same_state(a, b) for a, b in zip(before, states(ch, 2))) and ch.status() == 0
    # reserve grew the slots: three frames fit now, through either entry
    want, oracle = stepwise(cmc, 2, f, [0, 0, 0, 1], kw)
    got = ch.apply_host(f[2:], [0, 1])
    assert same_rows(got, [w[2:] for w in want])
    # a device-resident index out of range: the frame is skipped, the status latched
    ch2 = cmc.EccChain(2, max_frames=3, **kw)
    out = host(ch2.apply(f[:3], torch.tensor([0, 5, 1], device="cuda")))
    assert out[3].tolist() == [1, cmc.NO_FRAME, 1] and ch2.status() == 1
    assert ch2.state(0)[0] and ch2.state(1)[0]


# --------------------------------------------------------------------------------- the table
def test_warp_table_equals_one_ecc_per_sequence(cmc):
    """Three sequences, two frame sizes, masks with gaps, chunk 4."""
    imgs = [np.stack([np.stack([g] * 3, -1) for g in clip(33, 65, 12, 11)]),  # BGR
            clip(20, 30, 13, 9), np.stack([np.stack([g] * 3, -1) for g in clip(33, 65, 14, 12)])]
    masks = [np.ones(11, bool), np.ones(9, bool), np.ones(12, bool)]
    masks[0][[0, 4, 5]] = False
    masks[1][[3, 8]] = False
    masks[2][[1, 10, 11]] = False
    kw = dict(warp_mode=0, eps=1e-5, max_iter=100, scale=None)
    tab = cmc.warp_table([imgs[0], lambda t: imgs[1][t], imgs[2]], masks, chunk=4, **kw)
    got = tab.host()
    assert got["warps"].shape == (12, 3, 6) and got["code"].shape == (12, 3)
    assert tab.warps.is_cuda and tab.n_frames == 12 and tab.n_seq == 3
    eye = np.eye(2, 3).reshape(6)
    n_ok = 0
    for s in range(3):
        e = cmc.ECC(**kw)
        for t in range(12):
            if t >= masks[s].size or not masks[s][t]:
                assert np.array_equal(got["warps"][t, s], eye) and got["code"][t, s] == -1
                assert got["rho"][t, s] == 0 and got["iterations"][t, s] == 0
                continue
            e.apply(imgs[s][t])
            assert np.array_equal(got["warps"][t, s], e.last["warp"].reshape(6)), (s, t)
            assert got["rho"][t, s] == e.last["rho"] and got["code"][t, s] == e.last["code"]
            assert got["iterations"][t, s] == e.last["iterations"]
            n_ok += e.last["code"] == 0
    assert n_ok == sum(int(m.sum()) - 1 for m in masks)  # every pair but the first frames
    same = cmc.warp_table(imgs, masks, chunk=64, **kw).host()
    assert all(np.array_equal(same[k], got[k]) for k in got)
    tab.close()
    assert tab.warps is None

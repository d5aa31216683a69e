"""The detector front end on the device against the numpy restatement (tests/det_ref.py), bit for
bit: the letterbox in every type and geometry, the filter and the order of the candidates, the
suppression on boxes whose IoUs are exact, the two caps, independence of the images, and the
front end around a tiny model and into an engine."""

import numpy as np
import pytest

from tests import det_ref as D

pytestmark = pytest.mark.gpu

H, W = 48, 64


@pytest.fixture(scope="module")
def det():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from boxmot_amd import det as m

    return m


@pytest.fixture(scope="module")
def frames():
    return np.random.default_rng(27).integers(0, 256, (3, H, W, 3), dtype=np.uint8)


def same(got, want):
    """Equal types and shapes, NaNs in the same places, the same bits everywhere else (a NaN's
    payload is not part of the contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan],
                                                                 want.view(u)[~nan])


# --------------------------------------------------------------------------------- letterbox
#        limited by W, rows padded   W again   H: columns padded, a run across the edge
SIZES = [(32, 40), (40, 32), (27, 45), (96, 128), (50, 64), (7, 9)]
#                                       exact x2   2 rows   odd in_w: the store tail


@pytest.mark.parametrize("swap_rb", [True, False], ids=["rgb", "bgr"])
@pytest.mark.parametrize("half", [False, True], ids=["float32", "half"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_letterbox_is_bit_equal(det, frames, size, half, swap_rb):
    got, r = det.letterbox(frames, size, half=half, swap_rb=swap_rb)
    want, wr = D.letterbox(frames, size, half=half, swap_rb=swap_rb)
    assert r == wr and same(got.cpu().numpy(), want)
    got, _ = det.letterbox(frames, size, half=half, swap_rb=swap_rb, mean=None, std=None)
    assert same(got.cpu().numpy(), D.letterbox(frames, size, half=half, swap_rb=swap_rb,
                                               mean=None, std=None)[0])
    got, _ = det.letterbox(frames, size, half=half, swap_rb=swap_rb, std=None)
    assert same(got.cpu().numpy(), D.letterbox(frames, size, half=half, swap_rb=swap_rb,
                                               std=None)[0])


@pytest.mark.parametrize("half", [False, True], ids=["float32", "half"])
def test_letterbox_padding_is_the_value_of_114(det, frames, half):
    for size, (rh, rw) in (((50, 64), (48, 64)), ((27, 45), (27, 36)), ((32, 40), (30, 40)),
                           ((96, 128), (96, 128))):
        assert det.letterbox_geometry(H, W, size)[1:] == (rh, rw)
        got = det.letterbox(frames, size, half=half)[0].cpu().numpy()
        for c in range(3):
            pad = np.float32((114.0 / 255.0 - D.YOLOX_MEAN[c]) / D.YOLOX_STD[c])
            pad = pad.astype(np.float16) if half else pad
            assert np.all(got[:, c, rh:, :] == pad) and np.all(got[:, c, :, rw:] == pad)


def test_letterbox_frames_are_independent_and_inputs_may_live_anywhere(det, frames):
    import torch

    full = det.letterbox(frames, (27, 45))[0].cpu().numpy()
    for f in range(3):
        one, r = det.letterbox(frames[f], (27, 45))  # [H, W, 3]
        assert one.shape == (1, 3, 27, 45) and same(one.cpu().numpy()[0], full[f])
    dev = torch.from_numpy(frames).cuda()
    out = torch.full((3, 3, 27, 45), 7.0, device="cuda")
    got, _ = det.letterbox(dev, (27, 45), out=out)
    assert got is out and same(out.cpu().numpy(), full)
    with pytest.raises(ValueError):
        det.letterbox(dev, (27, 45), out=torch.empty(3, 3, 27, 44, device="cuda"))
    with pytest.raises(ValueError):
        det.letterbox(dev, (27, 45), half=True, out=out)
    assert det.letterbox(dev[:0], (27, 45))[0].shape == (0, 3, 27, 45)


def test_letterbox_at_the_model_size(det):
    big = np.random.default_rng(5).integers(0, 256, (1, 135, 240, 3), dtype=np.uint8)
    got, r = det.letterbox(big, (200, 360), half=True)  # 1080p into 800 x 1440, an eighth of it
    want, wr = D.letterbox(big, (200, 360), half=True)
    assert r == wr and same(got.cpu().numpy(), want)


# ----------------------------------------------------------------------------- post-process
def run_pp(det, pred, **kw):
    """postprocess on the device, cut to the rows det_off names."""
    import torch

    t = pred if isinstance(pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pred)).cuda()
    dets, off, anc, code = det.postprocess(t, **kw)
    off = off.cpu().numpy()
    B = t.shape[0]
    md = kw.get("max_det") or kw.get("cand_cap", 4096)
    assert dets.shape == (B * md, 6) and anc.shape == (B * md,) and off.shape == (B + 1,)
    return dets.cpu().numpy()[:off[-1]], off, anc.cpu().numpy()[:off[-1]], code.cpu().numpy()


def check(det, pred, **kw):
    got = run_pp(det, pred, **kw)
    okw = dict(kw)
    if "iou" in okw:
        okw["iou_thr"] = okw.pop("iou")
    want = D.postprocess(pred, **okw)
    for g, w, name in zip(got, want, ("dets", "det_off", "anchor_of", "code")):
        assert same(g, w), name
    return got


def spread(A, C, dtype=np.float32):
    """[A, 5 + C] rows whose boxes never touch (a 10-pixel grid, sides 4..6), class scores 0."""
    p = np.zeros((A, 5 + C), dtype)
    k = np.arange(A)
    p[:, 0], p[:, 1] = 10 * (k % 32) + 5, 10 * (k // 32) + 5
    p[:, 2], p[:, 3] = 4 + k % 3, 4 + k % 2
    return p


def filter_pred(A, C, dtype=np.float32):
    """Three images: no candidate; a mix with many exact ties, a score of exactly conf (0.25), a
    NaN score and a NaN coordinate; every row a candidate with one score."""
    rng = np.random.default_rng([A, C])
    pred = np.stack([spread(A, C, dtype) for _ in range(3)])
    cls = rng.integers(0, C, (3, A))
    conf = np.stack([np.full(A, 0.125), rng.choice([0.125, 0.25, 0.5, 0.75, 0.9], A),
                     np.full(A, 0.5)]).astype(dtype)
    conf[1, 0] = 0.25  # exactly the threshold: kept
    np.put_along_axis(pred[:, :, 5:], cls[..., None], conf[..., None], 2)
    pred[:, :, 4] = 1.0
    pred[1, 1::7, 4] = 0.5  # some objectness below one: more values, more ties (0.25 again)
    if A > 3:
        pred[1, 2, 4] = np.nan       # a NaN score is no candidate
        pred[1, 3, 0] = np.nan       # a NaN coordinate stays one, and is reported
        pred[1, 3, 5:] = 0.0
        pred[1, 3, 5 + C - 1] = 0.9
    return pred


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("A", [1, 63, 64, 65, 257, 1000])
def test_filter_and_order(det, A, C):
    pred = filter_pred(A, C)
    dets, off, anc, code = check(det, pred, conf=0.25, cand_cap=1024)
    assert off[1] == 0 and off[3] - off[2] == A and not code.any()
    assert np.array_equal(anc[off[2]:], np.arange(A))  # equal scores: by row
    assert 0 in anc[off[1]:off[2]]                     # the score of exactly conf
    if A > 3:
        mid = anc[off[1]:off[2]]
        assert 2 not in mid and 3 in mid
        assert np.isnan(dets[off[1]:off[2]][mid == 3][0, [0, 2]]).all()
    s = dets[off[1]:off[2], 4]
    assert np.all(s[:-1] >= s[1:]) and (A < 63 or len(np.unique(s)) < len(s))  # ties exist
    tie = s[:-1] == s[1:]
    assert np.all(np.diff(anc[off[1]:off[2]])[tie] > 0)


@pytest.mark.parametrize("A", [65, 257])
def test_half_and_strided_pred(det, A):
    import torch

    pred = filter_pred(A, 3, np.float16)
    check(det, pred, conf=0.25, cand_cap=512)
    wide = np.zeros((3, A + 2, 11), np.float32)
    wide[:, :, 9:] = 7.0
    wide[:, 1:A + 1, :8] = filter_pred(A, 3)
    view = torch.from_numpy(wide).cuda()[:, 1:A + 1, :8]
    assert view.stride() == ((A + 2) * 11, 11, 1) and not view.is_contiguous()
    got = run_pp(det, view, conf=0.25, cand_cap=512)
    want = D.postprocess(filter_pred(A, 3), conf=0.25, cand_cap=512)
    assert all(same(g, w) for g, w in zip(got, want))


def rows_of(boxes, scores, cls=None, C=1):
    """pred rows [n, 5 + C] of xyxy boxes with even integer corners (centres and sizes exact)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    p = np.zeros((len(b), 5 + C), np.float32)
    p[:, 0], p[:, 1] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    p[:, 2], p[:, 3] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    p[:, 4] = 1.0
    p[np.arange(len(b)), 5 + (np.zeros(len(b), int) if cls is None else np.asarray(cls))] = scores
    return p


def falling(n):
    """n scores strictly falling, exact in float32."""
    return (1.0 - np.arange(n) / 1024.0).astype(np.float32)


def test_iou_exactly_at_the_threshold_and_one_ulp_above(det):
    # the second box lies inside the first and has half its area: IoU = 8 / 16, exactly 0.5
    pred = rows_of([[0, 0, 4, 4], [0, 0, 4, 2], [20, 0, 24, 4]], falling(3))[None]
    assert D.iou(D.corners(pred[0])[0], D.corners(pred[0])[1]) == np.float32(0.5)
    _, off, anc, _ = check(det, pred, iou=0.5)
    assert anc.tolist() == [0, 1, 2]  # not above the threshold: kept
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    _, off, anc, _ = check(det, pred, iou=below)
    assert anc.tolist() == [0, 2]


def chain_scene():
    """150 rows in score order.  a (row 3) suppresses b, b alone would suppress c: b and c sit
    in a's block (rows 5, 9), and a second chain a', b', c' (rows 10, 70, 140) spans three
    blocks; everything else is far away and alone."""
    far = [[40 * (k % 20), 100 + 40 * (k // 20), 40 * (k % 20) + 10, 110 + 40 * (k // 20)]
           for k in range(150)]
    for row, x in ((3, 0), (5, 2), (9, 4)):
        far[row] = [x, 0, x + 10, 10]
    for row, x in ((10, 100), (70, 102), (140, 104)):
        far[row] = [x, 0, x + 10, 10]
    return rows_of(far, falling(150))[None]


def test_chains_inside_a_block_and_across_blocks(det):
    pred = chain_scene()
    _, off, anc, _ = check(det, pred, iou=0.5)
    assert sorted(set(range(150)) - set(anc.tolist())) == [5, 70]
    # the order of the rows is not the order of the candidates: the same boxes, rows reversed
    _, _, anc, _ = check(det, pred[:, ::-1].copy(), iou=0.5)
    assert sorted(set(range(150)) - set(anc.tolist())) == [149 - 70, 149 - 5]


def test_identical_and_zero_area_boxes(det):
    pred = rows_of(np.tile([[6, 6, 16, 18]], (130, 1)), np.full(130, 0.5, np.float32))[None]
    _, off, anc, _ = check(det, pred, iou=0.7)
    assert anc.tolist() == [0]  # equal scores: the first row is the first candidate
    # zero-area boxes: four at one point (0 / 0: NaN suppresses nothing), one inside a real box
    pred = rows_of([[4, 4, 4, 4]] * 4 + [[0, 0, 10, 10], [6, 6, 6, 8]], falling(6))[None]
    _, off, anc, _ = check(det, pred, iou=0.0)
    assert anc.tolist() == [0, 1, 2, 3, 4, 5]


def test_classes_agnostic_and_the_class_list(det):
    # two boxes on top of each other with classes 0 and 2, a third of class 2 beside them
    boxes = [[0, 0, 10, 10], [0, 0, 10, 10], [30, 0, 40, 10]]
    pred = rows_of(boxes, falling(3), cls=[0, 2, 2], C=3)[None]
    _, _, anc, _ = check(det, pred)
    assert anc.tolist() == [0, 1, 2]
    _, _, anc, _ = check(det, pred, class_agnostic=True)
    assert anc.tolist() == [0, 2]
    # class 0 is not reported, but its box suppressed the class-2 box under it first
    dets, _, anc, _ = check(det, pred, class_agnostic=True, classes=[2])
    assert anc.tolist() == [2] and dets[0, 5] == 2
    _, _, anc, _ = check(det, pred, classes=[2, 1])
    assert anc.tolist() == [1, 2]
    _, off, _, _ = check(det, pred, classes=[1])
    assert off.tolist() == [0, 0]


@pytest.mark.parametrize("n", [65, 200])
def test_candidate_cap(det, n):
    rng = np.random.default_rng(n)
    pred = spread(n, 1)
    pred[:, 4] = 1.0
    pred[:, 5] = rng.permutation(falling(n))
    dets, off, anc, code = check(det, pred[None], cand_cap=64)
    assert code.tolist() == [D.CAND_OVERFLOW] and off.tolist() == [0, 64]
    assert np.array_equal(anc, np.argsort(-pred[:, 5], kind="stable")[:64])
    _, off, _, code = check(det, pred[None, :64], cand_cap=64)
    assert code.tolist() == [0] and off.tolist() == [0, 64]  # exactly the cap: no flag


def test_max_det_and_offsets_with_an_empty_image(det):
    nine = spread(9, 1)
    nine[:, 4] = 1.0
    nine[:, 5] = falling(9)[::-1]
    none = spread(9, 1)
    pred = np.stack([nine, none, nine])
    pred[2, 4:, 5] = 0.0  # image 2: four candidates
    dets, off, anc, code = check(det, pred, max_det=5)
    assert off.tolist() == [0, 5, 5, 9] and code.tolist() == [D.MAX_DET, 0, 0]
    assert anc.tolist() == [8, 7, 6, 5, 4, 3, 2, 1, 0]
    _, off, _, code = check(det, pred, max_det=9)
    assert off.tolist() == [0, 9, 9, 13] and not code.any()  # exactly the limit: no flag
    _, off, _, code = check(det, pred[:, :0])
    assert off.tolist() == [0, 0, 0, 0] and not code.any()   # A == 0


def test_images_are_independent_and_outputs_may_be_given(det):
    import torch

    pred = np.concatenate([filter_pred(257, 3), chain_scene_c3()])
    full = run_pp(det, pred, conf=0.25, iou=0.5, cand_cap=512, ratio=0.75)
    for b in range(4):
        d, off, anc, code = run_pp(det, pred[b:b + 1], conf=0.25, iou=0.5, cand_cap=512,
                                   ratio=0.75)
        lo, hi = full[1][b], full[1][b + 1]
        assert same(d, full[0][lo:hi]) and same(anc, full[2][lo:hi]) and code[0] == full[3][b]
    ratio = torch.tensor([1.0, 0.5, 2.0, 0.75], device="cuda")
    out = (torch.zeros(4 * 512, 6, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda"),
           torch.zeros(4 * 512, dtype=torch.int32, device="cuda"),
           torch.zeros(4, dtype=torch.int32, device="cuda"))
    fo = torch.full((4 * 512,), -1, dtype=torch.int32, device="cuda")
    got = det.postprocess(torch.from_numpy(pred).cuda(), conf=0.25, iou=0.5, cand_cap=512,
                          ratio=ratio, out=out, frame_of=fo)
    assert all(g is o for g, o in zip(got, out))
    want = D.postprocess(pred, conf=0.25, iou_thr=0.5, cand_cap=512, ratio=[1.0, 0.5, 2.0, 0.75])
    n = int(want[1][-1])
    assert same(out[0].cpu().numpy()[:n], want[0]) and same(out[1].cpu().numpy(), want[1])
    assert not out[0].cpu().numpy()[n:].any()  # rows past det_off[B] are left alone
    assert np.array_equal(fo.cpu().numpy()[:n], np.repeat(np.arange(4), np.diff(want[1])))
    with pytest.raises(ValueError):
        det.postprocess(torch.from_numpy(pred).cuda(), cand_cap=512, out=out[:3])
    with pytest.raises(ValueError):
        det.postprocess(torch.from_numpy(pred).cuda(), cand_cap=256, out=out)
    with pytest.raises(ValueError):
        det.postprocess(torch.from_numpy(pred), cand_cap=512)


def chain_scene_c3():
    p = chain_scene()
    out = np.zeros((1, 257, 8), np.float32)
    out[0, :150, :6] = p[0]
    return out


def test_a_long_candidate_list_sorts_in_chunks(det):
    """More candidates than one chunk of the sort holds (8192): the merges across chunks."""
    A = 20000
    rng = np.random.default_rng(3)
    pred = np.zeros((2, A, 6), np.float32)
    pred[:, :, :4] = [5, 5, 4, 4]
    pred[:, :, 4] = 1.0
    pred[0, :, 5] = rng.integers(1, 64, A) / 64.0  # 63 values: long runs of ties
    pred[1, :9000, 5] = rng.permutation(9000) / 16384.0 + 0.25
    got = run_pp(det, pred, conf=0.01, iou=1.0, cand_cap=1024)  # (IoU 1 is never above 1)
    s0 = -pred[0, :, 5]
    order0 = np.lexsort((np.arange(A), s0))[:1024]
    order1 = np.argsort(-pred[1, :, 5], kind="stable")[:1024]
    assert got[1].tolist() == [0, 1024, 2048] and got[3].tolist() == [1, 1]
    assert np.array_equal(got[2][:1024], order0) and np.array_equal(got[2][1024:], order1)
    assert np.array_equal(got[0][:1024, 4], pred[0, order0, 5])


# --------------------------------------------------------------------------------- front end
def lookup_model(table, lib):
    """The tiny deterministic "model": a fixed table of predictions, with the objectness of row 0
    switched by the sign of the input's first element, so that the letterbox is in the result.
    ``lib`` is torch or numpy: both sides of a comparison run the same function."""
    hi, lo = table[0, 0, 4] * 0 + 0.875, table[0, 0, 4] * 0 + 0.75

    def model(x):
        y = table[: x.shape[0]].clone() if lib.__name__ == "torch" else table[: x.shape[0]].copy()
        y[:, 0, 4] = lib.where(x[:, 0, 0, 0] > 0, hi, lo)
        return y

    return model


def moving_table(t):
    """[3, 40, 6]: 12 candidates per image that drift with t, pairs of them overlapping."""
    p = np.stack([spread(40, 1) for _ in range(3)])
    p[:, :, 4] = 1.0
    p[:, :12, 5] = falling(12) * 0.9
    p[:, 12:, 5] = 0.001
    p[:, :12, 0] += 0.5 * t + np.arange(3)[:, None]
    p[:, 2, :4] = p[:, 1, :4] + [0.25, 0.25, 0, 0]  # on top of row 1: suppressed
    return p.astype(np.float32)


def test_front_end_is_model_on_restated_letterbox(det, frames):
    import torch

    table = moving_table(0)
    front = det.DetFrontEnd(lookup_model(torch.from_numpy(table).cuda(), torch),
                            input_size=(27, 45), conf=0.01, iou=0.7)
    x, r = D.letterbox(frames, (27, 45))
    assert len(set((x[:, 0, 0, 0] > 0).tolist())) == 2  # both branches of the model are taken
    want = D.postprocess(lookup_model(table, np)(x), conf=0.01, iou_thr=0.7, ratio=r)
    fo = torch.full((3 * 4096,), -1, dtype=torch.int32, device="cuda")
    dets, off, anc, code = front.detect(torch.from_numpy(frames).cuda(), frame_of=fo)
    n = int(want[1][-1])
    assert n == 33 and same(off.cpu().numpy(), want[1]) and same(dets.cpu().numpy()[:n], want[0])
    assert same(anc.cpu().numpy()[:n], want[2]) and not code.cpu().numpy().any()
    assert np.array_equal(fo.cpu().numpy()[:n], np.repeat(np.arange(3), 11))
    # one image, numpy in and out (the model sees a batch of one: the table's first image)
    mn = lookup_model(table, np)
    one = front(frames[1])
    assert one.dtype == np.float32 and same(one, D.postprocess(mn(x[1:2]), ratio=r)[0])
    # a model that returns a tuple, called in chunks of `batch` frames
    mt = front.model
    tup = det.DetFrontEnd(lambda x: (mt(x), None), input_size=(27, 45), batch=2)
    want2 = D.postprocess(np.concatenate([mn(x[:2]), mn(x[2:])]), ratio=r)
    got2 = tup.detect(torch.from_numpy(frames).cuda())
    assert same(got2[1].cpu().numpy(), want2[1])
    assert same(got2[0].cpu().numpy()[:int(want2[1][-1])], want2[0])


def test_call_returns_an_empty_array_for_no_detections(det, frames):
    import torch

    quiet = torch.zeros(1, 40, 6, device="cuda")
    front = det.DetFrontEnd(lambda x: quiet, input_size=(27, 45))
    out = front(frames[0])
    assert out.shape == (0, 6) and out.dtype == np.float32
    with pytest.raises(ValueError):
        front(frames[0].astype(np.float32))
    with pytest.raises(ValueError):
        front.detect(frames)  # numpy: detect takes CUDA frames


def test_detect_feeds_a_bytetrack_engine(det, frames):
    """The front end's dets / det_off go into Engine.step as they are; the rows are those the
    same engine gives on the restatement's detections."""
    import torch

    from boxmot_amd.engine import Engine

    dev_frames = torch.from_numpy(frames).cuda()
    x, r = D.letterbox(frames, (27, 45))

    def track(feed):
        eng = Engine("bytetrack", n_seq=3, track_cap=64, det_cap=64)
        rows = []
        for t in range(4):
            table = moving_table(t)
            if feed == "device":
                front = det.DetFrontEnd(lookup_model(torch.from_numpy(table).cuda(), torch),
                                        input_size=(27, 45), max_det=64)
                dets, off, _, _ = front.detect(dev_frames)
            else:
                d, o, _, _ = D.postprocess(lookup_model(table, np)(x), ratio=r)
                dets, off = torch.from_numpy(d).cuda(), torch.from_numpy(o).cuda()
            out = torch.zeros((3 * 64, 8), dtype=torch.float64, device="cuda")
            cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
            eng.step(dets, off, None, None, out, cnt)
            torch.cuda.synchronize()
            off, cnt, out = off.cpu().numpy(), cnt.cpu().numpy(), out.cpu().numpy()
            rows.append([out[off[s]: off[s] + cnt[s]] for s in range(3)])
        assert eng.status() == 0
        return rows

    a, b = track("device"), track("host")
    assert sum(len(r) for fr in a for r in fr) > 60  # (not a comparison of empty outputs)
    for fa, fb in zip(a, b):
        for ra, rb in zip(fa, fb):
            assert np.array_equal(ra, rb)


def test_detect_does_not_synchronise(det, frames):
    """With CUDA frames detect only enqueues: torch's sync debug mode turns every synchronising
    torch call (a copy from host values among them) into an error."""
    import torch

    table = moving_table(1)
    front = det.DetFrontEnd(lookup_model(torch.from_numpy(table).cuda(), torch),
                            input_size=(27, 45), classes=[0])
    dev = torch.from_numpy(frames).cuda()
    front.detect(dev)  # builds the buffers and the cached constants (these may synchronise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # the probe sees a host-to-device copy
            torch.tensor([1.0, 0.0], dtype=torch.float64, device="cuda")
        dets, off, anc, code = front.detect(dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    x, r = D.letterbox(frames, (27, 45))
    want = D.postprocess(lookup_model(table, np)(x), ratio=r, classes=[0])
    assert same(off.cpu().numpy(), want[1])
    assert same(dets.cpu().numpy()[:int(want[1][-1])], want[0])

"""The ReID front end on the device against the numpy restatement (tests/reid_ref.py), bit for
bit: crops in every layout and type, empty boxes, independence of the boxes, the unit rows
against numpy itself, the front end around a tiny model, and its way into the trackers."""

import numpy as np
import pytest

from tests import reid_ref as R

pytestmark = pytest.mark.gpu

H, W = 48, 64
SIZES = [(16, 8), (12, 10), (9, 7)]


@pytest.fixture(scope="module")
def reid():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from boxmot_amd import reid as m

    return m


@pytest.fixture(scope="module")
def frames():
    return np.random.default_rng(11).integers(0, 256, (3, H, W, 3), dtype=np.uint8)


def box_set(oh, ow):
    """Every kind of box the contract names, none of them empty."""
    return np.array([
        [10.3, 5.7, 30.2, 40.9], [3.25, 2.75, 9.6, 20.1], [40.49, 1.51, 52.2, 46.8],  # interior
        [2.5, 3.5, 20.5, 30.5], [11.5, 0.5, 13.5, 47.5],               # corners at exactly .5
        [-5, 10, 12, 30], [50, 10, 70, 30], [10, -7, 30, 12], [10, 40, 30, 55],  # one border each
        [-4, -4, 70, 60],                                                # all four
        [20, 10, 21, 30], [20, 10, 40, 11], [63, 47, 64, 48],            # width 1, height 1, both
        [30, 20, 33, 24], [1, 1, 63, 47],                                # upscaled, downscaled
        [5, 6, 5 + ow, 6 + oh],                                          # the output's size
        [0, 0, W, H],                                                    # the whole frame
    ], np.float32)


def bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    return np.array_equal(bits(np.ascontiguousarray(got)), bits(np.ascontiguousarray(want)))


def run(reid, frames, boxes, frame_of=None, **kw):
    import torch

    n = len(boxes)
    codes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    out = reid.crop_batch(frames, boxes, frame_of, codes=codes, **kw)
    return out.cpu().numpy(), codes.cpu().numpy()


# ------------------------------------------------------------------------------------- crops
@pytest.mark.parametrize("swap_rb", [True, False], ids=["rgb", "bgr"])
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("half", [False, True], ids=["float32", "half"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_crops_are_bit_equal(reid, frames, size, half, nhwc, swap_rb):
    boxes = box_set(*size)
    fo = (np.arange(len(boxes)) * 2) % 3
    kw = dict(size=size, half=half, nhwc=nhwc, swap_rb=swap_rb)
    got, codes = run(reid, frames, boxes, fo, **kw)
    want, wcodes = R.crops(frames, boxes, fo, **kw)
    assert not wcodes.any() and np.array_equal(codes, wcodes)
    assert same(got, want)


@pytest.mark.parametrize("half", [False, True], ids=["float32", "half"])
@pytest.mark.parametrize("size", [(256, 128), (384, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_sized_crops(reid, frames, size, half):
    boxes = np.array([[10.3, 5.7, 30.2, 40.9], [-4, -4, 70, 60], [20, 10, 21, 30]], np.float32)
    got, codes = run(reid, frames, boxes, [2, 0, 1], size=size, half=half)
    want, wcodes = R.crops(frames, boxes, [2, 0, 1], size=size, half=half)
    assert np.array_equal(codes, wcodes) and same(got, want)


def random_boxes(n, seed):
    rng = np.random.default_rng(seed)
    x1, y1 = rng.uniform(-6, W - 2, n), rng.uniform(-6, H - 2, n)
    b = np.stack([x1, y1, x1 + rng.uniform(1, 40, n), y1 + rng.uniform(1, 40, n)], 1)
    return b.astype(np.float32), rng.integers(0, 3, n).astype(np.int32)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("n", [0, 1, 67])
def test_box_counts_over_three_frames(reid, frames, n, nhwc):
    boxes, fo = random_boxes(n, 100 + n)
    for size in ((12, 10), (9, 7)):
        got, codes = run(reid, frames, boxes, fo, size=size, nhwc=nhwc)
        want, wcodes = R.crops(frames, boxes, fo, size=size, nhwc=nhwc)
        assert np.array_equal(codes, wcodes) and same(got, want)


def test_frame_of_null_and_host_or_device_inputs(reid, frames):
    import torch

    boxes, _ = random_boxes(9, 7)
    want, wcodes = R.crops(frames[:1], boxes, None, size=(16, 8))
    got, codes = run(reid, frames, boxes, None, size=(16, 8))  # every box reads frame 0
    assert same(got, want) and np.array_equal(codes, wcodes)
    one = reid.crop_batch(frames[0], boxes.astype(np.float64), size=(16, 8))  # [H, W, 3], float64
    assert same(one.cpu().numpy(), want)
    dev = reid.crop_batch(torch.from_numpy(frames).cuda(), torch.from_numpy(boxes).cuda(),
                          torch.zeros(9, dtype=torch.int64, device="cuda"), size=(16, 8))
    assert same(dev.cpu().numpy(), want)


def test_empty_boxes_get_the_code_and_a_zero_row(reid, frames):
    import torch

    good = [10.3, 5.7, 30.2, 40.9]
    rows = [  # (box, frame, constructed to be empty)
        (good, 0, False), ([30, 10, 20, 40], 0, True), (good, 1, False),
        ([10, 40, 30, 20], 1, True), ([70, 10, 90, 40], 2, True), ([10, -30, 30, -2], 0, True),
        (good, 2, False), ([np.nan, 5, 30, 40], 0, True), ([10, 5, np.inf, 40], 1, True),
        ([-np.inf, 5, 30, 40], 1, True), ([1e9, 5, 2e9, 40], 2, True), (good, 0, False),
        (good, 3, True), (good, -1, True), ([10, 10, 10.4, 40], 0, True),
        ([-1e9, -1e9, 1e9, 1e9], 1, False), (good, 1, False)]
    boxes = np.array([r[0] for r in rows], np.float32)
    fo = np.array([r[1] for r in rows], np.int32)
    built_empty = np.array([r[2] for r in rows])
    want, wcodes = R.crops(frames, boxes, fo, size=(12, 10))
    assert np.array_equal(wcodes == R.EMPTY, built_empty)  # the restatement: exactly that set
    for half in (False, True):
        want, _ = R.crops(frames, boxes, fo, size=(12, 10), half=half)
        out = torch.full((len(rows), 3, 12, 10), 7.0, device="cuda",
                         dtype=torch.float16 if half else torch.float32)
        codes = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
        reid.crop_batch(frames, boxes, fo, size=(12, 10), half=half, out=out, codes=codes)
        got, codes = out.cpu().numpy(), codes.cpu().numpy()
        assert set(np.flatnonzero(codes == reid.CROP_EMPTY)) <= set(np.flatnonzero(built_empty))
        assert np.array_equal(codes, wcodes)
        assert not got[built_empty].any()           # zero rows, written over the fill
        assert same(got, want)                      # neighbours untouched
    # codes are optional
    assert same(reid.crop_batch(frames, boxes, fo, size=(12, 10)).cpu().numpy(),
                R.crops(frames, boxes, fo, size=(12, 10))[0])


def test_boxes_are_independent(reid, frames):
    boxes, fo = random_boxes(67, 167)
    full, codes = run(reid, frames, boxes, fo, size=(9, 7), half=True)
    rng = np.random.default_rng(1)
    for k in (1, 5, 31):
        idx = rng.choice(67, k, replace=False)
        part, pcodes = run(reid, frames, boxes[idx], fo[idx], size=(9, 7), half=True)
        assert same(part, full[idx]) and np.array_equal(pcodes, codes[idx])


def test_crop_arguments_are_checked(reid, frames):
    import torch

    boxes = np.array([[1, 1, 9, 9]], np.float32)
    with pytest.raises(ValueError):
        reid.crop_batch(frames, boxes, std=(0.2, 0.0, 0.2))
    with pytest.raises(ValueError):
        reid.crop_batch(frames, boxes, size=(0, 8))
    with pytest.raises(ValueError):
        reid.crop_batch(frames.astype(np.float32), boxes)
    with pytest.raises(ValueError):
        reid.crop_batch(frames, boxes, [0, 1])
    with pytest.raises(ValueError):
        reid.crop_batch(frames, boxes, out=torch.empty(1, 3, 8, 8, device="cuda"))


# ----------------------------------------------------------------------------- normalisation
def numpy_rows(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.linalg.norm(x, axis=-1, keepdims=True)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("F", [1, 7, 128, 129, 512, 2051])
def test_unit_rows_match_numpy(reid, F, n):
    import torch

    x = np.random.default_rng([F, n]).standard_normal((n, F)).astype(np.float32)
    x *= np.float32(3.7)
    got = reid.normalize_features(torch.from_numpy(x).cuda())
    assert same(got.cpu().numpy(), numpy_rows(x))
    # float64 out: the exact widening
    got64 = reid.normalize_features(torch.from_numpy(x).cuda(), torch.float64)
    assert same(got64.cpu().numpy(), numpy_rows(x).astype(np.float64))
    # fp16 in: the same expression on the widened array
    xh = x.astype(np.float16)
    goth = reid.normalize_features(torch.from_numpy(xh).cuda())
    assert same(goth.cpu().numpy(), numpy_rows(xh.astype(np.float32)))
    assert same(goth.cpu().numpy(), R.unit_rows(xh))


def test_unit_rows_strided_and_zero_row(reid):
    import torch

    x = np.random.default_rng(4).standard_normal((9, 200)).astype(np.float32)
    x[4] = 0.0
    wide = torch.from_numpy(x).cuda()
    view = wide[:, :129]  # row stride 200, F = 129
    assert view.stride(0) == 200 and not view.is_contiguous()
    got = reid.normalize_features(view).cpu().numpy()
    want = numpy_rows(x[:, :129].copy())
    assert np.isnan(want[4]).all() and np.isnan(got[4]).all()
    keep = np.arange(9) != 4
    assert same(got[keep], want[keep])
    assert reid.normalize_features(torch.empty(0, 16, device="cuda")).shape == (0, 16)
    with pytest.raises(ValueError):
        reid.normalize_features(torch.empty(4, device="cuda"))
    with pytest.raises(ValueError):
        reid.normalize_features(wide, torch.float16)


# --------------------------------------------------------------------------------- front end
def tiny_model():
    """One conv, a mean over space, a linear layer to 16; fixed seed."""
    import torch

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 4, 3, padding=1)
            self.fc = torch.nn.Linear(4, 16)

        def forward(self, x):
            return self.fc(self.conv(x).mean((2, 3)))

    torch.manual_seed(0)
    return Tiny().cuda().eval()


def model_on_restated(model, frames, boxes, fo, size, chunks):
    """model(restated crops, uploaded) chunk by chunk, then numpy's division."""
    import torch

    crops, _ = R.crops(frames, boxes, fo, size=size)
    with torch.no_grad():
        y = [model(torch.from_numpy(crops[lo:hi]).cuda()).cpu().numpy() for lo, hi in chunks]
    return numpy_rows(np.concatenate(y))


def test_get_features_is_model_on_restated_crops(reid, frames):
    model = tiny_model()
    boxes = box_set(16, 8)[:12]
    front = reid.ReidFrontEnd(model, input_shape=(16, 8))
    got = front.get_features(boxes.astype(np.float64), frames[1])
    assert got.dtype == np.float32 and got.shape == (12, 16)
    assert same(got, model_on_restated(model, frames[1:2], boxes, None, (16, 8), [(0, 12)]))
    # chunked by `batch`: the same chunks through the model
    front5 = reid.ReidFrontEnd(model, input_shape=(16, 8), batch=5)
    assert same(front5.get_features(boxes, frames[1]),
                model_on_restated(model, frames[1:2], boxes, None, (16, 8),
                                  [(0, 5), (5, 10), (10, 12)]))
    # a model that returns a tuple; no boxes
    tup = reid.ReidFrontEnd(lambda x: (model(x), None), input_shape=(16, 8))
    assert same(tup.get_features(boxes, frames[1]), got)
    empty = front.get_features(np.empty((0, 4)), frames[1])
    assert empty.shape == (0,) and empty.dtype == np.float64


def test_features_over_three_frames(reid, frames):
    import torch

    model = tiny_model()
    # one crop per model call on both sides: the model's own arithmetic sees the same shapes
    front = reid.ReidFrontEnd(model, input_shape=(16, 8), batch=1)
    boxes = np.concatenate([box_set(16, 8)[:5], box_set(16, 8)[9:14]])
    fo = np.array([2, 0, 1, 1, 0, 2, 2, 0, 1, 0], np.int32)
    feats, codes = front.features(torch.from_numpy(frames).cuda(), torch.from_numpy(boxes).cuda(),
                                  torch.from_numpy(fo).cuda())
    assert feats.is_cuda and feats.dtype == torch.float32 and not codes.cpu().numpy().any()
    feats = feats.cpu().numpy()
    for f in range(3):
        assert same(feats[fo == f], front.get_features(boxes[fo == f], frames[f]))
    out = torch.empty(10, 16, device="cuda")
    again, _ = front.features(torch.from_numpy(frames).cuda(), torch.from_numpy(boxes).cuda(),
                              torch.from_numpy(fo).cuda(), out=out)
    assert again is out and same(out.cpu().numpy(), feats)


def test_an_empty_crop_raises_or_is_flagged(reid, frames):
    import torch

    front = reid.ReidFrontEnd(tiny_model(), input_shape=(16, 8))
    boxes = np.array([[10, 5, 30, 40], [3, 3, 9, 20], [30, 10, 20, 40], [70, 1, 90, 9]],
                     np.float32)
    with pytest.raises(ValueError, match="box 2 "):
        front.get_features(boxes, frames[0])
    _, codes = front.features(torch.from_numpy(frames).cuda(), torch.from_numpy(boxes).cuda())
    assert codes.cpu().numpy().tolist() == [0, 0, 1, 1]


# ---------------------------------------------------------------------------------- trackers
def make_tracker(name):
    import boxmot_amd as B

    return {
        "botsort": lambda: B.BotSort(),
        "boosttrack": lambda: B.BoostTrack(with_reid=True),
        "strongsort": lambda: B.StrongSort(),
        "deepocsort": lambda: B.DeepOcSort(),
        "hybridsort": lambda: B.HybridSort(None, None, False, 0.3),
        "deepocsort_per_class": lambda: B.DeepOcSortPerClass(nr_classes=2),
        "hybridsort_per_class": lambda: B.HybridSortPerClass(None, None, False, 0.3,
                                                             nr_classes=2),
    }[name]()


TRACKERS = ["botsort", "boosttrack", "strongsort", "deepocsort", "hybridsort",
            "deepocsort_per_class", "hybridsort_per_class"]


def strongsort_frames():
    """Five frames of four 6x10 objects in the lower right of the image.  The default occlusion
    handler reads tlwh rows as xyxy and raises TypeError on the overlaps
    that reading finds; boxes whose left edge lies right of every width have none."""
    rng = np.random.default_rng(31)
    c0 = np.array([[36.0, 30.0], [46.0, 30.0], [56.0, 30.0], [46.0, 42.0]])
    half = np.array([3.0, 5.0])
    out = []
    for t in range(1, 6):
        c = c0 + 0.3 * t
        box = np.concatenate([c - half, c + half], 1) + rng.normal(0.0, 0.2, (4, 4))
        out.append(np.concatenate([box, np.full((4, 1), 0.9), np.zeros((4, 1))], 1))
    return out


@pytest.mark.parametrize("name", TRACKERS)
def test_tracker_with_a_model_equals_tracker_fed_embs(reid, name, monkeypatch):
    from boxmot_amd.synth import SyntheticScene

    if name == "strongsort":
        # the reference never matches a Tentative track, so StrongSort
        # reports nothing, on any scene, unless tracks are born confirmed as in the reference's
        # own CI (sort/track.py:98-105).  Everything else is the default configuration.
        monkeypatch.setenv("GITHUB_ACTIONS", "true")
        monkeypatch.delenv("GITHUB_JOB", raising=False)

    img = np.random.default_rng(21).integers(0, 256, (H, W, 3), dtype=np.uint8)
    scene = SyntheticScene(n_obj=8, seed=3, p_det=0.9, width=float(W), height=float(H),
                           classes=(0, 1) if name.endswith("per_class") else ())
    front = reid.ReidFrontEnd(tiny_model(), input_shape=(16, 8), batch=1)
    frames = [scene.frame(t)[0] for t in range(1, 6)]
    if name == "strongsort":
        frames = strongsort_frames()
    assert all(len(d) for d in frames)

    def run_frames(feed):
        # (one tracker after the other: the id counters are class attributes, as the reference's,
        # and every constructor but BoostTrack's resets its own)
        import boxmot_amd as B

        B.BoostTrack._id_count = 0
        tr = make_tracker(name)
        assert tr.model is None
        if not feed:
            tr.model = front
        return [np.asarray(tr.update(d, img, front.get_features(d[:, 0:4], img)) if feed
                           else tr.update(d, img)) for d in frames]

    with_model, fed = run_frames(False), run_frames(True)
    for t, (a, b) in enumerate(zip(with_model, fed), 1):
        assert same(a, b), (name, t)
    assert sum(a.shape[0] for a in with_model if a.size) > 0  # (not a comparison of empty outputs)


ERRORS = {
    "botsort": "BotSort(with_reid=True) on the MI355X engine needs `embs`: ReID inference is "
               "outside the association path",
    "boosttrack": "BoostTrack with_reid on the engine needs precomputed embeddings",
    "strongsort": "StrongSort on the engine needs precomputed embeddings",
    "deepocsort": "DeepOcSort(embedding_off=False) on the MI355X engine needs `embs`: ReID "
                  "inference is outside the association path",
    "hybridsort": "HybridSort on the MI355X engine needs `embs`: ReID inference is outside the "
                  "association path",
}


@pytest.mark.parametrize("name", TRACKERS)
def test_tracker_without_a_model_raises_as_before(reid, name):
    tr = make_tracker(name)
    dets = np.array([[5, 5, 20, 40, 0.9, 0], [30, 5, 45, 40, 0.8, 1]])
    with pytest.raises(ValueError) as e:
        tr.update(dets, np.zeros((H, W, 3), np.uint8))
    assert str(e.value) == ERRORS[name.replace("_per_class", "")]

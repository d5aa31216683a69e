"""boxmot_amd.tune.sweep_bot on the GPU: the files of a K-config sweep of ByteTrack and BoT-SORT
against run_sequences once per config (its default path: every frame assembled on the host), byte
for byte, BoT-SORT also under warps and a sub-range of frames; the rows in memory against the
files; and the sweep's scores, on the device and on the host, against evaluate_mot of those
files."""
import numpy as np
import pytest

from tests import sweep_bot_data as BD
from tests import sweep_reid_data as RD
from tests import tune_data as TD

pytestmark = pytest.mark.gpu

S, K = BD.S, BD.K
KINDS = list(BD.KINDS)


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return t


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    from boxmot_amd import motio

    d = tmp_path_factory.mktemp("bot_packed")
    out = {}
    for s in range(S):
        rows, embs = RD.packed_rows(BD.scene(s))
        out[f"seq{s}"] = motio.pack_arrays(rows, embs, d / f"seq{s}.bxmot")
    return out


def _warps():
    """name -> the warp at every iterated frame: the frames that have detections."""
    out = {}
    for s in range(S):
        has = [bool(d.shape[0]) for d, _ in BD.scene(s)]
        out[f"seq{s}"] = RD.frame_warps(s)[has]
    return out


WARPS = _warps()


@pytest.fixture(scope="module")
def loop(torch, packed, tmp_path_factory):
    """The loop the sweep replaces: run_sequences once per config; root/<kind> and, for BoT-SORT
    under warps, root/warp."""
    from boxmot_amd import motio

    root = tmp_path_factory.mktemp("bot_loop")
    for kind in KINDS:
        for k, cfg in enumerate(BD.configs(kind)):
            motio.run_sequences(kind, packed, root / kind / f"{k:04d}", tracker_kwargs=cfg)
    for k, cfg in enumerate(BD.configs("botsort")):
        motio.run_sequences("botsort", packed, root / "warp" / f"{k:04d}", tracker_kwargs=cfg,
                            warps=WARPS)
    return root


def same_files(got, want, names):
    texts = []
    for k in range(K):
        for nm in names:
            a = (got / f"{k:04d}" / f"{nm}.txt").read_bytes()
            assert a == (want / f"{k:04d}" / f"{nm}.txt").read_bytes(), (k, nm)
            assert len(a) > 500
            texts.append(a)
    return texts


@pytest.mark.parametrize("kind", KINDS)
def test_sweep_files_match_run_sequences(torch, packed, loop, tmp_path, kind):
    from boxmot_amd import tune

    cfgs = BD.configs(kind)
    res = tune.sweep_bot(kind, packed, cfgs, exp_dir=tmp_path)
    assert [r["config"] for r in res] == cfgs and all(r["summary"] is None for r in res)
    texts = same_files(tmp_path, loop / kind, packed)
    assert len(set(texts)) == K * S  # the configs tell themselves apart on every sequence
    assert sorted(p.name for p in tmp_path.iterdir()) == ["0000", "0001", "0002"]
    for k in range(K):  # the rows in memory are the files' rows
        for nm in packed:
            rows = res[k]["results"][nm]
            file_rows = np.loadtxt(tmp_path / f"{k:04d}" / f"{nm}.txt", delimiter=",", ndmin=2)
            assert rows.dtype == np.float64 and rows.shape == file_rows.shape
            np.testing.assert_array_equal(rows[:, :8], file_rows[:, :8])


def test_sweep_without_reid_matches_run_sequences(torch, packed, tmp_path):
    """with_reid=False in every config: an engine without embeddings fed from sequences that have
    them."""
    from boxmot_amd import motio, tune

    cfgs = BD.configs("botsort", with_reid=False)
    tune.sweep_bot("botsort", packed, cfgs, exp_dir=tmp_path / "sweep")
    for k, cfg in enumerate(cfgs):
        motio.run_sequences("botsort", packed, tmp_path / "loop" / f"{k:04d}", tracker_kwargs=cfg)
    same_files(tmp_path / "sweep", tmp_path / "loop", packed)


def test_sweep_with_warps_matches_run_sequences(torch, packed, loop, tmp_path):
    """Every config's copy of a sequence gets that sequence's warp; the warps change the rows."""
    from boxmot_amd import tune

    tune.sweep_bot("botsort", packed, BD.configs("botsort"), exp_dir=tmp_path, warps=WARPS)
    texts = same_files(tmp_path, loop / "warp", packed)
    plain = same_files(loop / "botsort", loop / "botsort", packed)
    assert texts != plain


@pytest.mark.parametrize("kind", KINDS)
def test_sweep_honours_frame_ids(torch, packed, tmp_path, kind):
    from boxmot_amd import motio, tune

    fids = {"seq0": list(range(5, 30))}
    cfgs = BD.configs(kind)[:2]
    tune.sweep_bot(kind, packed, cfgs, exp_dir=tmp_path / "sweep", frame_ids=fids)
    for k, cfg in enumerate(cfgs):
        motio.run_sequences(kind, packed, tmp_path / "loop" / f"{k:04d}", frame_ids=fids,
                            tracker_kwargs=cfg)
        for nm in packed:
            a = (tmp_path / "sweep" / f"{k:04d}" / f"{nm}.txt").read_bytes()
            assert a == (tmp_path / "loop" / f"{k:04d}" / f"{nm}.txt").read_bytes(), (k, nm)
            assert len(a) > 500


@pytest.mark.parametrize("kind", KINDS)
def test_sweep_scores_match_evaluate_mot(torch, packed, loop, kind):
    from boxmot_amd import evaluate_mot, mot_summary, tune

    gt = {f"seq{s}": TD.synthetic_gt(s) for s in range(S)}
    cfgs = BD.configs(kind)
    host = tune.sweep_bot(kind, packed, cfgs, gt=gt)
    dev = tune.sweep_bot(kind, packed, cfgs, gt=gt, score="device")
    lean = tune.sweep_bot(kind, packed, cfgs, gt=gt, score="device", keep_results=False)
    summaries = []
    for k in range(K):
        want = mot_summary(evaluate_mot(gt, loop / kind / f"{k:04d}"))
        assert host[k]["summary"] == want and dev[k]["summary"] == want, k
        assert lean[k]["summary"] == want and lean[k]["results"] is None, k
        assert all(dev[k]["results"][nm].tobytes() == host[k]["results"][nm].tobytes()
                   for nm in packed)
        assert want["HOTA"] > 5.0
        summaries.append(tuple(want.values()))
    assert len(set(summaries)) == K

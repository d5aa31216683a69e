"""boxmot_amd.tune.sweep_boost on the GPU: the files of a K-config BoostTrack sweep against
run_sequences once per config (its default path: every frame assembled on the host), byte for
byte, with and without ReID, with and without warps, and over a sub-range of frames that holds a
frame without detections; the rows in memory against the files; and the sweep's scores, on the
device and on the host, against evaluate_mot of those files."""
import numpy as np
import pytest

from tests import sweep_boost_data as BD
from tests import tune_data as TD

pytestmark = pytest.mark.gpu

S, K = BD.S, BD.K
# run_sequences refuses warps for a config that switches use_ecc off: the warp sweeps leave it out
ECC_ON = [k for k, c in enumerate(BD.CONFIGS) if c.get("use_ecc", True)]


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

    d = tmp_path_factory.mktemp("boost_packed")
    out = {}
    for s in range(S):
        rows, embs = BD.packed_rows(BD.scene(s))
        out[f"seq{s}"] = motio.pack_arrays(rows, embs, d / f"seq{s}.bxmot")
    return out


def _warps():
    """name -> the warp at every iterated frame: the frames that have detections."""
    out = {}
    for s in range(S):
        has = [bool(d.shape[0]) for d, _ in BD.scene(s)]
        out[f"seq{s}"] = BD.warps(s)[has]
    return out


WARPS = _warps()


@pytest.fixture(scope="module")
def loop(torch, packed, tmp_path_factory):
    """The loop the sweep replaces: run_sequences once per config; root/reid, root/noreid and,
    under warps, root/warp (the configs of ECC_ON)."""
    from boxmot_amd import motio

    root = tmp_path_factory.mktemp("boost_loop")
    for name, reid in (("reid", True), ("noreid", False)):
        for k, cfg in enumerate(BD.configs(reid)):
            motio.run_sequences("boosttrack", packed, root / name / f"{k:04d}",
                                tracker_kwargs=cfg)
    for j, k in enumerate(ECC_ON):
        motio.run_sequences("boosttrack", packed, root / "warp" / f"{j:04d}",
                            tracker_kwargs=BD.configs()[k], warps=WARPS)
    return root


def same_files(got, want, names, n):
    texts = []
    for k in range(n):
        for nm in names:
            a = (got / f"{k:04d}" / f"{nm}.txt").read_bytes()
            assert a == (want / f"{k:04d}" / f"{nm}.txt").read_bytes(), (k, nm)
            assert len(a) > 500
            texts.append(a)
    return texts


@pytest.mark.parametrize("name,reid", [("reid", True), ("noreid", False)])
def test_sweep_files_match_run_sequences(torch, packed, loop, tmp_path, name, reid):
    """Without ReID: an engine without embeddings fed from sequences that have them."""
    from boxmot_amd import tune

    cfgs = BD.configs(reid)
    res = tune.sweep_boost(packed, cfgs, exp_dir=tmp_path)
    assert [r["config"] for r in res] == cfgs and all(r["summary"] is None for r in res)
    texts = same_files(tmp_path, loop / name, packed, K)
    assert len(set(texts)) == K * S  # the configs tell themselves apart on every sequence
    assert sorted(p.name for p in tmp_path.iterdir()) == [f"{k:04d}" for k in range(K)]
    for k in range(K):  # the rows in memory are the files' rows
        for nm in packed:
            rows = res[k]["results"][nm]
            file_rows = np.loadtxt(tmp_path / f"{k:04d}" / f"{nm}.txt", delimiter=",", ndmin=2)
            assert rows.dtype == np.float64 and rows.shape == file_rows.shape
            np.testing.assert_array_equal(rows[:, :8], file_rows[:, :8])


def test_sweep_with_warps_matches_run_sequences(torch, packed, loop, tmp_path):
    """Every config's copy of a sequence gets that sequence's warp; the warps change the rows."""
    from boxmot_amd import tune

    cfgs = [BD.configs()[k] for k in ECC_ON]
    tune.sweep_boost(packed, cfgs, exp_dir=tmp_path, warps=WARPS)
    texts = same_files(tmp_path, loop / "warp", packed, len(cfgs))
    plain = [(loop / "reid" / f"{k:04d}" / f"{nm}.txt").read_bytes() for k in ECC_ON
             for nm in packed]
    assert all(a != b for a, b in zip(texts, plain))


def test_sweep_without_reid_with_warps(torch, packed, tmp_path):
    from boxmot_amd import motio, tune

    cfgs = [BD.configs(False)[k] for k in ECC_ON][:3]
    tune.sweep_boost(packed, cfgs, exp_dir=tmp_path / "sweep", warps=WARPS)
    for k, cfg in enumerate(cfgs):
        motio.run_sequences("boosttrack", packed, tmp_path / "loop" / f"{k:04d}",
                            tracker_kwargs=cfg, warps=WARPS)
    same_files(tmp_path / "sweep", tmp_path / "loop", packed, len(cfgs))


def test_sweep_honours_frame_ids(torch, packed, tmp_path):
    """A sub-range of sequence 1 that holds its frame without detections (TD.EMPTY)."""
    from boxmot_amd import motio, tune

    assert TD.EMPTY == (1, 9)
    fids = {"seq1": list(range(5, 30))}
    cfgs = BD.configs()[:3]
    tune.sweep_boost(packed, cfgs, exp_dir=tmp_path / "sweep", frame_ids=fids)
    for k, cfg in enumerate(cfgs):
        got = motio.run_sequences("boosttrack", packed, tmp_path / "loop" / f"{k:04d}",
                                  frame_ids=fids, tracker_kwargs=cfg)
        assert got["seq1"] == fids["seq1"]
    texts = same_files(tmp_path / "sweep", tmp_path / "loop", packed, len(cfgs))
    frames = np.loadtxt(tmp_path / "sweep" / "0000" / "seq1.txt", delimiter=",", ndmin=2)[:, 0]
    assert frames.min() >= 5 and frames.max() <= 29 and 9 not in frames
    assert len(set(texts)) == len(texts)


def test_sweep_scores_match_evaluate_mot(torch, packed, loop):
    from boxmot_amd import evaluate_mot, mot_summary, tune

    gt = {f"seq{s}": TD.synthetic_gt(s) for s in range(S)}
    cfgs = BD.configs()
    host = tune.sweep_boost(packed, cfgs, gt=gt)
    dev = tune.sweep_boost(packed, cfgs, gt=gt, score="device")
    lean = tune.sweep_boost(packed, cfgs, gt=gt, score="device", keep_results=False)
    summaries = []
    for k in range(K):
        want = mot_summary(evaluate_mot(gt, loop / "reid" / f"{k:04d}"))
        assert host[k]["summary"] == want and dev[k]["summary"] == want, k
        assert lean[k]["summary"] == want and lean[k]["results"] is None, k
        assert all(dev[k]["results"][nm].tobytes() == host[k]["results"][nm].tobytes()
                   for nm in packed)
        assert want["HOTA"] > 1.0
        summaries.append(tuple(want.values()))
    assert len(set(summaries)) == K

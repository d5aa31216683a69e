"""boxmot_amd.tune.sweep_reid on the GPU: the files of a K-config sweep of DeepOCSort and HybridSort
against run_sequences(resident=True) once per config, byte for byte (DeepOCSort also under warps);
and the sweep's scores, on the device and on the host, against evaluate_mot of those files."""
import numpy as np
import pytest

from tests import sweep_reid_data as RD
from tests import tune_data as TD

pytestmark = pytest.mark.gpu

S, K = RD.S, RD.K
KINDS = ["deepocsort", "hybridsort"]


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

    d = tmp_path_factory.mktemp("reid_packed")
    out = {}
    for s in range(S):
        rows, embs = RD.packed_rows(RD.scene(s))
        out[f"seq{s}"] = motio.pack_arrays(rows, embs, d / f"seq{s}.bxmot")
    return out


def configs(kind):
    return [dict(c, **RD.CAPS) for c in RD.CONFIGS[kind]]


def _warps():
    """name -> the warp at every iterated frame: the frames that have detections."""
    out = {}
    for s in range(S):
        has = [bool(d.shape[0]) for d, _ in RD.scene(s)]
        out[f"seq{s}"] = RD.frame_warps(s)[has]
    return out


WARPS = _warps()


@pytest.fixture(scope="module")
def loop(torch, packed, tmp_path_factory):
    """The loop the sweep replaces: run_sequences(resident=True) once per config; root/<kind> and,
    for DeepOCSort under warps, root/warp."""
    from boxmot_amd import motio

    root = tmp_path_factory.mktemp("reid_loop")
    for kind in KINDS:
        for k, cfg in enumerate(configs(kind)):
            motio.run_sequences(kind, packed, root / kind / f"{k:04d}", tracker_kwargs=cfg,
                                resident=True)
    for k, cfg in enumerate(configs("deepocsort")):
        motio.run_sequences("deepocsort", packed, root / "warp" / f"{k:04d}", tracker_kwargs=cfg,
                            resident=True, warps=WARPS)
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

    res = tune.sweep_reid(kind, packed, configs(kind), exp_dir=tmp_path)
    assert [r["config"] for r in res] == configs(kind) and all(r["summary"] is None for r in res)
    texts = same_files(tmp_path, loop / kind, packed)
    assert len(set(texts)) == K * S  # the configs tell themselves apart on every sequence
    assert sorted(p.name for p in tmp_path.iterdir()) == ["0000", "0001", "0002"]
    for k in range(K):
        for nm in packed:
            rows = res[k]["results"][nm]
            file_rows = np.loadtxt(tmp_path / f"{k:04d}" / f"{nm}.txt", delimiter=",", ndmin=2)
            assert rows.dtype == np.float64 and rows.shape == file_rows.shape
            np.testing.assert_array_equal(rows[:, :8], file_rows[:, :8])


def test_sweep_with_warps_matches_run_sequences(torch, packed, loop, tmp_path):
    """Every config's copy of a sequence gets that sequence's warp; the warps change the rows."""
    from boxmot_amd import tune

    tune.sweep_reid("deepocsort", packed, configs("deepocsort"), exp_dir=tmp_path, warps=WARPS)
    texts = same_files(tmp_path, loop / "warp", packed)
    assert texts != same_files(loop / "deepocsort", loop / "deepocsort", packed)


def test_sweep_honours_frame_ids_and_sizes(torch, packed, tmp_path):
    from boxmot_amd import motio, tune

    fids = {"seq0": list(range(5, 30))}
    sizes = {"seq1": (1280, 720)}
    cfgs = [dict(c, asso_func="centroid") for c in configs("hybridsort")[:2]]
    tune.sweep_reid("hybridsort", packed, cfgs, exp_dir=tmp_path / "sweep", frame_ids=fids,
                    frame_sizes=sizes)
    for k, cfg in enumerate(cfgs):
        motio.run_sequences("hybridsort", packed, tmp_path / "loop" / f"{k:04d}", frame_ids=fids,
                            frame_sizes=sizes, tracker_kwargs=cfg, resident=True)
        for nm in packed:
            assert (tmp_path / "sweep" / f"{k:04d}" / f"{nm}.txt").read_bytes() == \
                (tmp_path / "loop" / f"{k:04d}" / f"{nm}.txt").read_bytes(), (k, nm)


@pytest.mark.parametrize("kind", KINDS)
def test_sweep_scores_match_evaluate_mot(torch, packed, loop, kind):
    from boxmot_amd import evaluate_mot, mot_summary, tune

    gt = {f"seq{s}": TD.synthetic_gt(s) for s in range(S)}
    host = tune.sweep_reid(kind, packed, configs(kind), gt=gt)
    dev = tune.sweep_reid(kind, packed, configs(kind), gt=gt, score="device")
    lean = tune.sweep_reid(kind, packed, configs(kind), gt=gt, score="device",
                           keep_results=False)
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

"""boxmot_amd.tune.sweep_strong on the GPU: the files of a K-config StrongSort sweep against
run_sequences once per config, byte for byte, with handle_occlusions off and on, with and without
warps, and over a frame range holding a frame without detections; and the sweep's scores on the
device and on the host against evaluate_mot of the files.  Tracks are born Confirmed
(GITHUB_ACTIONS=true, the fork's switch): born Tentative StrongSort writes no rows.  Every
case, occlusion on or off, runs the whole scene: sequence 1 goes through crowd mode, sequence 0
holds a pair the occlusion handler edits, and no pair makes it raise."""
import numpy as np
import pytest

from tests import sweep_strong_data as SD
from tests import tune_data as TD

pytestmark = pytest.mark.gpu

S, K = SD.S, SD.K


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    return t


@pytest.fixture(autouse=True)
def born_confirmed(monkeypatch):
    monkeypatch.setenv("GITHUB_ACTIONS", "true")
    monkeypatch.delenv("GITHUB_JOB", raising=False)


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    from boxmot_amd import motio

    d = tmp_path_factory.mktemp("ss_packed")
    out = {}
    for s in range(S):
        rows, embs = SD.packed_rows(SD.scene(s))
        out[f"seq{s}"] = motio.pack_arrays(rows, embs, d / f"seq{s}.bxmot")
    return out


def _warps():
    return {f"seq{s}": SD.warps(s)[[bool(d.shape[0]) for d, _ in SD.scene(s)]]
            for s in range(S)}


def loop(packed, root, cfgs, **kw):
    from boxmot_amd import motio

    for k, cfg in enumerate(cfgs):
        motio.run_sequences("strongsort", packed, root / f"{k:04d}", tracker_kwargs=cfg, **kw)


def same_files(got, want, names, n):
    texts = []
    for k in range(n):
        for nm in names:
            a = (got / f"{k:04d}" / f"{nm}.txt").read_bytes()
            assert a == (want / f"{k:04d}" / f"{nm}.txt").read_bytes(), (k, nm)
            assert len(a) > 500
            texts.append(a)
    return texts


@pytest.mark.parametrize("occ,warps", [(False, False), (False, True), (True, False),
                                       (True, True)])
def test_sweep_files_match_run_sequences(torch, packed, tmp_path, occ, warps):
    from boxmot_amd import tune

    seqs, cfgs = packed, SD.configs(occ)
    kw = dict(warps=_warps()) if warps else {}
    res = tune.sweep_strong(seqs, cfgs, exp_dir=tmp_path / "sweep", **kw)
    loop(seqs, tmp_path / "loop", cfgs, **kw)
    assert [r["config"] for r in res] == cfgs
    texts = same_files(tmp_path / "sweep", tmp_path / "loop", seqs, K)
    per_config = {tuple(texts[k * S: (k + 1) * S]) for k in range(K)}
    assert len(per_config) == K  # the configs tell themselves apart, crowd_detection included
    for k in range(K):  # the rows in memory are the files' rows
        for nm in seqs:
            f = np.loadtxt(tmp_path / "sweep" / f"{k:04d}" / f"{nm}.txt", delimiter=",", ndmin=2)
            np.testing.assert_array_equal(res[k]["results"][nm][:, :8], f[:, :8])


def test_occlusion_handler_edits_a_track(torch, packed, tmp_path):
    """With handle_occlusions the handler edits the occluded track of sequence 0's pair
    (tests/sweep_strong_data.py): every config's file of that sequence differs from the one
    without."""
    from boxmot_amd import tune

    seqs = packed
    tune.sweep_strong(seqs, SD.configs(True)[:2], exp_dir=tmp_path / "on")
    tune.sweep_strong(seqs, SD.configs(False)[:2], exp_dir=tmp_path / "off")
    for k in range(2):
        nm = f"seq{SD.PAIR_SEQ}"
        on = (tmp_path / "on" / f"{k:04d}" / f"{nm}.txt").read_bytes()
        off = (tmp_path / "off" / f"{k:04d}" / f"{nm}.txt").read_bytes()
        assert on != off, k


@pytest.mark.parametrize("occ", [False, True])
def test_frame_range_with_an_empty_frame(torch, packed, tmp_path, occ):
    from boxmot_amd import tune

    seqs, cfgs = packed, SD.configs(occ)[:3]
    es, et = TD.EMPTY
    fids = {f"seq{s}": list(range(5, 25)) for s in range(S)}
    assert fids[f"seq{es}"][0] < et < fids[f"seq{es}"][-1]
    tune.sweep_strong(seqs, cfgs, exp_dir=tmp_path / "sweep", frame_ids=fids)
    loop(seqs, tmp_path / "loop", cfgs, frame_ids=fids)
    same_files(tmp_path / "sweep", tmp_path / "loop", seqs, 3)


def test_scores_device_host_files(torch, packed, tmp_path):
    from boxmot_amd import evaluate_mot, mot_summary, tune

    seqs, cfgs = packed, SD.configs(False)
    gt = {f"seq{s}": TD.synthetic_gt(s) for s in range(S)}
    host = tune.sweep_strong(seqs, cfgs, exp_dir=tmp_path, gt=gt)
    dev = tune.sweep_strong(seqs, cfgs, gt=gt, score="device")
    lean = tune.sweep_strong(seqs, cfgs, gt=gt, score="device", keep_results=False)
    for k in range(K):
        want = mot_summary(evaluate_mot(gt, tmp_path / f"{k:04d}"))
        assert host[k]["summary"] == want and dev[k]["summary"] == want, k
        assert lean[k]["summary"] == want and lean[k]["results"] is None, k
        assert all(dev[k]["results"][nm].tobytes() == host[k]["results"][nm].tobytes()
                   for nm in seqs)
        assert want["HOTA"] > 1.0
    with pytest.raises(ValueError):
        tune.sweep_strong(seqs, SD.configs(True), gt=gt, score="device")

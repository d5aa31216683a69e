"""The many-sequence flows with StrongSort's occlusion handling on the device:
run_sequences, sweep_strong_device and sweep_gsi with ``occlusion="device"`` against the same
flows with the host handler, byte for byte, on the scenes of tests/sweep_strong_data.py."""
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

    d = tmp_path_factory.mktemp("ss_occ_packed")
    out = {}
    for s in range(S):
        rows, embs = SD.packed_rows(SD.scene(s))
        out[f"seq{s}"] = motio.pack_arrays(rows, embs, d / f"seq{s}.bxmot")
    return out


def _warps():
    return {f"seq{s}": SD.warps(s)[[bool(d.shape[0]) for d, _ in SD.scene(s)]]
            for s in range(S)}


def same_dir(a, b, names, min_len=500):
    for nm in names:
        x = (a / f"{nm}.txt").read_bytes()
        assert x == (b / f"{nm}.txt").read_bytes(), nm
        assert len(x) > min_len


@pytest.mark.parametrize("case", ["plain", "warps", "empty_frame"])
def test_run_sequences_device_equals_host(torch, packed, tmp_path, case):
    from boxmot_amd import motio

    cfg = SD.configs(True)[0]
    kw = {}
    if case == "warps":
        kw["warps"] = _warps()
    if case == "empty_frame":
        es, et = TD.EMPTY
        kw["frame_ids"] = {f"seq{s}": list(range(5, 25)) for s in range(S)}
        assert kw["frame_ids"][f"seq{es}"][0] < et < kw["frame_ids"][f"seq{es}"][-1]
    motio.run_sequences("strongsort", packed, tmp_path / "host", tracker_kwargs=cfg, **kw)
    motio.run_sequences("strongsort", packed, tmp_path / "dev", tracker_kwargs=cfg,
                        occlusion="device", **kw)
    same_dir(tmp_path / "dev", tmp_path / "host", packed)
    if case == "plain":  # the pass edits: the pair's sequence differs from the run without it
        motio.run_sequences("strongsort", packed, tmp_path / "off",
                            tracker_kwargs=dict(cfg, handle_occlusions=False),
                            occlusion="device")  # (ignored: no pass)
        nm = f"seq{SD.PAIR_SEQ}"
        assert (tmp_path / "off" / f"{nm}.txt").read_bytes() != \
            (tmp_path / "dev" / f"{nm}.txt").read_bytes()


def test_sweep_device_equals_host_and_scores(torch, packed, tmp_path):
    from boxmot_amd import tune

    cfgs = SD.configs(True)
    gt = {f"seq{s}": TD.synthetic_gt(s) for s in range(S)}
    host = tune.sweep_strong(packed, cfgs, exp_dir=tmp_path / "host", gt=gt)
    dev = tune.sweep_strong_device(packed, cfgs, exp_dir=tmp_path / "dev", gt=gt)
    lean = tune.sweep_strong_device(packed, cfgs, gt=gt, score="device", keep_results=False)
    for k in range(K):
        same_dir(tmp_path / "dev" / f"{k:04d}", tmp_path / "host" / f"{k:04d}", packed)
        assert dev[k]["summary"] == host[k]["summary"], k
        assert lean[k]["summary"] == host[k]["summary"] and lean[k]["results"] is None, k


def test_sweep_mixes_handle_occlusions(torch, packed, tmp_path):
    from boxmot_amd import motio, tune

    cfgs = [SD.configs(True)[0], SD.configs(False)[1], SD.configs(True)[2]]
    tune.sweep_strong_device(packed, cfgs, exp_dir=tmp_path / "sweep")
    for k, cfg in enumerate(cfgs):
        motio.run_sequences("strongsort", packed, tmp_path / "loop" / f"{k:04d}",
                            tracker_kwargs=cfg)
        same_dir(tmp_path / "sweep" / f"{k:04d}", tmp_path / "loop" / f"{k:04d}", packed)


def test_sweep_gsi_device(torch, packed, tmp_path):
    from boxmot_amd import postprocessing, tune

    cfgs = SD.configs(True)[:2]
    gt = {f"seq{s}": TD.synthetic_gt(s) for s in range(S)}
    got = tune.sweep_gsi("strongsort", packed, cfgs, exp_dir=tmp_path / "dev", gt=gt,
                         occlusion="device", score="device")
    want = tune.sweep_gsi("strongsort", packed, cfgs, gt=gt)
    tune.sweep_strong(packed, cfgs, exp_dir=tmp_path / "host")
    for k in range(2):
        # gsi() globs MOT*.txt: the plain files under such names
        d = tmp_path / "gsi" / f"{k:04d}"
        d.mkdir(parents=True)
        for nm in packed:
            (d / f"MOT-{nm}.txt").write_bytes((tmp_path / "host" / f"{k:04d}" / f"{nm}.txt")
                                              .read_bytes())
        postprocessing.gsi(d)
        for nm in packed:
            assert (tmp_path / "dev" / f"{k:04d}" / f"{nm}.txt").read_bytes() == \
                (d / f"MOT-{nm}.txt").read_bytes(), (k, nm)
        assert got[k]["summary"] == want[k]["summary"], k


def test_mutual_occlusion_raises_and_writes_nothing(torch, tmp_path):
    """Two equal boxes near the corner: the reference's TypeError at their first update."""
    from boxmot_amd import motio

    rng = np.random.default_rng(5)
    rows, embs = [], []
    for t in range(1, 4):
        for tl, wh in (((10.0, 10.0), 300.0), ((20.0, 20.0), 310.0)):  # equal areas as corners
            rows.append([t, tl[0], tl[1], tl[0] + wh, tl[1] + wh, 0.9, 0])
        embs.append(np.eye(2, SD.F) + 0.01 * rng.standard_normal((2, SD.F)))
    seq = {"mutual": motio.pack_arrays(np.array(rows), np.concatenate(embs),
                                       tmp_path / "mutual.bxmot")}
    with pytest.raises(TypeError, match="not iterable"):
        motio.run_sequences("strongsort", seq, tmp_path / "host", tracker_kwargs=dict(SD.CAPS))
    with pytest.raises(TypeError, match=r"not iterable.*mutual.*update 1"):
        motio.run_sequences("strongsort", seq, tmp_path / "dev", tracker_kwargs=dict(SD.CAPS),
                            occlusion="device")
    assert not (tmp_path / "host").exists() and not (tmp_path / "dev").exists()

"""boxmot_amd.tune.sweep scoring from device memory (score="device"): the K configs' summaries
from ONE evaluator run of K groups over the feeder's result buffers (SequenceFeeder.results_device,
MotEvaluator.set_gt / run_device) equal the host-row path's and evaluate_mot's, exactly; with
keep_results=False the rows are never copied to the host."""
import pytest

from tests import tune_data as TD

pytestmark = pytest.mark.gpu

S, K = TD.S, TD.K


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

    d = tmp_path_factory.mktemp("tune_device_packed")
    return {f"seq{s}": motio.pack_arrays(TD.packed_rows(TD.scene_frames(s)), None,
                                         d / f"seq{s}.bxmot") for s in range(S)}


def test_sweep_device_scores_equal_host_scores(torch, packed, tmp_path):
    from boxmot_amd import evaluate_mot, mot_summary, tune

    gt = {f"seq{s}": TD.synthetic_gt(s) for s in range(S)}
    host = tune.sweep("ocsort", packed, TD.CONFIGS, gt=gt, score="host", exp_dir=tmp_path)
    dev = tune.sweep("ocsort", packed, TD.CONFIGS, gt=gt, score="device")
    lean = tune.sweep("ocsort", packed, TD.CONFIGS, gt=gt, score="device", keep_results=False)
    summaries = set()
    for k in range(K):
        want = mot_summary(evaluate_mot(gt, tmp_path / f"{k:04d}"))
        assert host[k]["summary"] == want and want["HOTA"] > 5.0, k
        assert dev[k]["summary"] == want, k
        assert lean[k]["summary"] == want and lean[k]["results"] is None, k
        assert lean[k]["config"] == TD.CONFIGS[k]
        for nm in packed:
            assert dev[k]["results"][nm].tobytes() == host[k]["results"][nm].tobytes()
        summaries.add(tuple(want.values()))
    assert len(summaries) == K


"""boxmot_amd.tune.sweep_gsi on the GPU: the sweep with GSI applied before the rows are scored,
returned or written, against the flow it replaces (the plain sweep's files, ``boxmot_amd.gsi`` on
every config's folder, ``evaluate_mot`` per config).

The scenes are those of tests/tune_data.py (two sequences of 40 and 33 frames, object 2 undetected
in frames 14-18, three configs), under names that begin with ``MOT`` because ``gsi`` globs
``MOT*.txt``.  A tracker that keeps object 2's id through the gap leaves a gap of 6 frames in its
rows, below the interval of 20, so GSI inserts rows: the comparison is not one of equal inputs.
"""
import numpy as np
import pytest

from tests import sweep_bot_data as BD
from tests import sweep_reid_data as RD
from tests import tune_data as TD

pytestmark = pytest.mark.gpu

S, K = TD.S, TD.K
NAMES = [f"MOT17-{s:02d}" for s in range(S)]
INTERVAL, TAU = 20, 10
KINDS = ("ocsort", "bytetrack", "deepocsort")


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return t


@pytest.fixture(scope="module")
def gt():
    return {nm: TD.synthetic_gt(s) for s, nm in enumerate(NAMES)}


def configs(kind):
    if kind == "ocsort":
        return TD.CONFIGS
    if kind == "bytetrack":
        return BD.configs(kind)
    return [dict(c, **RD.CAPS) for c in RD.CONFIGS[kind]]


def plain_sweep(kind, packed, **kw):
    from boxmot_amd import tune

    if kind == "ocsort":
        return tune.sweep(kind, packed, configs(kind), **kw)
    if kind == "bytetrack":
        return tune.sweep_bot(kind, packed, configs(kind), **kw)
    return tune.sweep_reid(kind, packed, configs(kind), **kw)


@pytest.fixture(scope="module")
def flows(torch, gt, tmp_path_factory):
    """Per tracker, computed once: the packed sequences, folder ``b`` (plain sweep, then gsi on
    every config's folder) with the plain rows, and the three sweep_gsi runs (``a`` holds the
    files of the first)."""
    import boxmot_amd
    from boxmot_amd import motio, tune

    out = {}
    for kind in KINDS:
        d = tmp_path_factory.mktemp(f"gsi_{kind}")
        packed = {}
        for s, nm in enumerate(NAMES):
            if kind == "ocsort":
                rows, embs = TD.packed_rows(TD.scene_frames(s)), None
            else:
                rows, embs = RD.packed_rows(BD.scene(s))
            packed[nm] = motio.pack_arrays(rows, embs, d / f"{nm}.bxmot")
        a, b = d / "a", d / "b"
        plain = plain_sweep(kind, packed, exp_dir=b)
        for k in range(K):
            boxmot_amd.gsi(b / f"{k:04d}", INTERVAL, TAU)
        kw = dict(interval=INTERVAL, tau=TAU, gt=gt)
        out[kind] = dict(
            a=a, b=b, plain=plain,
            host=tune.sweep_gsi(kind, packed, configs(kind), exp_dir=a, **kw),
            dev=tune.sweep_gsi(kind, packed, configs(kind), score="device", **kw),
            lean=tune.sweep_gsi(kind, packed, configs(kind), score="device", keep_results=False,
                                **kw))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_files_match_sweep_then_gsi(flows, kind):
    f = flows[kind]
    grew = 0
    for k in range(K):
        for nm in NAMES:
            got = (f["a"] / f"{k:04d}" / f"{nm}.txt").read_bytes()
            want = (f["b"] / f"{k:04d}" / f"{nm}.txt").read_bytes()
            assert got == want, (k, nm)
            assert len(got) > 500 and b"," not in got
            grew += len(got.splitlines()) > f["plain"][k]["results"][nm].shape[0]
    print(kind, "files with inserted rows:", grew, "of", K * S)
    assert grew >= 1  # GSI changed something: the gap of object 2 was filled


@pytest.mark.parametrize("kind", KINDS)
def test_results_are_the_files_values(flows, kind):
    f = flows[kind]
    for k in range(K):
        for run in ("host", "dev"):
            assert f[run][k]["config"] == configs(kind)[k]
            for nm in NAMES:
                rows = f[run][k]["results"][nm]
                want = np.loadtxt(f["b"] / f"{k:04d}" / f"{nm}.txt", ndmin=2)
                assert rows.dtype == np.float64 and rows.shape == want.shape == (len(want), 9)
                assert np.array_equal(rows.view(np.uint64), want.view(np.uint64)), (run, k, nm)
        assert f["lean"][k]["results"] is None


def test_post_stage_for_rows_formed_on_the_host(flows):
    """What a StrongSort sweep with handle_occlusions hands the post-stage: host rows per engine
    sequence, one of them empty; the same values as gsi_batch and the "%d" truncation."""
    from boxmot_amd import tune
    from boxmot_amd.postprocessing import gsi_batch

    res = flows["ocsort"]["plain"][0]["results"]
    rows = [res[NAMES[0]], np.empty((0, 9)), res[NAMES[1]]]
    got = tune._gsi_host_rows(rows, (INTERVAL, float(TAU)))
    want = [np.trunc(x) + 0.0 for x in gsi_batch(rows, INTERVAL, TAU)]
    assert [g.shape for g in got] == [w.shape for w in want] and got[1].shape == (0, 9)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64))


@pytest.mark.parametrize("kind", KINDS)
def test_scores_match_evaluate_mot(flows, gt, kind):
    from boxmot_amd import evaluate_mot, mot_summary

    f = flows[kind]
    summaries = []
    for k in range(K):
        want = mot_summary(evaluate_mot(gt, f["b"] / f"{k:04d}"))
        assert f["host"][k]["summary"] == want, k
        assert f["dev"][k]["summary"] == want and f["lean"][k]["summary"] == want, k
        summaries.append(repr(want))
    plain = [repr(mot_summary(evaluate_mot(gt, {nm: r for nm, r in p["results"].items()})))
             for p in f["plain"]]
    print(kind, "configs whose summary GSI changed:",
          sum(a != b for a, b in zip(summaries, plain)), "of", K)
    assert summaries != plain

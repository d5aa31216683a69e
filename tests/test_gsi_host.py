"""CPU-side checks of the GSI post-processing surface: names, signatures, fixtures, argument
validation, and that run_sequences only reaches it when asked to."""
import inspect
from pathlib import Path

import numpy as np
import pytest

from boxmot_amd import gaussian_smooth, gsi, linear_interpolation
from boxmot_amd import motio, postprocessing

GOLDEN = Path(__file__).resolve().parent / "golden"
NAMES = ["tiny", "gaps", "mixed", "long", "unsorted"]


def test_names_are_the_package_surface():
    import boxmot_amd

    for n in ("gsi", "linear_interpolation", "gaussian_smooth"):
        assert n in boxmot_amd.__all__ and getattr(boxmot_amd, n) is getattr(postprocessing, n)


def test_signatures_match_the_reference():
    # boxmot/postprocessing/gsi.py:13, :57, :115
    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert sig(linear_interpolation) == [("data", E), ("interval", E)]
    assert sig(gaussian_smooth) == [("data", E), ("tau", E)]
    assert sig(gsi) == [("mot_results_folder", E), ("interval", 20), ("tau", 10)]
    rs = inspect.signature(motio.run_sequences).parameters
    assert (rs["gsi"].default, rs["gsi_interval"].default, rs["gsi_tau"].default) == (False, 20, 10)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_keys_and_shapes(name):
    z = np.load(GOLDEN / f"gsi_{name}.npz")
    assert sorted(z.files) == ["input", "interpolated", "interval", "smoothed", "solver_spread",
                               "tau"]
    inp, itp, sm = z["input"], z["interpolated"], z["smoothed"]
    assert inp.dtype == itp.dtype == sm.dtype == np.float64
    assert inp.ndim == 2 and inp.shape[1] >= 8 and itp.shape[1] == inp.shape[1]
    assert itp.shape[0] >= inp.shape[0] and sm.shape == (itp.shape[0], 9)
    assert int(z["interval"]) == 20 and float(z["tau"]) == 10
    assert 0 < float(z["solver_spread"]) < 1e-3
    # the reference's output order: ids ascending, frames ascending within an id
    assert np.array_equal(np.lexsort((itp[:, 0], itp[:, 1])), np.arange(itp.shape[0]))
    assert np.array_equal(sm[:, :2], itp[:, :2]) and np.all(sm[:, 8] == -1)


@pytest.mark.parametrize("name,tau,ncol", [("tiles", 10, 8), ("deep", 15, 8), ("wide", 10, 10)])
def test_more_fixture_keys_and_shapes(name, tau, ncol):
    z = np.load(GOLDEN / f"gsi_{name}.npz")
    assert sorted(z.files) == ["input", "interpolated", "interval", "smoothed", "solver_spread",
                               "tau"]
    inp, itp, sm = z["input"], z["interpolated"], z["smoothed"]
    assert inp.dtype == itp.dtype == sm.dtype == np.float64
    assert inp.shape[1] == itp.shape[1] == ncol
    assert itp.shape[0] > inp.shape[0] and sm.shape == (itp.shape[0], 9)
    assert int(z["interval"]) == 20 and float(z["tau"]) == tau
    assert 0 < 4 * float(z["solver_spread"]) < 1e-3  # the bound is the spread's, not the cap
    assert np.array_equal(np.lexsort((itp[:, 0], itp[:, 1])), np.arange(itp.shape[0]))
    assert np.array_equal(sm[:, [0, 1, 6, 7]], itp[:, [0, 1, 6, 7]]) and np.all(sm[:, 8] == -1)
    lens = np.unique(itp[:, 1], return_counts=True)[1].tolist()
    if name == "tiles":
        assert lens == [15, 16, 17, 34, 93, 94, 95, 96, 97, 127, 128, 129, 159, 160, 161, 207,
                        208, 209, 223, 224, 225]
    elif name == "deep":
        assert lens == [1201, 2049]
        # the smoothing does real work on both (on `long`'s 1200 rows it moves boxes by 6e-8 px)
        for i in (1, 2):
            assert np.abs(sm[sm[:, 1] == i][:, 2:6] - itp[itp[:, 1] == i][:, 2:6]).max() > 1.0
        lg = np.load(GOLDEN / "gsi_long.npz")
        m = lg["smoothed"][:, 1] == 1
        assert m.sum() == 1200
        assert np.abs(lg["smoothed"][m][:, 2:6] - lg["interpolated"][m][:, 2:6]).max() < 1e-6


def test_params_and_rows_fixtures():
    p = np.load(GOLDEN / "gsi_params.npz")
    assert len(p.files) == 18
    for k, (interval, tau) in enumerate([(2, 2), (5, 3), (50, 10)]):
        assert (int(p[f"interval_{k}"]), float(p[f"tau_{k}"])) == (interval, tau)
        assert p[f"smoothed_{k}"].shape == (p[f"interpolated_{k}"].shape[0], 9)
        assert 0 < 4 * float(p[f"solver_spread_{k}"]) < 1e-3
    assert p["interpolated_0"].shape == p["input_0"].shape
    assert p["interpolated_1"].shape[0] == p["input_1"].shape[0] + 6
    assert p["interpolated_2"].shape[0] == p["input_2"].shape[0] + 48
    r = np.load(GOLDEN / "gsi_rows.npz")
    assert len(r.files) == 18 and not any(f.startswith("smoothed") for f in r.files)
    assert [r[f"input_{k}"].shape[0] for k in range(5)] == [1, 1023, 1024, 1025, 2048]
    d = r["input_5"]
    assert np.unique(d[:, :2], axis=0).shape[0] < d.shape[0]  # duplicate (frame, id) rows


def test_gsi_leaves_an_empty_file_untouched(tmp_path):
    f = tmp_path / "MOT17-02.txt"
    f.write_text("")
    other = tmp_path / "notes.txt"
    other.write_text("1,2,3\n")
    gsi(tmp_path)  # nothing to process: never reaches the device
    assert f.read_text() == "" and other.read_text() == "1,2,3\n"


@pytest.mark.parametrize("fn,arg", [(linear_interpolation, 20), (gaussian_smooth, 10)])
@pytest.mark.parametrize("bad", [np.zeros((4, 7)), np.zeros(8), np.zeros((2, 3, 8))],
                         ids=["7cols", "1d", "3d"])
def test_bad_shapes_raise(fn, arg, bad):
    with pytest.raises(ValueError):
        fn(bad, arg)


def test_batch_rejects_bad_shapes_before_the_device():
    with pytest.raises(ValueError):
        postprocessing.gsi_batch([np.zeros((3, 8)), np.zeros((3, 5))], 20, 10)


class Probe:
    """Stands in for the batched engine: no sequences, so no frame is ever stepped."""

    def status(self):
        return 0


def test_run_sequences_reaches_gsi_only_when_asked(monkeypatch, tmp_path):
    calls = []
    monkeypatch.setattr(motio, "_batched_engine", lambda *a, **k: (Probe(), np.float32, 8))
    monkeypatch.setattr(postprocessing, "gsi", lambda *a, **k: calls.append((a, k)))
    for entry in ("_interpolate_device", "_smooth_device", "gsi_batch"):
        monkeypatch.setattr(postprocessing, entry,
                            lambda *a, **k: pytest.fail("native GSI entry point reached"))
    assert motio.run_sequences("bytetrack", {}, tmp_path) == {}
    assert motio.run_sequences("bytetrack", {}, tmp_path, gsi=False) == {}
    assert calls == []
    motio.run_sequences("bytetrack", {}, tmp_path, gsi=True, gsi_interval=7, gsi_tau=3)
    assert calls == [((tmp_path,), {"interval": 7, "tau": 3})]

"""HybridSort's camera-motion compensation without a GPU: the new entry points and their
bindings, the drop-in's keyword, attribute and lazy estimator, and the refusals of the flows."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from boxmot_amd import HybridSort, HybridSortPerClass, motio, tune
from boxmot_amd import _native as N
from boxmot_amd import engine as E
from tests.hybcmc_util import camera_update

ROOT = Path(__file__).resolve().parents[1]
NEW = ["bx_hybrid_set_ecc_host", "bx_hybrid_ecc_host", "bx_hybrid_step_cmc",
       "bx_hybrid_update_host_cmc", "bx_hybrid_step_classes_cmc",
       "bx_hybrid_update_classes_host_cmc"]


def test_entry_points_are_declared_bound_and_exported():
    header = (ROOT / "include" / "bxhybridsort.h").read_text()
    lib = N.build()
    import ctypes

    dll = ctypes.CDLL(str(lib))
    for s in NEW:
        assert re.search(rf"\bint {s}\(", header), s
        assert s in N.EXPORTS and getattr(dll, s)
    # the existing step is untouched and the new one is its signature plus the warps
    sig = lambda name: re.search(rf"int {name}\((.*?)\);", header, re.S).group(1).split(",")
    old, new = sig("bx_hybrid_step"), sig("bx_hybrid_step_cmc")
    assert len(new) == len(old) + 1 and "const double *warps" in " ".join(new[6].split())


def test_engine_classes():
    assert issubclass(E.HybridsortCmcEngine, E.HybridsortEngine)
    assert issubclass(E.HybridsortCmcTableEngine, E.HybridsortCmcEngine)
    for cls in (E.HybridsortCmcEngine, E.HybridsortCmcTableEngine):
        assert "warps" in inspect.signature(cls.step).parameters
        assert inspect.signature(cls.step).parameters["warps"].default is None
        assert list(inspect.signature(cls.set_ecc).parameters)[:3] == ["self", "seq0", "flags"]
    assert E.HybridsortCmcParams().ECC is False and not hasattr(E.HybridsortParams(), "ECC")


def make(cls=HybridSort, **kw):
    return cls(reid_weights=None, device=None, half=False, det_thresh=0.3, **kw)


def test_attribute_keyword_and_lazy_cmc():
    """ECC is the reference's plain attribute; HybridSort's constructor signature is pinned to the
    reference's (tests/test_hybridsort_host.py), so only HybridSortPerClass, which takes
    **kwargs, has it as a keyword too."""
    tr = make()
    assert tr.ECC is False and tr._cmc is None
    tr.ECC = True
    assert tr.ECC is True and tr._cmc is None  # nothing built yet
    sentinel = object()
    tr.cmc = sentinel
    assert tr.cmc is sentinel
    pc = make(HybridSortPerClass, nr_classes=3, ECC=True)
    assert pc.ECC is True and pc._cmc is None
    eng = motio._batched_engine  # ECC in tracker_kwargs never reaches HybridSort's constructor
    assert "ECC" not in inspect.signature(HybridSort.__init__).parameters and callable(eng)


def test_default_cmc_is_ecc():
    """ECC's constructor touches no device (its handle is built at the first apply)."""
    from boxmot_amd import ECC

    tr = make()
    tr.ECC = True
    got = tr.cmc
    assert isinstance(got, ECC) and tr.cmc is got


def test_warp_trackers_unchanged():
    assert motio.WARP_TRACKERS == ("botsort", "boosttrack", "strongsort", "deepocsort")


def test_refusals(tmp_path):
    w = {"a": np.zeros((3, 6))}
    chk = motio._check_warp_args
    with pytest.raises(ValueError, match="hybridsort takes no camera-motion warp"):
        chk("hybridsort", {}, 0, w, None, None)
    with pytest.raises(ValueError, match="hybridsort takes no camera-motion warp"):
        chk("hybridsort", {"ECC": False}, 0, w, None, None)
    assert chk("hybridsort", {"ECC": True}, 0, w, None, None) is None
    assert chk("hybridsort", {"ECC": True}, 0, None, {"a": None}, "ecc") == {}
    with pytest.raises(ValueError, match="per_class run"):
        chk("hybridsort", {"ECC": True}, 3, w, None, None)
    with pytest.raises(ValueError, match="hybridsort takes no camera-motion warp"):
        motio.run_sequences("hybridsort", {}, tmp_path / "x", warps=w)
    with pytest.raises(ValueError, match="hybridsort takes no camera-motion warp"):
        tune._check_reid("hybridsort", [{}, {"ECC": False}], w, "host", True)
    tune._check_reid("hybridsort", [{}, {"ECC": True}], w, "host", True)
    with pytest.raises(ValueError, match="per_class run"):
        motio.run_sequences("hybridsort", {}, tmp_path / "x", warps=w, n_classes=2,
                            tracker_kwargs={"ECC": True})
    assert not list(tmp_path.iterdir())


def test_warp_table_of_the_wrong_shape(tmp_path):
    rows = np.array([[1, 10, 10, 50, 90, 0.9, 0], [2, 11, 10, 51, 90, 0.9, 0]], np.float64)
    e = np.eye(2, 4)
    p = motio.pack_arrays(rows, e, tmp_path / "a.bxmot")
    seq = motio.BinSequence(p)
    with pytest.raises(ValueError, match="warps of shape"):
        motio._flow_warps(["a"], [seq], [seq.frame_ids], 4, {"a": np.zeros((5, 6))}, None, None)


def test_restatement_round_trip_is_not_the_identity():
    """The state -> corner box -> state round trip under the identity changes bits."""
    rng = np.random.default_rng(0)
    x = np.zeros((200, 9))
    x[:, 0], x[:, 1] = rng.uniform(0, 1900, 200), rng.uniform(0, 1000, 200)
    x[:, 2], x[:, 3], x[:, 4] = rng.uniform(500, 9000, 200), rng.uniform(0.3, 1, 200), \
        rng.uniform(0.3, 0.9, 200)
    y, skipped = camera_update(x, np.eye(2, 3))
    assert skipped == 0 and np.abs(y - x).max() < 1e-6 and not np.array_equal(x, y)
    assert np.array_equal(y[:, 3], x[:, 3]) and np.array_equal(y[:, 5:], x[:, 5:])
    x[7, 3] = 0.0
    y, skipped = camera_update(x, np.eye(2, 3))
    assert skipped == 1 and np.array_equal(y[7], x[7])


GOLDEN = ROOT / "tests" / "golden"


@pytest.mark.parametrize("name", ["crowd40", "noisy40", "identity"])
def test_restatement_is_the_reference_bit_for_bit(name):
    """The fixtures hold kf.x of every track right before and right after the reference's
    camera_update of their last frame: the restatement (and with it the summation order
    fma(m0, x, m1 * y) + m2, which the GPU edge test holds the kernel to byte for byte) gives the
    reference's bytes, and the unfused order does not."""
    with np.load(GOLDEN / f"hybcmc_{name}.npz") as fx:
        before, after, w = fx["cam_before"], fx["cam_after"], fx["warps"][-1]
    assert before.shape == after.shape and before.shape[0] >= 20 and before.shape[1] == 9
    got, skipped = camera_update(before, w)
    assert skipped == 0 and got.tobytes() == after.tobytes()
    assert before.tobytes() != after.tobytes()  # (the identity warp's round trip included)
    if name != "identity":
        import tests.hybcmc_util as U

        fused = U.fma
        U.fma = lambda a, b, c: a * b + c  # (m0 x + m1 y) + m2, each rounded
        try:
            assert camera_update(before, w)[0].tobytes() != after.tobytes()
        finally:
            U.fma = fused

"""CPU checks of the device occlusion pass's boundary: the CPython set order the
kernel restates (bx_pyset_order_host against real sets), the refusals of the ``occlusion=``
argument, raised before any engine is built, and the new symbols."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def pyset_order(adds):
    from boxmot_amd import _native as N

    a = np.ascontiguousarray(adds, np.int64)
    out = np.zeros(max(a.size, 1), np.int64)
    n = C.c_int()
    N.check(N.load().bx_pyset_order_host(a.ctypes.data, int(a.size), out.ctypes.data,
                                         C.byref(n)), "bx_pyset_order_host")
    return out[: n.value].tolist()


def real_order(adds):
    s = set()
    for x in adds:
        s.add(int(x))
    return list(s)


def test_pyset_order_matches_cpython_random():
    """Lengths 1-40, ids up to 5000: tests/test_oracle.py::test_pyset_order_matches_cpython's
    ranges, 4000 seeded lists (duplicates included)."""
    rng = np.random.default_rng(20261021)
    for _ in range(4000):
        adds = rng.integers(1, 5001, int(rng.integers(1, 41)))
        assert pyset_order(adds) == real_order(adds), adds.tolist()


@pytest.mark.parametrize("adds", [
    [6, 7, 8],                         # one table of 8: 8 wraps to slot 0
    [1, 2, 3, 4, 5],                   # the fifth key grows 8 -> 32
    [8, 16, 24, 32, 40, 48],           # collisions in slot 0 across the 8 -> 32 growth
    list(range(3, 22)),                # 19 keys: 32 -> 128
    [32 * k + 1 for k in range(1, 25)],  # one slot's chain across 32 -> 128 (perturbation)
    list(range(1, 80)),                # 128 -> 512
    list(range(1023, 0, -1)),          # a full track list's worth: up to 2048 slots
    [7, 7, 7, 3, 3, 7],                # duplicates only
    [0, 8, 16],                        # key 0 is a key, not an empty slot
])
def test_pyset_order_hand_cases(adds):
    assert pyset_order(adds) == real_order(adds)


def test_pyset_order_empty_and_negative():
    assert pyset_order([]) == []
    with pytest.raises(ValueError):
        pyset_order([3, -1])


def test_occlusion_argument_refusals(tmp_path):
    """Raised by the argument check, before sequences are opened or an engine is built: the
    sequences here are paths that do not exist."""
    from boxmot_amd import motio, tune

    seqs = {"nowhere": tmp_path / "missing.bin"}
    for kind in ("bytetrack", "botsort", "ocsort", "boosttrack", "deepocsort", "hybridsort"):
        with pytest.raises(ValueError, match="occlusion"):
            motio.run_sequences(kind, seqs, tmp_path, occlusion="device")
    for bad in ("gpu", "", None, True):
        with pytest.raises(ValueError, match="occlusion"):
            motio.run_sequences("strongsort", seqs, tmp_path, occlusion=bad)
        with pytest.raises(ValueError, match="occlusion"):
            tune.sweep_strong_device(seqs, [dict()], occlusion=bad)
    with pytest.raises(ValueError, match="occlusion"):
        tune.sweep_gsi("strongsort", seqs, [dict()], occlusion="nowhere")
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("configs, kw", [
    ([dict(handle_occlusions=False), dict()], {}),       # mixed handle_occlusions
    ([dict()], dict(score="device", gt={})),              # device scores of host-edited rows
    ([dict()], dict(keep_results=False, gt={}, score="device")),
    ([dict(handle_occlusions=True)], dict(keep_results=False)),
])
def test_host_sweep_keeps_its_refusals(tmp_path, configs, kw):
    """``occlusion="host"`` (the default, and spelled out) refuses what it refused."""
    from boxmot_amd import tune

    seqs = {"nowhere": tmp_path / "missing.bin"}
    with pytest.raises(ValueError):
        tune.sweep_strong(seqs, configs, **kw)
    with pytest.raises(ValueError):
        tune.sweep_strong_device(seqs, configs, occlusion="host", **kw)


def test_symbols_and_methods():
    from boxmot_amd import _native as N
    from boxmot_amd import engine, motio, tune
    import inspect

    text = (ROOT / "include" / "bxstrongsort.h").read_text()
    names = ("bx_ss_set_occlusion_host", "bx_ss_occlusion_host", "bx_ss_occlusion_buffer_host",
             "bx_pyset_order_host")
    for name in names:
        assert re.search(rf"^int {name}\(", text, re.M) and name in N.EXPORTS and name in N._SIGS
    nm = subprocess.run(["nm", "-D", "--defined-only", str(N.build())], capture_output=True,
                        text=True, check=True).stdout
    for name in names:
        assert re.search(rf"\bT {name}$", nm, re.M), name
    assert "bx_strongsort_occ.hip" in N.SOURCES
    for m in ("set_occlusion", "occlusion", "occlusion_buffer", "grown"):
        assert callable(getattr(engine.SsTableEngine, m))
    assert inspect.signature(motio.run_sequences).parameters["occlusion"].default == "host"
    assert inspect.signature(tune.sweep_strong_device).parameters["occlusion"].default == "device"

"""Chained ECC and the warps of the file flow, host side, no GPU: the ABI is declared, bound and
exported, the chunk plan is a pure function, and run_sequences refuses what it cannot do before
any engine or table is built."""
import inspect
import re
import subprocess

import numpy as np
import pytest

import boxmot_amd
from boxmot_amd import _native as N
from boxmot_amd import cmc, motio

NEW = ("bx_ecc_chain_reserve", "bx_ecc_apply_chain", "bx_ecc_apply_chain_host")


def test_symbols_declared_bound_and_exported():
    text = N.HEADER_CMC.read_text()
    for s in NEW:
        assert re.search(rf"^int {s}\(", text, re.M), s
        assert s in N.EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", str(N.build())], capture_output=True,
                        text=True, check=True).stdout
    assert set(NEW) <= set(re.findall(r"\bT (bx_\w+)$", nm, re.M))
    L = N.load()
    # the header's argument lists: 17 and 16 arguments, dst the only int64 pointer
    assert len(L.bx_ecc_apply_chain.argtypes) == 17 and len(L.bx_ecc_chain_reserve.argtypes) == 2
    assert len(L.bx_ecc_apply_chain_host.argtypes) == 16
    decl = re.search(r"int bx_ecc_apply_chain\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == 17 and "const int64_t *dst" in decl
    decl = re.search(r"int bx_ecc_apply_chain_host\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == 16 and "dst" not in decl and "init" not in decl


def test_python_surface():
    for name in ("EccChain", "warp_table"):
        assert name in boxmot_amd.__all__ and getattr(boxmot_amd, name) is getattr(cmc, name)
    p = inspect.signature(cmc.warp_table).parameters
    assert [k for k, v in p.items() if v.kind is v.KEYWORD_ONLY] == \
        ["warp_mode", "eps", "max_iter", "scale", "chunk"]
    ecc = inspect.signature(cmc.ECC.__init__).parameters
    for k in ("warp_mode", "eps", "max_iter", "scale"):  # ECC()'s defaults
        assert p[k].default == ecc[k].default
    assert p["chunk"].default == 64 and cmc.NOT_STEPPED == -1
    # the classes other tests pin keep their methods: the chain is a class of its own
    assert not hasattr(cmc.EccBatch, "apply_chain") and not hasattr(cmc.ECC, "apply_chain")
    with pytest.raises(ValueError):
        cmc.EccChain(1, max_frames=0)


def test_run_sequences_defaults_change_nothing():
    p = inspect.signature(motio.run_sequences).parameters
    assert (p["warps"].default, p["images"].default, p["cmc"].default) == (None, None, None)
    assert list(p)[-3:] == ["warps", "images", "cmc"]  # after every earlier argument
    assert motio.WARP_TRACKERS == ("botsort", "boosttrack", "strongsort", "deepocsort")


# ------------------------------------------------------------------------------ the chunk plan
def check_plan(stepped, sizes, chunk):
    calls = cmc.chain_plan(stepped, sizes, chunk)
    seen = {k: [] for k in range(len(stepped))}
    for size, seq, t in calls:
        assert 1 <= seq.size == t.size <= chunk and seq.dtype == t.dtype == np.int64
        assert all(sizes[k] == size for k in seq)  # a call never mixes sizes
        starts = seq[np.r_[True, seq[1:] != seq[:-1]]]
        assert len(set(starts.tolist())) == starts.size  # one contiguous run per sequence
        for k, x in zip(seq, t):
            seen[int(k)].append(int(x))
    for k, m in enumerate(stepped):  # every stepped frame exactly once, in order
        assert seen[k] == np.flatnonzero(np.asarray(m, bool)).tolist(), k
    return calls


MASKS = [np.array([1, 0, 1, 1, 0, 0, 1, 1, 1], bool), np.zeros(5, bool),
         np.array([0, 1, 1, 1, 1], bool), np.ones(7, bool), np.array([1], bool)]
SIZES = [(48, 64, 3), None, (40, 56, 3), (48, 64, 3), (40, 56, 3)]


@pytest.mark.parametrize("chunk", [1, 3, 4, 1000])
def test_chain_plan(chunk):
    calls = check_plan(MASKS, SIZES, chunk)
    total = sum(int(m.sum()) for m in MASKS)
    by_size = {}
    for size, seq, _ in calls:
        by_size[size] = by_size.get(size, 0) + seq.size
    assert by_size == {(48, 64, 3): 13, (40, 56, 3): 5} and sum(by_size.values()) == total
    # as few calls as the chunk allows, each size on its own
    assert len(calls) == -(-13 // chunk) + -(-5 // chunk)
    if chunk == 1000:
        assert [c[1].tolist() for c in calls] == [[0] * 6 + [3] * 7, [2] * 4 + [4]]
    if chunk == 1:
        assert all(c[1].size == 1 for c in calls)
    again = cmc.chain_plan(MASKS, SIZES, chunk)  # pure: the same plan again
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
               for a, b in zip(calls, again))


def test_chain_plan_edges():
    assert cmc.chain_plan([], [], 4) == []
    assert cmc.chain_plan([np.zeros(3, bool)], [None], 4) == []
    with pytest.raises(ValueError):
        cmc.chain_plan(MASKS, SIZES, 0)
    with pytest.raises(ValueError):
        cmc.chain_plan(MASKS, SIZES[:2], 4)
    # a sequence cut by the end of a call goes on at the start of the next
    calls = check_plan([np.ones(5, bool), np.ones(2, bool)], ["a", "a"], 3)
    assert [c[1].tolist() for c in calls] == [[0, 0, 0], [0, 0, 1], [1]]
    assert [c[2].tolist() for c in calls] == [[0, 1, 2], [3, 4, 0], [1]]


# ---------------------------------------------------------------------------------- refusals
@pytest.fixture
def no_engine(monkeypatch):
    """Any way to an engine or a table fails the test (the pattern of tests/test_tune_host.py)."""
    from boxmot_amd import engine, tracker_zoo

    def fail(*a, **k):
        pytest.fail("an engine or a table was built")

    monkeypatch.setattr(motio, "_batched_engine", fail)
    monkeypatch.setattr(tracker_zoo, "create_tracker", fail)
    monkeypatch.setattr(engine, "SequenceFeeder", fail)
    monkeypatch.setattr(cmc, "warp_table", fail)
    monkeypatch.setattr(cmc, "EccChain", fail)
    monkeypatch.setattr(cmc, "_Handle", fail)


EYE = np.tile(np.eye(2, 3).reshape(6), (3, 1))


@pytest.mark.parametrize("kind", ["bytetrack", "ocsort", "hybridsort"])
def test_trackers_without_cmc_are_refused(no_engine, tmp_path, kind):
    seqs = {"a": tmp_path / "missing"}  # never opened
    with pytest.raises(ValueError, match="takes no camera-motion warp"):
        motio.run_sequences(kind, seqs, tmp_path / "out", warps={"a": EYE})
    with pytest.raises(ValueError, match="takes no camera-motion warp"):
        motio.run_sequences(kind, seqs, tmp_path / "out", images={"a": None}, cmc="ecc")
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("kind", motio.WARP_TRACKERS)
def test_argument_refusals(no_engine, tmp_path, kind):
    seqs = {"a": tmp_path / "missing"}
    out = tmp_path / "out"
    img = {"a": np.zeros((3, 8, 8), np.uint8)}
    with pytest.raises(ValueError, match="per_class"):
        motio.run_sequences(kind, seqs, out, warps={"a": EYE}, tracker_kwargs={"per_class": True})
    with pytest.raises(ValueError, match="per_class"):
        motio.run_sequences(kind, seqs, out, images=img, cmc="ecc", n_classes=2)
    with pytest.raises(ValueError, match="images need cmc"):
        motio.run_sequences(kind, seqs, out, images=img)
    with pytest.raises(ValueError, match="not both"):
        motio.run_sequences(kind, seqs, out, images=img, cmc="ecc", warps={"a": EYE})
    with pytest.raises(ValueError, match="give images too"):
        motio.run_sequences(kind, seqs, out, cmc="ecc")
    with pytest.raises(ValueError, match="cmc goes with images"):
        motio.run_sequences(kind, seqs, out, warps={"a": EYE}, cmc="ecc")
    for bad in ("sof", {"levels": 3}, 7):
        with pytest.raises(ValueError, match="cmc must be"):
            motio.run_sequences(kind, seqs, out, images=img, cmc=bad)
    assert not list(tmp_path.iterdir())


def test_shape_refusals(no_engine, tmp_path):
    import torch

    rng = np.random.default_rng(0)

    def pack(name, frames):
        d = np.column_stack([np.repeat(frames, 2), rng.uniform(0, 50, (2 * len(frames), 4)),
                             np.full(2 * len(frames), 0.9), np.zeros(2 * len(frames))])
        return motio.pack_arrays(d, None, tmp_path / name)

    seqs = {"a": pack("a", [1, 2, 4]), "b": pack("b", [1, 2, 3, 4, 5])}
    out = tmp_path / "out"
    eye = lambda n: np.tile(np.eye(2, 3).reshape(6), (n, 1))  # noqa: E731
    with pytest.raises(ValueError, match="no warps for b"):
        motio.run_sequences("botsort", seqs, out, warps={"a": eye(3)})
    with pytest.raises(ValueError, match="for 3 iterated frames"):
        motio.run_sequences("botsort", seqs, out, warps={"a": eye(4), "b": eye(5)})
    with pytest.raises(ValueError, match="for 6 iterated frames"):  # frame_ids decide the length
        motio.run_sequences("botsort", seqs, out, warps={"a": eye(3), "b": eye(5)},
                            frame_ids={"b": [1, 2, 3, 4, 5, 6]})
    with pytest.raises(ValueError, match="mapping"):
        motio.run_sequences("botsort", seqs, out, warps=np.zeros((5, 2, 6)))

    def table(T, S):
        w = torch.zeros(T, S, 6, dtype=torch.float64)
        return cmc.WarpTable(w, torch.zeros(T, S, dtype=torch.float64),
                             torch.zeros(T, S, dtype=torch.int32),
                             torch.zeros(T, S, dtype=torch.int32))

    for T, S in ((5, 3), (4, 2), (6, 2)):
        with pytest.raises(ValueError, match="warp table"):
            motio.run_sequences("botsort", seqs, out, warps=table(T, S))
    with pytest.raises(ValueError, match="no images for b"):
        motio.run_sequences("botsort", seqs, out, images={"a": np.zeros((3, 8, 8), np.uint8)},
                            cmc="ecc")
    with pytest.raises(ValueError, match="4 images for 3 iterated frames"):
        motio.run_sequences("botsort", seqs, out, cmc={"scale": None},
                            images={"a": np.zeros((4, 8, 8), np.uint8),
                                    "b": np.zeros((5, 8, 8), np.uint8)})
    assert not out.exists()

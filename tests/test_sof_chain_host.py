"""Chained sparse optical flow and its way into the file flow, host side, no GPU: the ABI is
declared, bound and exported, and run_sequences takes a SOF instance as cmc and refuses what it
cannot do before any engine, handle or table is built."""
import inspect
import re
import subprocess

import numpy as np
import pytest

import boxmot_amd
from boxmot_amd import _native as N
from boxmot_amd import cmc, motio

NEW = ("bx_sof_chain_reserve", "bx_sof_apply_chain", "bx_sof_apply_chain_host")


def test_symbols_declared_bound_and_exported():
    text = N.HEADER_SOF.read_text()
    for s in NEW:
        assert re.search(rf"^int {s}\(", text, re.M), s
        assert s in N.EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", str(N.build())], capture_output=True,
                        text=True, check=True).stdout
    assert set(NEW) <= set(re.findall(r"\bT (bx_\w+)$", nm, re.M))
    L = N.load()
    # the header's argument lists: bx_sof_apply's 14 and dst; the host entry has no dst
    assert len(L.bx_sof_apply_chain.argtypes) == 15 and len(L.bx_sof_chain_reserve.argtypes) == 2
    assert len(L.bx_sof_apply_chain_host.argtypes) == 14 == len(L.bx_sof_apply_host.argtypes)
    decl = re.search(r"int bx_sof_apply_chain\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == 15 and "const int64_t *dst" in decl
    decl = re.search(r"int bx_sof_apply_chain_host\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == 14 and "dst" not in decl
    assert "bytes per slot" in text  # the header states what a slot costs


def test_python_surface():
    for name in ("SofChain", "sof_warp_table"):
        assert name in boxmot_amd.__all__ and getattr(boxmot_amd, name) is getattr(cmc, name)
    p = inspect.signature(cmc.sof_warp_table).parameters
    assert [k for k, v in p.items() if v.kind is v.KEYWORD_ONLY] == ["sof", "chunk"]
    assert p["sof"].default is None and p["chunk"].default == 64
    p = inspect.signature(cmc.SofChain.__init__).parameters
    assert list(p)[1:] == ["n_streams", "max_frames", "scale", "max_h", "max_w"]
    assert p["max_frames"].default == 64 and p["scale"].default == 0.15
    for m in ("apply", "apply_host", "reserve", "reset", "status", "state", "points", "close"):
        assert callable(getattr(cmc.SofChain, m))
    with pytest.raises(ValueError):
        cmc.SofChain(1, max_frames=0)
    # SOF's settings as attributes, with SOF's values; the chain's are those of its plain batch
    ch, sof = cmc.SofChain(2), cmc.SOF()
    for k in cmc._SOF_SETTINGS + ("scale", "grayscale"):
        assert getattr(ch, k) == getattr(sof, k), k
    ch.win_size = 9
    assert ch.batch.win_size == 9 and ch._params().win_size == 9
    assert ch.status() == 0 and not ch.state(0)["has_prev"]  # no handle yet: nothing to ask
    assert issubclass(cmc.SofWarpTable, cmc.WarpTable)
    # the classes other tests pin keep their methods: the chain is a class of its own
    assert not hasattr(cmc.SofBatch, "apply_chain") and not hasattr(cmc.SOF, "apply_chain")


# ---------------------------------------------------------------------------------- refusals
@pytest.fixture
def no_engine(monkeypatch):
    """Any way to an engine, a handle or a table fails the test."""
    from boxmot_amd import engine, tracker_zoo

    def fail(*a, **k):
        pytest.fail("an engine, a handle or a table was built")

    monkeypatch.setattr(motio, "_batched_engine", fail)
    monkeypatch.setattr(tracker_zoo, "create_tracker", fail)
    monkeypatch.setattr(engine, "SequenceFeeder", fail)
    for name in ("warp_table", "sof_warp_table", "EccChain", "SofChain", "SofBatch", "_Handle",
                 "_SofHandle"):
        monkeypatch.setattr(cmc, name, fail)


IMG = {"a": np.zeros((3, 8, 8), np.uint8)}
EYE = np.tile(np.eye(2, 3).reshape(6), (3, 1))


@pytest.mark.parametrize("kind", motio.WARP_TRACKERS)
def test_a_sof_instance_passes_the_checks(no_engine, kind):
    sof = cmc.SOF(scale=None)
    sof.win_size = 9
    before = dict(vars(sof))
    got = motio._check_warp_args(kind, {}, 0, None, IMG, sof)
    assert got == {"sof": sof} and vars(sof) == before  # neither run nor changed


@pytest.mark.parametrize("kind", ["bytetrack", "ocsort", "hybridsort"])
def test_trackers_without_cmc_are_refused(no_engine, tmp_path, kind):
    seqs = {"a": tmp_path / "missing"}  # never opened
    with pytest.raises(ValueError, match="takes no camera-motion warp"):
        motio.run_sequences(kind, seqs, tmp_path / "out", images=IMG, cmc=cmc.SOF())
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("kind", motio.WARP_TRACKERS)
def test_argument_refusals(no_engine, tmp_path, kind):
    seqs = {"a": tmp_path / "missing"}
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="per_class"):
        motio.run_sequences(kind, seqs, out, images=IMG, cmc=cmc.SOF(), n_classes=2)
    with pytest.raises(ValueError, match="per_class"):
        motio.run_sequences(kind, seqs, out, images=IMG, cmc=cmc.SOF(),
                            tracker_kwargs={"per_class": True})
    with pytest.raises(ValueError, match="switched off"):
        motio.run_sequences(kind, seqs, out, images=IMG, cmc=cmc.SOF(),
                            tracker_kwargs={"cmc_off": True})
    with pytest.raises(ValueError, match="not both"):
        motio.run_sequences(kind, seqs, out, images=IMG, cmc=cmc.SOF(), warps={"a": EYE})
    with pytest.raises(ValueError, match="give images too"):
        motio.run_sequences(kind, seqs, out, cmc=cmc.SOF())
    # SOF's own refusals come before any engine or table
    sof = cmc.SOF()
    sof.min_distance = 2
    with pytest.raises(NotImplementedError, match="min_distance"):
        motio.run_sequences(kind, seqs, out, images=IMG, cmc=sof)
    sof = cmc.SOF()
    sof.block_size = 5
    with pytest.raises(NotImplementedError, match="block_size"):
        motio.run_sequences(kind, seqs, out, images=IMG, cmc=sof)
    sof = cmc.SOF()
    sof.win_size = 8
    with pytest.raises(ValueError, match="win_size"):
        motio.run_sequences(kind, seqs, out, images=IMG, cmc=sof)
    # the interface is an instance: the string, the class and a batch are still refused
    for bad in ("sof", cmc.SOF, {"sof": cmc.SOF()}):
        with pytest.raises(ValueError, match="cmc must be"):
            motio.run_sequences(kind, seqs, out, images=IMG, cmc=bad)
    assert not list(tmp_path.iterdir())


def test_sof_warp_table_refuses_settings_first(no_engine):
    """The settings are checked before a frame is read or a handle is built."""
    sof = cmc.SOF()
    sof.min_distance = 2

    def unread(t):
        pytest.fail("a frame was read")

    with pytest.raises(NotImplementedError, match="min_distance"):  # (cmc's attribute is patched)
        boxmot_amd.sof_warp_table([unread], [np.ones(3, bool)], sof=sof)

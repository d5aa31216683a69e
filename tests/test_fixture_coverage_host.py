"""The reference-captured DeepOcSort, HybridSort and per-class fixtures, checked without a GPU:
each names the branches it is there for and reached them, its state snapshots are consistent,
and it stays small."""
import ast
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = sorted(p for pat in ("deepoc_*.npz", "hybrid_*.npz", "perclass_*.npz")
                  for p in GOLDEN.glob(pat))
# One limit for the three families: the size of the largest of these fixtures
# (hybrid_crowd96_f32) before the cases off the defaults were added.  A limit per family cannot
# hold: the largest deepoc_* file was 60700 bytes before its fixtures carried state, and
# deepoc_crowd96_f32 alone is some 200 KB with its four snapshots of 96 tracks
LARGEST = 317569
STATE_WIDTH = {"deepoc": 7, "hybrid": 9}


def test_the_families_are_there():
    stems = {p.stem for p in FIXTURES}
    assert len(FIXTURES) >= 34
    assert {"deepoc_dt7_warp", "deepoc_stop76", "hybrid_dt7", "hybrid_stop76",
            "perclass_deepoc_crowd24"} <= stems


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.stem)
def test_fixture_reaches_its_branches_and_stays_small(path):
    assert path.stat().st_size <= LARGEST
    family = path.stem.split("_")[0]
    with np.load(path) as fx:
        needs = ast.literal_eval(str(fx["needs"]))
        assert needs and all(int(fx[k]) > 0 for k in needs), needs
        assert int(fx["n_frames"]) <= 120
        if family == "perclass":
            assert not any(k.startswith("state_") for k in fx.files)
            return
        off, frames = fx["state_off"], fx["state_frames"]
        nf, n = int(fx["n_frames"]), STATE_WIDTH[family]
        assert list(frames) == [nf // 4, nf // 2, 3 * nf // 4, nf] and off.shape == (5,)
        assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] > 0
        rows = int(off[-1])
        arrays = [k for k in fx.files if k.startswith("state_") and k not in ("state_off",
                                                                               "state_frames")]
        assert {"state_id", "state_x", "state_P"} <= set(arrays)
        for k in arrays:
            assert fx[k].shape[0] == rows and np.isfinite(fx[k]).all(), k
        assert fx["state_x"].shape == (rows, n) and fx["state_P"].shape == (rows, n, n)
        for j in range(4):  # ids are unique inside a snapshot
            ids = fx["state_id"][off[j]: off[j + 1]]
            assert len(set(ids.tolist())) == ids.shape[0]
        if "state_emb" in fx.files:  # a track's embedding is a detection's row or a unit vector
            np.testing.assert_allclose(np.linalg.norm(fx["state_emb"], axis=1), 1.0, atol=1e-6)

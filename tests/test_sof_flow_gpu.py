"""Sparse-optical-flow warps in the many-sequence file flow (motio.run_sequences(images=,
cmc=SOF(...))): the files against one drop-in per sequence with ``tracker.cmc =
SOF(same settings)`` fed the same images frame by frame, byte for byte, and against the run
without warps, which must differ.  The scene is tests/test_cmc_flow_gpu.py's shaken texture."""
from pathlib import Path

import numpy as np
import pytest

from tests.test_cmc_flow_gpu import files, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu

KINDS = [("deepocsort", False), ("deepocsort", True), ("botsort", False)]


def dropin_files(kind, packed, images, fids, out):
    """process_sequence with one fresh drop-in per sequence, its cmc a SOF(scale=None)."""
    from boxmot_amd import BoostTrack, ByteTrack, DeepOcSort, cmc, motio
    from boxmot_amd.tracker_zoo import create_tracker

    codes = {}
    for nm, p in packed.items():
        ByteTrack.clear_count()
        BoostTrack._id_count = 0
        tr = DeepOcSort() if kind == "deepocsort" else create_tracker(kind)
        sof = cmc.SOF(scale=None)
        tr.cmc = sof
        seq = motio.BinSequence(p)
        res, codes[nm] = [], []
        for t, fid in enumerate(fids[nm]):
            d, e = seq.frame(fid)
            if not (d.size and e.size):
                continue
            rows = np.asarray(tr.update(d, images[nm][t], e), np.float64)
            codes[nm].append(sof.last["code"])
            if rows.size:
                res.append(motio.convert_to_mot_format(rows.reshape(rows.shape[0], -1), fid))
        motio.write_mot_results(Path(out) / f"{nm}.txt", np.vstack(res) if res else np.empty((0, 0)))
    return codes


@pytest.mark.parametrize("kind,resident", KINDS,
                         ids=[k + ("-resident" if r else "") for k, r in KINDS])
def test_flow_with_sof_equals_dropins(scene, kind, resident):  # noqa: F811
    from boxmot_amd import SOF, motio

    packed, images, fids, tmp = scene
    tag = tmp / ("sof_" + kind + ("_res" if resident else ""))
    kw = dict(frame_ids=fids, resident=resident)
    codes = dropin_files(kind, packed, images, fids, tag / "single")
    single = files(tag / "single", packed)
    assert all(len(b) > 0 for b in single.values())
    for nm, c in codes.items():  # every pair gives an estimate: the warps are not identities
        assert c[0] == 1 and set(c[1:]) == {0}, (nm, c)

    sof = SOF(scale=None)
    motio.run_sequences(kind, packed, tag / "images", images=images, cmc=sof, **kw)
    assert sof.last is None and sof._handle is None  # only its settings were read
    got = files(tag / "images", packed)
    for nm in packed:
        assert got[nm] == single[nm], f"{kind} {nm}: images= differs from the drop-in with SOF"

    motio.run_sequences(kind, packed, tag / "none", **kw)
    none = files(tag / "none", packed)
    for nm in packed:
        assert none[nm] != single[nm], f"{kind} {nm}: the warp changed nothing"

"""Camera-motion warps in the many-sequence file flow (motio.run_sequences(images=, cmc=) and
warps=): the files against one drop-in per sequence with ``tracker.cmc = ECC(same settings)`` fed
the same images frame by frame, byte for byte, and against the run without warps, which must
differ."""
import os
from pathlib import Path

import numpy as np
import pytest

from tests import ecc_ref as R

pytestmark = pytest.mark.gpu

F = 16
N_FRAMES = 12
ECC_KW = dict(warp_mode=0, eps=1e-5, max_iter=100, scale=None)
# name -> (image size, texture seed, the frame left without detections)
SEQS = {"PAN-A": ((48, 64), 21, None), "PAN-B": ((48, 64), 22, 5), "PAN-C": ((40, 56), 23, None)}
KINDS = [("botsort", False), ("strongsort", False), ("boosttrack", False), ("deepocsort", False),
         ("deepocsort", True)]


def pan(t):
    """The camera's offset at frame t: a shake of about (1.6, 1.5) px from every frame to the
    next, inside ECC's basin on this texture and nothing a constant-velocity filter predicts (a
    smooth pan it follows by itself, and the files would not show the warp)."""
    s = 1.0 if t % 2 else -1.0
    return np.array([0.8 * s + 0.1 * np.sin(t), 0.75 * s + 0.1 * np.cos(t)])


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from boxmot_amd import motio

    tmp = tmp_path_factory.mktemp("cmc_flow")
    # Boxes of 3 x 4 px (area 12, over the trackers' min_box_area of 10) under a shake of
    # (1.6, 1.5) px a frame: without the warp a predicted box overlaps its detection by an IoU
    # of 0.17, under every tracker's 0.3, and lies outside StrongSort's Mahalanobis gate (its
    # position sigma is h / 20), so the association itself changes.  (DeepOcSort outputs the
    # matched observation, StrongSort's update all but follows a 0.9 detection, and the files
    # hold whole pixels: a warp that only nudged the Kalman state would not show in them.)
    boxes = np.array([[8, 7, 11, 11], [26, 12, 29, 16], [43, 8, 46, 12], [13, 29, 16, 33],
                      [37, 27, 40, 31]], np.float64)
    packed, images, fids = {}, {}, {}
    for q, (nm, ((H, W), seed, hole)) in enumerate(SEQS.items()):
        rng = np.random.default_rng(50 + q)
        base = rng.standard_normal((len(boxes), F))
        rows, embs, imgs = [], [], []
        for t in range(N_FRAMES):
            c = pan(t + q)
            imgs.append(np.stack([R.texture(H, W, seed, R.shift_warp(*c))] * 3, -1))
            if t == hole:
                continue
            d = np.zeros((len(boxes), 7))
            d[:, 0] = t + 1
            d[:, 1:5] = boxes + np.tile(c, 2) + rng.normal(0, 0.05, boxes.shape)
            d[:, 5] = 0.9
            e = base + 0.02 * rng.standard_normal(base.shape)
            rows.append(d)
            embs.append(e / np.linalg.norm(e, axis=1, keepdims=True))
        packed[nm] = motio.pack_arrays(np.concatenate(rows), np.concatenate(embs),
                                       tmp / f"{nm}.bxmot")
        images[nm] = np.stack(imgs)
        fids[nm] = list(range(1, N_FRAMES + 1))
    return packed, images, fids, tmp


def tracker_kwargs(kind):
    return dict(handle_occlusions=False) if kind == "strongsort" else {}


def dropin_files(kind, packed, images, fids, out, with_ecc):
    """process_sequence with one fresh drop-in per sequence, its cmc an ECC of the same settings
    (or left as it is: the identity)."""
    from boxmot_amd import BoostTrack, ByteTrack, DeepOcSort, cmc, motio
    from boxmot_amd.tracker_zoo import create_tracker

    kw = tracker_kwargs(kind)
    warps = {}
    for nm, p in packed.items():
        ByteTrack.clear_count()
        BoostTrack._id_count = 0
        if kind == "deepocsort":
            tr = DeepOcSort()
        else:
            tr = create_tracker(kind, evolve_param_dict=kw) if kw else create_tracker(kind)
        ecc = cmc.ECC(**ECC_KW)
        if with_ecc:
            tr.cmc = ecc
        seq = motio.BinSequence(p)
        res = []
        warps[nm] = np.tile(np.eye(2, 3).reshape(6), (len(fids[nm]), 1))
        for t, fid in enumerate(fids[nm]):
            d, e = seq.frame(fid)
            if not (d.size and e.size):
                continue
            rows = np.asarray(tr.update(d, images[nm][t], e), np.float64)
            if with_ecc:
                warps[nm][t] = ecc.last["warp"].reshape(6)
            if rows.size:
                res.append(motio.convert_to_mot_format(rows.reshape(rows.shape[0], -1), fid))
        motio.write_mot_results(Path(out) / f"{nm}.txt", np.vstack(res) if res else np.empty((0, 0)))
    return warps


def files(d, names):
    return {nm: (Path(d) / f"{nm}.txt").read_bytes() for nm in names}


@pytest.mark.parametrize("kind,resident", KINDS,
                         ids=[k + ("-resident" if r else "") for k, r in KINDS])
def test_flow_with_ecc_equals_dropins(scene, monkeypatch, kind, resident):
    from boxmot_amd import motio

    monkeypatch.setenv("GITHUB_ACTIONS", "true")  # StrongSort born Confirmed, like its fixtures
    monkeypatch.delenv("GITHUB_JOB", raising=False)
    packed, images, fids, tmp = scene
    tag = tmp / (kind + ("_res" if resident else ""))
    kw = dict(frame_ids=fids, tracker_kwargs=tracker_kwargs(kind), resident=resident)
    ecc_warps = dropin_files(kind, packed, images, fids, tag / "single", True)
    single = files(tag / "single", packed)
    assert all(len(b) > 0 for b in single.values())

    motio.run_sequences(kind, packed, tag / "images", images=images, cmc=dict(ECC_KW), **kw)
    got = files(tag / "images", packed)
    for nm in packed:
        assert got[nm] == single[nm], f"{kind} {nm}: images= differs from the drop-in with ECC"

    # the same warps as plain arrays (frames that are not stepped hold the identity)
    motio.run_sequences(kind, packed, tag / "arrays", warps=ecc_warps, **kw)
    got = files(tag / "arrays", packed)
    for nm in packed:
        assert got[nm] == single[nm], f"{kind} {nm}: warps= differs from the drop-in with ECC"

    # without the warps the files are other files, and they are today's
    motio.run_sequences(kind, packed, tag / "none", **kw)
    none = files(tag / "none", packed)
    dropin_files(kind, packed, images, fids, tag / "single_none", False)
    assert none == files(tag / "single_none", packed)
    for nm in packed:
        assert none[nm] != single[nm], f"{kind} {nm}: the warp changed nothing"


def test_table_reused_across_runs(scene):
    """A table built once feeds any number of runs."""
    from boxmot_amd import cmc, motio

    packed, images, fids, tmp = scene
    stepped = [np.array([t != SEQS[nm][2] for t in range(N_FRAMES)]) for nm in packed]
    tab = cmc.warp_table([images[nm] for nm in packed], stepped, **ECC_KW)
    code = tab.host()["code"]
    assert code[5, 1] == -1 and code[0].tolist() == [1, 1, 1] and (code[1:] <= 0).all()
    for k in range(2):
        motio.run_sequences("botsort", packed, tmp / f"tab{k}", frame_ids=fids, warps=tab)
    motio.run_sequences("botsort", packed, tmp / "tab_img", frame_ids=fids, images=images,
                        cmc=dict(ECC_KW))
    assert files(tmp / "tab0", packed) == files(tmp / "tab1", packed) == \
        files(tmp / "tab_img", packed)
    tab.close()
    with pytest.raises(ValueError, match="warp table"):
        motio.run_sequences("botsort", packed, tmp / "closed", frame_ids=fids, warps=tab)
    assert not (tmp / "closed").exists() and os.path.isdir(tmp / "tab0")

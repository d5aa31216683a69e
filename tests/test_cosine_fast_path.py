"""K1c (`cosine_kernel`): the chunk-verdict divisions and the split, de-interleaved fp64 chains
against the element-by-element restatement (`cosine_kernel_any`, cosine mode 1) — same gated
pairs, bitwise-equal distances, identical outputs — and both against the oracle.

Geometry: 100-px boxes in rows, neighbours shifted 10 px (IoU 0.82 / 0.67 / 0.54 / 0.43 at 1 / 2 /
3 / 4 steps: under the duplicate-removal IoU of 0.85, gated with 3 neighbours on each side), the
rows of a sequence far apart.  A row of g boxes gates 1, 4, 9 pairs for g = 1, 2, 3 and 7g - 12
from g = 4, so the row sizes below fix every sequence's pair count."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

# the kernel's work split, read from the source the library is built from
_SRC = (Path(__file__).resolve().parents[1] / "boxmot_amd" / "csrc" / "bx_engine.hip").read_text()
COS_P = int(re.search(r"constexpr int COS_P = (\d+);", _SRC).group(1))
COS_BLOCKS = int(re.search(r"#define BX_COS_BLOCKS (\d+)", _SRC).group(1))
NWAVE = 4  # WG / WAVE = 256 / 64
# rows of boxes per sequence -> gated pairs: 0 (no detections after the first frame), 1,
# COS_P - 1, COS_P, COS_P + 1, and a second trip of the grid-stride loop
ROWS = [[2], [1], [3, 2, 1, 1], [4], [4, 1], [21]]
NO_DETS_AFTER_BIRTH = 0
PARAMS = dict(track_high_thresh=0.6, new_track_thresh=0.7, match_thresh=0.8)


def row_pairs(g):
    return g * g if g < 4 else 7 * g - 12


EXPECTED = [0 if s == NO_DETS_AFTER_BIRTH else sum(row_pairs(g) for g in rows)
            for s, rows in enumerate(ROWS)]
assert COS_P == 16, "ROWS is laid out for 16 pairs per wave: lay it out again"
assert EXPECTED == [0, 1, COS_P - 1, COS_P, COS_P + 1, 135]
assert EXPECTED[-1] > COS_BLOCKS * NWAVE * COS_P


def boxes(rows):
    out = []
    for r, g in enumerate(rows):
        for i in range(g):
            x, y = 50.0 + 10.0 * i, 40.0 + 300.0 * r
            out.append([x, y, x + 100.0, y + 100.0, 0.9, 0.0])
    return np.asarray(out, np.float32).reshape(-1, 6)


def embeddings(rng, base, content, dtype):
    e = base + 0.05 * rng.standard_normal(base.shape)
    if content == "relu":
        e = np.maximum(e, 0.0)
        zeros = np.argwhere(e == 0.0)
        for r, c in zeros[::3]:
            e[r, c] = -0.0
    e = e.astype(dtype)
    if content == "denormal" and e.shape[0] > 1:
        e[1, 5] = dtype(1e-40)  # one chunk of one wave takes the element-by-element redo
    return e


def frames(F, dtype, content):
    rng = np.random.default_rng(7 * F + len(content))
    dets = [boxes(rows) for rows in ROWS]
    # the objects of a sequence share a common direction (cosine ~0.8 between any two), so the
    # distance of every gated pair stays under appearance_thresh instead of saturating to 1.0
    base = [rng.standard_normal((1, F)) + 0.5 * rng.standard_normal((d.shape[0], F))
            for d in dets]
    out = []
    for t in range(1, 5):
        fr = []
        for s, d in enumerate(dets):
            e = embeddings(rng, base[s], content, dtype)
            if s == NO_DETS_AFTER_BIRTH and t > 1:
                d, e = d[:0], e[:0]
            fr.append((d, e))
        out.append(fr)
    return out


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return torch


def run_engine(torch, mode, F, dtype, frs):
    """Per frame: (output rows per sequence, sorted pair words and their distances per sequence)."""
    from boxmot_amd.engine import Engine, EngineParams

    S = len(ROWS)
    eng = Engine("botsort", n_seq=S, track_cap=64, det_cap=32, emb_dim=F,
                 emb_f64=dtype is np.float64, params=EngineParams(**PARAMS))
    eng.set_cosine_mode(mode)
    res = []
    for fr in frs:
        off = np.zeros(S + 1, np.int32)
        off[1:] = np.cumsum([d.shape[0] for d, _ in fr])
        d = torch.from_numpy(np.concatenate([d for d, _ in fr])).cuda()
        e = torch.from_numpy(np.concatenate([e for _, e in fr])).cuda()
        o = torch.empty((int(off[-1]), 8), dtype=torch.float64, device="cuda")
        c = torch.empty(S, dtype=torch.int32, device="cuda")
        eng.step(d, torch.from_numpy(off).cuda(), e, None, o, c)
        torch.cuda.synchronize()
        o, c = o.cpu().numpy(), c.cpu().numpy()
        rows = [o[off[s]: off[s] + c[s]].copy() for s in range(S)]
        dist = []
        for s in range(S):
            p, x = eng.embdist_host(s)
            k = np.argsort(p, kind="stable")
            dist.append((p[k], x[k]))
        res.append((rows, dist))
    assert eng.status() == 0
    eng.close()
    return res


@pytest.mark.parametrize("content", ["normal", "relu", "denormal"])
@pytest.mark.parametrize("F,dtype", [(512, np.float32), (64, np.float32), (96, np.float32),
                                     (64, np.float64)])
def test_cosine_fast_path_vs_restatement_and_oracle(torch_cuda, F, dtype, content):
    frs = frames(F, dtype, content)
    if content == "relu":
        e = np.concatenate([e for _, e in frs[1]])
        assert (e == 0).mean() >= 0.4 and np.signbit(e[e == 0]).any()
    fast = run_engine(torch_cuda, 0, F, dtype, frs)
    plain = run_engine(torch_cuda, 1, F, dtype, frs)
    oracles = [po.OracleTracker("botsort", **PARAMS) for _ in ROWS]
    informative = []
    for t, fr in enumerate(frs):
        for s, (d, e) in enumerate(fr):
            ref = oracles[s].update(d, e)
            np.testing.assert_array_equal(fast[t][0][s], plain[t][0][s],
                                          err_msg=f"rows, frame {t + 1} seq {s}")
            np.testing.assert_array_equal(fast[t][0][s], ref, err_msg=f"frame {t + 1} seq {s}")
            if t == 0:
                continue  # the first frame births the tracks: nothing to gate yet
            (pf, xf), (pp, xp) = fast[t][1][s], plain[t][1][s]
            assert len(pf) == EXPECTED[s], f"frame {t + 1} seq {s}: {len(pf)} gated pairs"
            np.testing.assert_array_equal(pf, pp)
            assert len(np.unique(pf)) == len(pf)
            np.testing.assert_array_equal(xf.view(np.uint64), xp.view(np.uint64),
                                          err_msg=f"distances, frame {t + 1} seq {s}")
            assert not np.isnan(xf).any()
            informative.append(xf < 1.0)
    informative = np.concatenate(informative)
    assert informative.mean() >= 0.9, f"{informative.mean():.2f} of the distances below 1.0"

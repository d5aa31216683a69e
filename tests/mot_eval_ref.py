"""numpy / scipy restatement of the MOT evaluation contract: HOTA, CLEAR and
Identity with the MOT16/17/20 pedestrian preprocessing, written from that contract and the
published metric definitions with plain loops and scipy's linear_sum_assignment.  It is the oracle
of tests/test_eval_gpu.py and tests/test_eval_cases_gpu.py and is itself pinned by the hand-worked
cases of tests/test_eval_host.py and tests/test_eval_cases_host.py.

evaluate_ref takes what boxmot_amd.evaluation.prepare_inputs returns and gives the dictionary
evaluate_mot gives.  With ``gaps`` (a list) it also records, for every preprocessing, HOTA and
CLEAR assignment, by how much the optimum falls when one of its value-carrying pairs is
forbidden (for a pair that stands alone in its row and column, a lower bound of that, without a
second solve): a positive gap for every pair means those pairs are the same in every optimum.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = np.finfo(np.float64).eps
ALPHAS = np.arange(0.05, 0.99, 0.05)
NA = len(ALPHAS)
DISTRACTORS = {"MOT16": (2, 7, 8, 12), "MOT17": (2, 7, 8, 12), "MOT20": (2, 7, 8, 12, 6)}


def iou_xywh(g, t):
    """[a, 4] x [b, 4] xywh boxes -> [a, b] IoU (areas from the corner form).  One gt box at a
    time against all tracker boxes: the same operations in the same order for every pair."""
    g, t = np.asarray(g, np.float64), np.asarray(t, np.float64)
    out = np.zeros((len(g), len(t)))
    if len(g) == 0 or len(t) == 0:
        return out
    bx0, by0 = t[:, 0], t[:, 1]
    bx1, by1 = t[:, 0] + t[:, 2], t[:, 1] + t[:, 3]
    ab = (bx1 - bx0) * (by1 - by0)
    for i in range(len(g)):
        ax0, ay0 = g[i, 0], g[i, 1]
        ax1, ay1 = g[i, 0] + g[i, 2], g[i, 1] + g[i, 3]
        aa = (ax1 - ax0) * (ay1 - ay0)
        inter = np.maximum(np.minimum(ax1, bx1) - np.maximum(ax0, bx0), 0.0) * \
            np.maximum(np.minimum(ay1, by1) - np.maximum(ay0, by0), 0.0)
        union = aa + ab - inter
        inter = np.where((aa <= EPS) | (ab <= EPS), 0.0, inter)
        empty = union <= EPS
        out[i] = np.where(empty, 0.0, inter) / np.where(empty, 1.0, union)
    return out


def _solve(score, gaps, floor=EPS):
    """linear_sum_assignment(-score); the pairs, and into gaps the loss of forbidding each pair
    whose score exceeds floor."""
    r, c = linear_sum_assignment(-score)
    if gaps is not None:
        best = score[r, c].sum()
        alone = (score > 0).sum(1)[:, None] + (score > 0).sum(0)[None, :] == 2
        alone &= score.min() >= 0
        for i, j in zip(r, c):
            if score[i, j] > floor and alone[i, j]:
                # the only positive entry of its row and its column, no negative one anywhere:
                # an assignment without it gains nothing from row i and column j and at most the
                # optimum of the rest from the rest, so the loss is at least score[i, j]
                gaps.append(score[i, j])
            elif score[i, j] > floor:
                alt = score.copy()
                alt[i, j] = -1e6
                r2, c2 = linear_sum_assignment(-alt)
                gaps.append(best - alt[r2, c2].sum())
    return r, c


def preprocess(gt, tr, T, benchmark, gaps=None):
    """Per frame (kept gt ids, kept tracker ids, their IoU tile), ids relabelled 0..n-1."""
    distract = DISTRACTORS[benchmark]
    frames = []
    for t in range(1, T + 1):
        g = gt[gt[:, 0] == t]
        r = tr[tr[:, 0] == t]
        keep_t = np.ones(len(r), bool)
        if len(g) and len(r):
            m = iou_xywh(g[:, 2:6], r[:, 2:6])
            m[m < 0.5 - EPS] = 0.0
            rows, cols = _solve(m, gaps)
            for i, j in zip(rows, cols):
                if m[i, j] > EPS and int(g[i, 7]) in distract:
                    keep_t[j] = False
        keep_g = (g[:, 6] != 0) & (g[:, 7] == 1) if len(g) else np.zeros(0, bool)
        g, r = g[keep_g], r[keep_t]
        frames.append((g[:, 1].astype(np.int64), r[:, 1].astype(np.int64),
                       iou_xywh(g[:, 2:6], r[:, 2:6])))
    gids = np.unique(np.concatenate([f[0] for f in frames]))
    tids = np.unique(np.concatenate([f[1] for f in frames]))
    frames = [(np.searchsorted(gids, a), np.searchsorted(tids, b), s) for a, b, s in frames]
    return frames, len(gids), len(tids)


def hota_final(res):
    tp, fn, fp = res["HOTA_TP"], res["HOTA_FN"], res["HOTA_FP"]
    res["DetA"] = tp / np.maximum(1.0, tp + fn + fp)
    res["DetRe"] = tp / np.maximum(1.0, tp + fn)
    res["DetPr"] = tp / np.maximum(1.0, tp + fp)
    res["HOTA"] = np.sqrt(res["DetA"] * res["AssA"])
    return res


def hota(frames, G, T, gaps=None):
    res = {k: np.zeros(NA) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP", "AssA", "AssRe", "AssPr",
                                     "LocA")}
    gdets = sum(len(f[0]) for f in frames)
    dets = sum(len(f[1]) for f in frames)
    if dets == 0 or gdets == 0:
        res["HOTA_FN"] += gdets if dets == 0 else 0
        res["HOTA_FP"] += dets if gdets == 0 else 0
        res["LocA"] += 1.0
        return hota_final(res)
    pot = np.zeros((G, T))
    gc = np.zeros(G)
    tc = np.zeros(T)
    for gi, ti, sim in frames:
        for i in gi:
            gc[i] += 1
        for j in ti:
            tc[j] += 1
        if len(gi) == 0 or len(ti) == 0:
            continue
        rs = [sum(sim[p, q] for q in range(len(ti))) for p in range(len(gi))]
        cs = [sum(sim[p, q] for p in range(len(gi))) for q in range(len(ti))]
        for p, i in enumerate(gi):
            for q, j in enumerate(ti):
                den = rs[p] + cs[q] - sim[p, q]
                if den > EPS:
                    pot[i, j] += sim[p, q] / den
    glob = pot / (gc[:, None] + tc[None, :] - pot)
    mc = np.zeros((NA, G, T))
    loc = np.zeros(NA)
    for gi, ti, sim in frames:
        if len(gi) == 0:
            res["HOTA_FP"] += len(ti)
            continue
        if len(ti) == 0:
            res["HOTA_FN"] += len(gi)
            continue
        score = glob[gi[:, None], ti[None, :]] * sim
        rows, cols = _solve(score, gaps, floor=0.0)
        for a, alpha in enumerate(ALPHAS):
            n = 0
            for p, q in zip(rows, cols):
                if sim[p, q] >= alpha - EPS:
                    n += 1
                    loc[a] += sim[p, q]
                    mc[a, gi[p], ti[q]] += 1
            res["HOTA_TP"][a] += n
            res["HOTA_FN"][a] += len(gi) - n
            res["HOTA_FP"][a] += len(ti) - n
    for a in range(NA):
        m = mc[a]
        tp = max(1.0, res["HOTA_TP"][a])
        res["AssA"][a] = np.sum(m * (m / np.maximum(1.0, gc[:, None] + tc[None, :] - m))) / tp
        res["AssRe"][a] = np.sum(m * (m / np.maximum(1.0, gc[:, None]))) / tp
        res["AssPr"][a] = np.sum(m * (m / np.maximum(1.0, tc[None, :]))) / tp
        res["LocA"][a] = loc[a] / max(1e-10, res["HOTA_TP"][a])
    return hota_final(res)


def hota_combine(all_res):
    res = {k: sum(r[k] for r in all_res) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP")}
    tp = res["HOTA_TP"]
    for k in ("AssA", "AssRe", "AssPr"):
        res[k] = sum(r[k] * r["HOTA_TP"] for r in all_res) / np.maximum(1.0, tp)
    wl = sum(r["LocA"] * r["HOTA_TP"] for r in all_res)
    res["LocA"] = np.where(tp == 0, 1.0, wl / np.where(tp == 0, 1.0, tp))
    return hota_final(res)


CLEAR_SUMS = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag", "MOTP_sum",
              "CLR_Frames")


def clear_final(res, degenerate=False):
    tp, fn, fp, idsw = res["CLR_TP"], res["CLR_FN"], res["CLR_FP"], res["IDSW"]
    gt = max(1.0, tp + fn)
    ids = max(1.0, res["MT"] + res["PT"] + res["ML"])
    res["MOTA"] = (tp - fp - idsw) / gt
    res["MOTP"] = res["MOTP_sum"] / max(1.0, tp)
    res["MODA"] = (tp - fp) / gt
    res["sMOTA"] = (res["MOTP_sum"] - fp - idsw) / gt
    res["CLR_Re"] = tp / gt
    res["CLR_Pr"] = tp / max(1.0, tp + fp)
    res["MTR"] = res["MT"] / ids
    res["PTR"] = res["PT"] / ids
    res["MLR"] = 1.0 if degenerate else res["ML"] / ids
    return res


def clear(frames, G, T, gaps=None):
    res = {k: 0 for k in CLEAR_SUMS}
    res["MOTP_sum"] = 0.0
    gdets = sum(len(f[0]) for f in frames)
    dets = sum(len(f[1]) for f in frames)
    if dets == 0 or gdets == 0:
        if dets == 0:
            res["CLR_FN"], res["ML"] = gdets, G
        else:
            res["CLR_FP"] = dets
        return clear_final(res, degenerate=True)
    gc = np.zeros(G)
    matched = np.zeros(G)
    frag = np.zeros(G)
    prev = np.full(G, -1)
    prev_t = np.full(G, -1)
    for gi, ti, sim in frames:
        if len(gi) == 0:
            res["CLR_FP"] += len(ti)
            continue
        for i in gi:
            gc[i] += 1
        if len(ti) == 0:
            res["CLR_FN"] += len(gi)
            prev_t[:] = -1
            continue
        score = np.zeros(sim.shape)
        for p, i in enumerate(gi):
            for q, j in enumerate(ti):
                score[p, q] = (1000.0 if prev_t[i] == j else 0.0) + sim[p, q]
                if sim[p, q] < 0.5 - EPS:
                    score[p, q] = 0.0
        rows, cols = _solve(score, gaps)
        new_t = np.full(G, -1)
        n = 0
        for p, q in zip(rows, cols):
            if not score[p, q] > EPS:
                continue
            i, j = gi[p], ti[q]
            n += 1
            if prev[i] >= 0 and prev[i] != j:
                res["IDSW"] += 1
            matched[i] += 1
            if prev_t[i] < 0:
                frag[i] += 1
            prev[i] = j
            new_t[i] = j
            res["MOTP_sum"] += sim[p, q]
        prev_t = new_t
        res["CLR_TP"] += n
        res["CLR_FN"] += len(gi) - n
        res["CLR_FP"] += len(ti) - n
    ratio = matched[gc > 0] / gc[gc > 0]
    res["MT"] = int(np.sum(ratio > 0.8))
    res["PT"] = int(np.sum(ratio >= 0.2)) - res["MT"]
    res["ML"] = G - res["MT"] - res["PT"]
    res["Frag"] = int(np.sum(frag[frag > 0] - 1))
    res["CLR_Frames"] = len(frames)
    return clear_final(res)


def identity_final(res):
    tp, fn, fp = res["IDTP"], res["IDFN"], res["IDFP"]
    res["IDF1"] = tp / max(1.0, tp + 0.5 * fp + 0.5 * fn)
    res["IDR"] = tp / max(1.0, tp + fn)
    res["IDP"] = tp / max(1.0, tp + fp)
    return res


def identity(frames, G, T):
    gdets = sum(len(f[0]) for f in frames)
    dets = sum(len(f[1]) for f in frames)
    if dets == 0 or gdets == 0:
        return identity_final({"IDTP": 0, "IDFN": gdets if dets == 0 else 0,
                               "IDFP": dets if gdets == 0 else 0})
    pot = np.zeros((G, T))
    gc = np.zeros(G)
    tc = np.zeros(T)
    for gi, ti, sim in frames:
        for p, i in enumerate(gi):
            gc[i] += 1
            for q, j in enumerate(ti):
                if sim[p, q] >= 0.5 - EPS:
                    pot[i, j] += 1
        for j in ti:
            tc[j] += 1
    n = G + T
    fn = np.full((n, n), 1e10)
    fp = np.full((n, n), 1e10)
    fn[G:, T:] = fp[G:, T:] = 0.0
    for i in range(G):
        for j in range(T):
            fn[i, j] = gc[i] - pot[i, j]
            fp[i, j] = tc[j] - pot[i, j]
        fn[i, T + i], fp[i, T + i] = gc[i], 0.0   # gt id i left unmatched
    for j in range(T):
        fn[G + j, j], fp[G + j, j] = 0.0, tc[j]   # tracker id j left unmatched
    rows, cols = linear_sum_assignment(fn + fp)
    idfn = int(fn[rows, cols].sum())
    idfp = int(fp[rows, cols].sum())
    return identity_final({"IDTP": gdets - idfn, "IDFN": idfn, "IDFP": idfp})


def _pack(h, c, d, count):
    hh = {}
    for k, v in h.items():
        hh[k + "_alpha"] = v.astype(np.int64) if k in ("HOTA_TP", "HOTA_FN", "HOTA_FP") else v
        hh[k] = float(np.mean(v))
    return {"HOTA": hh, "CLEAR": c, "Identity": d, "Count": count}


def evaluate_ref(names, frames, gts, trs, benchmark="MOT17", gaps=None):
    res, hs, cs, ds, ns = {}, [], [], [], []
    for name, T, gt, tr in zip(names, frames, gts, trs):
        fr, G, Tn = preprocess(gt, tr, int(T), benchmark, gaps)
        count = {"Dets": sum(len(f[1]) for f in fr), "GT_Dets": sum(len(f[0]) for f in fr),
                 "IDs": Tn, "GT_IDs": G}
        h, c, d = hota(fr, G, Tn, gaps), clear(fr, G, Tn, gaps), identity(fr, G, Tn)
        res[name] = _pack(h, c, d, count)
        hs.append(h), cs.append(c), ds.append(d), ns.append(count)
    comb_c = clear_final({k: sum(c[k] for c in cs) for k in CLEAR_SUMS})
    comb_d = identity_final({k: sum(d[k] for d in ds) for k in ("IDTP", "IDFN", "IDFP")})
    comb_n = {k: sum(n[k] for n in ns) for k in ns[0]}
    res["COMBINED"] = _pack(hota_combine(hs), comb_c, comb_d, comb_n)
    return res

"""Structured inputs of the MOT evaluation, shared by tests/test_eval_host.py,
tests/test_eval_cases_host.py (the numpy/scipy restatement alone) and tests/test_eval_cases_gpu.py
(the device against it).  A plain module: scene builders, named cases, their hand-derived
expectations, and the helpers that run a case.

Every coordinate and size (thresholds_exact apart) is a small integer (at most 2^20), so every
corner, area, intersection and union is exact in fp64 in any evaluation order and an IoU is one
correctly rounded division: the device and the restatement have to agree bit for bit on which
side of a threshold a pair lies.  Objects sit at least 100 px apart, so a value-carrying pair is the only candidate of its
row and its column and no case depends on a tie order (test_eval_cases_host.py checks the
assignment gaps of every case).  No number here comes from the code under test: the expectations
are worked out in the comments next to them."""
from collections import namedtuple

import numpy as np

import mot_eval_ref as R
from boxmot_amd import evaluation

# gt / tr / lengths: sequence name -> rows [n, 9] / rows [n, 9] / frames.  expect: sequence name
# (or "COMBINED") -> family -> field -> the exact value (an int, or a list of 19 for *_alpha).
Case = namedtuple("Case", "name gt tr lengths benchmark expect max_boxes")


def box(k, t=0):
    """Object k's 10 x 20 box, 100 px from its neighbours, drifting 1 px per frame."""
    return [100.0 * k + t, 50.0, 10.0, 20.0]


def gt_row(t, i, k, zm=1, cls=1):
    return [t, i, *box(k, t), zm, cls, 1.0]


def tr_row(t, i, k):
    return [t, i, *box(k, t), 0.9, -1, -1]


def rows(r):
    return np.asarray(r, float).reshape(-1, 9)


# ------------------------------------------------- the hand-worked scenes of test_eval_host.py
def perfect_tracker():
    gt = [gt_row(t, i, i) for t in range(1, 6) for i in (1, 2)]
    tr = [tr_row(t, 10 + i, i) for t in range(1, 6) for i in (1, 2)]
    return gt, tr


def id_swap_midway():
    """Two gt tracks, 10 frames; the tracker's two ids swap after frame 5.  Every box is exact."""
    gt = [gt_row(t, i, i) for t in range(1, 11) for i in (1, 2)]
    tr = [tr_row(t, (i if t <= 5 else 3 - i), i) for t in range(1, 11) for i in (1, 2)]
    return gt, tr


def track_dropped_for_three_frames():
    gt = [gt_row(t, i, i) for t in range(1, 11) for i in (1, 2)]
    tr = [tr_row(t, i, i) for t in range(1, 11) for i in (1, 2) if not (i == 2 and 4 <= t <= 6)]
    return gt, tr


def whole_frames_dropped():
    """One object; frames 4..6 have no tracker box at all."""
    gt = [gt_row(t, 1, 1) for t in range(1, 11)]
    tr = [tr_row(t, 1, 1) for t in range(1, 11) if not 4 <= t <= 6]
    return gt, tr


def distractor_and_zero_marked_rows():
    """Object 1 is a pedestrian, object 2 a class-8 distractor, object 3 a class-1 row with
    zero_marked = 0; the tracker reports all three."""
    gt = [r for t in range(1, 5) for r in (gt_row(t, 1, 1), gt_row(t, 2, 2, zm=0, cls=8),
                                           gt_row(t, 3, 3, zm=0, cls=1))]
    tr = [tr_row(t, i, i) for t in range(1, 5) for i in (1, 2, 3)]
    return gt, tr


def class6_rows():
    """Object 2 is class 6: a distractor for MOT20 only."""
    gt = [r for t in range(1, 5) for r in (gt_row(t, 1, 1), gt_row(t, 2, 2, zm=0, cls=6))]
    tr = [tr_row(t, i, i) for t in range(1, 5) for i in (1, 2)]
    return gt, tr


def gt_free_frames():
    """3 frames of two objects; tracker id 1 goes on over frames 4 and 5, which have no gt."""
    gt = [gt_row(t, i, i) for t in range(1, 4) for i in (1, 2)]
    tr = [tr_row(t, 1, 1) for t in range(1, 6)] + [tr_row(t, 2, 2) for t in range(1, 4)]
    return gt, tr


def _one(name, gt, tr, T, expect, benchmark="MOT17", max_boxes=None):
    return Case(name, {"S": rows(gt)}, {"S": rows(tr)}, {"S": T}, benchmark, {"S": expect},
                max_boxes)


def _hand_cases():
    """The scenes above as cases; the numbers are those test_eval_host.py derives and asserts."""
    a19 = lambda v: [v] * 19  # noqa: E731
    yield _one("hand_perfect", *perfect_tracker(), 5, {
        "HOTA": {"HOTA_TP_alpha": a19(10), "HOTA_FN_alpha": a19(0), "HOTA_FP_alpha": a19(0)},
        "CLEAR": {"CLR_TP": 10, "CLR_FN": 0, "CLR_FP": 0, "IDSW": 0, "Frag": 0, "MT": 2,
                  "CLR_Frames": 5},
        "Identity": {"IDTP": 10, "IDFN": 0, "IDFP": 0},
        "Count": {"Dets": 10, "GT_Dets": 10, "IDs": 2, "GT_IDs": 2}})
    yield _one("hand_id_swap", *id_swap_midway(), 10, {
        "HOTA": {"HOTA_TP_alpha": a19(20)},
        "CLEAR": {"CLR_TP": 20, "CLR_FN": 0, "CLR_FP": 0, "IDSW": 2, "Frag": 0, "MT": 2, "PT": 0,
                  "ML": 0},
        "Identity": {"IDTP": 10, "IDFN": 10, "IDFP": 10}})
    yield _one("hand_dropped_track", *track_dropped_for_three_frames(), 10, {
        "CLEAR": {"CLR_TP": 17, "CLR_FN": 3, "CLR_FP": 0, "IDSW": 0, "Frag": 1, "MT": 1, "PT": 1,
                  "ML": 0}})
    yield _one("hand_dropped_frames", *whole_frames_dropped(), 10, {
        "CLEAR": {"CLR_TP": 7, "CLR_FN": 3, "CLR_FP": 0, "IDSW": 0, "Frag": 1}})
    yield _one("hand_distractors", *distractor_and_zero_marked_rows(), 4, {
        "CLEAR": {"CLR_TP": 4, "CLR_FN": 0, "CLR_FP": 4},
        "Identity": {"IDTP": 4, "IDFN": 0, "IDFP": 4},
        "Count": {"Dets": 8, "GT_Dets": 4, "IDs": 2, "GT_IDs": 1}})
    for bm, dets in (("MOT17", 8), ("MOT20", 4)):
        yield _one(f"hand_class6_{bm}", *class6_rows(), 4, {"Count": {"Dets": dets, "GT_Dets": 4}},
                   benchmark=bm)
    yield _one("hand_gt_free_frames", *gt_free_frames(), 5, {
        "HOTA": {"HOTA_TP_alpha": a19(6), "HOTA_FP_alpha": a19(2)},
        "CLEAR": {"CLR_TP": 6, "CLR_FP": 2, "CLR_FN": 0, "CLR_Frames": 5},
        "Identity": {"IDTP": 6, "IDFP": 2}})


# ----------------------------------------------------------------------------- frame_kinds
# B: gt and tracker boxes, G: gt only, T: tracker boxes only, N: neither.  A digit after B is the
# phase: in phase 0 tracker id 11 sits on gt 1 and 12 on gt 2, in phase 1 the two are exchanged
# (a T frame carries the ids of the phase before it).  Frames 1..17 are a de Bruijn walk over the
# kinds (BB BG GB BT TB BN NG GG GT TG GN NT TT TN NN NB: all 16 ordered pairs); then the runs
#   17-19  B0 T B0   a gt-free gap, same id:         no Frag, no IDSW
#   19-21  B0 G B0   a tracker-free gap, same id:    one more fragment per gt id, no IDSW
#   21-23  B0 T B1   a gt-free gap, then the other id:       IDSW, no fragment
#   23-25  B1 G B0   a tracker-free gap, then the other id:  IDSW and a fragment
# and the same gaps over N and over runs of two.
FRAME_KINDS = ("B0 B0 G B0 T B0 N G G T G N T T N N B0 T B0 G B0 T B1 G B0 N B1 B1 G G B1 T T B1 "
               "N N B1 B0 G T").split()
# Per gt id (the two behave alike).  prev_t is empty at the start and after a G frame; T and N
# frames leave it alone.  A B frame with prev_t empty starts a fragment (frag_count + 1); a B
# frame whose phase differs from the last B frame's is an IDSW (the box of the old id lies on
# the other object, 100 px away: IoU 0, so the 1000-bonus is wiped out and the new id matches).
#   frame  1 B0  frag_count 1          frame 23 B1  IDSW 1 (prev_t still set by 21: no fragment)
#   frame  4 B0  frag_count 2 (3 is G) frame 25 B0  frag_count 5 (24 is G), IDSW 2
#   frame  6 B0  -  (5 is T)           frame 27 B1  IDSW 3 (26 is N: no fragment)
#   frame 17 B0  frag_count 3 (8 G)    frame 28 B1  -
#   frame 19 B0  -  (18 is T)          frame 31 B1  frag_count 6 (29, 30 are G), same id
#   frame 21 B0  frag_count 4 (20 G)   frames 34, 37 B1  -  (T T and N N before them)
#                                      frame 38 B0  IDSW 4
# so frag_count = 6 -> Frag 5 and IDSW 4 per gt id: Frag = 10, IDSW = 8.  15 B, 9 G, 9 T and 7 N
# frames: CLR_TP = 2 * 15, CLR_FN = 2 * 9, CLR_FP = 2 * 9 (the T frames' boxes); every IoU is 1,
# so HOTA_TP = 30 at every alpha and MOTP_sum = 30; matched / gt boxes = 15 / 24 per id: PT = 2.
# Identity: gt 1 shares 9 frames with id 11 (B0) and 6 with id 12 (B1), gt 2 the reverse; the
# best one-to-one map keeps 9 + 9 of the 48 boxes of either side.
FRAME_KINDS_EXPECT = {
    "HOTA": {"HOTA_TP_alpha": [30] * 19, "HOTA_FN_alpha": [18] * 19, "HOTA_FP_alpha": [18] * 19},
    "CLEAR": {"CLR_TP": 30, "CLR_FN": 18, "CLR_FP": 18, "IDSW": 8, "Frag": 10, "MT": 0, "PT": 2,
              "ML": 0, "CLR_Frames": 40},
    "Identity": {"IDTP": 18, "IDFN": 30, "IDFP": 30},
    "Count": {"Dets": 48, "GT_Dets": 48, "IDs": 2, "GT_IDs": 2}}


def _frame_kinds():
    gt, tr, phase = [], [], 0
    for t, kind in enumerate(FRAME_KINDS, 1):
        if kind[0] == "B":
            phase = int(kind[1])
        if kind[0] in "BG":
            gt += [gt_row(t, i, i) for i in (1, 2)]
        if kind[0] in "BT":
            tr += [tr_row(t, 11 + (i - 1 + phase) % 2, i) for i in (1, 2)]
    return _one("frame_kinds", gt, tr, len(FRAME_KINDS), FRAME_KINDS_EXPECT)


# ------------------------------------------------------------------------------ thresholds
# Nested boxes: gt (0, 0, 2000, 1), tracker (0, 0, w, 1): IoU = fl(w / 2000) exactly.  Frames
# 1..57: gt id 1 / tracker id 1 with w = 100 k - 1, 100 k, 100 k + 1 for k = 1..19.  Frames
# 58..60: w = 999, 1000, 1001 under gt id 2 / tracker id 2, and 500 px below them the same three
# widths over a class-8 distractor (gt id 3 / tracker id 3), which shows the 0.5 rule of the
# preprocessing: the boxes of 1000 and 1001 are removed, the one of 999 stays as an FP.
# HOTA_TP at alpha index a = frames with w >= 100 (a + 1); equality counts (fl(w / 2000) and
# 0.05 + 0.05 a differ by an ulp at most, eps is two at the least):
#   frames 1..57: 3 per k > a + 1 and 2 for k = a + 1, that is 3 (18 - a) + 2;
#   frames 58..60: 3 for a <= 8 (999 >= 900), 2 for a = 9, 0 above.
THRESHOLD_TP = [59, 56, 53, 50, 47, 44, 41, 38, 35, 31, 26, 23, 20, 17, 14, 11, 8, 5, 2]
# CLEAR / Identity (IoU >= 0.5 - eps): w >= 1000, that is 2 + 3 * 9 of frames 1..57 and 2 of
# 58..60: 31 of the 60 pedestrian boxes.  Tracker boxes kept: 57 + 3 + 1 (the 999 on the
# distractor); 61 - 31 = 30 of them are FPs.
THRESHOLDS_EXPECT = {
    "HOTA": {"HOTA_TP_alpha": THRESHOLD_TP, "HOTA_FN_alpha": [60 - v for v in THRESHOLD_TP],
             "HOTA_FP_alpha": [61 - v for v in THRESHOLD_TP]},
    "CLEAR": {"CLR_TP": 31, "CLR_FN": 29, "CLR_FP": 30, "IDSW": 0, "CLR_Frames": 60},
    "Identity": {"IDTP": 31, "IDFN": 29, "IDFP": 30},
    "Count": {"Dets": 61, "GT_Dets": 60, "IDs": 3, "GT_IDs": 2}}


def _thresholds():
    gt, tr, t = [], [], 0
    for k in range(1, 20):
        for w in (100 * k - 1, 100 * k, 100 * k + 1):
            t += 1
            gt.append([t, 1, 0, 0, 2000, 1, 1, 1, 1.0])
            tr.append([t, 1, 0, 0, w, 1, 0.9, -1, -1])
    for w in (999, 1000, 1001):
        t += 1
        gt.append([t, 2, 0, 0, 2000, 1, 1, 1, 1.0])
        tr.append([t, 2, 0, 0, w, 1, 0.9, -1, -1])
        gt.append([t, 3, 0, 500, 2000, 1, 0, 8, 1.0])
        tr.append([t, 3, 0, 500, w, 1, 0.9, -1, -1])
    return _one("thresholds", gt, tr, 60, THRESHOLDS_EXPECT)


# ------------------------------------------------------------------------ thresholds_exact
# The one case off the integer grid.  fl(w / 2000) never EQUALS a threshold alpha - eps (a ratio
# of small integers is never that close to k / 20 without being it), so the case above cannot
# tell `>= alpha - eps` from `> alpha - eps`.  Here gt (0, 0, 1, 1) holds tracker (0, 0, w, 1):
# inter = area = w, union = fl(fl(1 + w) - w), and for the widths below that is 1, so the IoU is
# w itself, bit for bit (test_eval_cases_host.py checks that with the restatement's IoU).
#   frames 1..17:  w = thr_a = fl(alpha_a - eps), a in THR_EXACT_AT:    a TP at indices <= a
#   frames 18..32: w = the double just below thr_a, a in THR_BELOW_AT:  a TP at indices < a
# (the a left out are those where the union does not round to 1).  HOTA_TP at index b is
# #{a in THR_EXACT_AT, a >= b} + #{a in THR_BELOW_AT, a > b}:
#   b      0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17 18
#   exact 17 16 15 14 13 12 11 10  9  8  7  6  5  4  4  3  2  1  0
#   below 14 13 13 12 11 10 10  9  8  7  6  6  5  4  3  2  2  1  0
# CLEAR and Identity keep IoU >= 0.5 - eps = thr_9: the 8 exact frames with a >= 9 (thr_9 itself
# is one: not `< 0.5 - eps`) and the 7 below frames with a > 9.
THR_EXACT_AT = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17)
THR_BELOW_AT = (0, 1, 3, 4, 5, 7, 8, 9, 10, 12, 13, 14, 15, 17, 18)
THRESHOLDS_EXACT_TP = [31, 29, 28, 26, 24, 22, 21, 19, 17, 15, 13, 12, 10, 8, 7, 5, 4, 2, 0]
THRESHOLDS_EXACT_EXPECT = {
    "HOTA": {"HOTA_TP_alpha": THRESHOLDS_EXACT_TP,
             "HOTA_FN_alpha": [32 - v for v in THRESHOLDS_EXACT_TP],
             "HOTA_FP_alpha": [32 - v for v in THRESHOLDS_EXACT_TP]},
    "CLEAR": {"CLR_TP": 15, "CLR_FN": 17, "CLR_FP": 17, "IDSW": 0, "CLR_Frames": 32},
    "Identity": {"IDTP": 15, "IDFN": 17, "IDFP": 17},
    "Count": {"Dets": 32, "GT_Dets": 32, "IDs": 1, "GT_IDs": 1}}


def threshold_widths():
    """The 17 + 15 tracker widths of thresholds_exact, in frame order."""
    thr = [0.05 + 0.05 * a - np.finfo(np.float64).eps for a in range(19)]
    return [thr[a] for a in THR_EXACT_AT] + [float(np.nextafter(thr[a], 0.0)) for a in THR_BELOW_AT]


def _thresholds_exact():
    gt, tr = [], []
    for t, w in enumerate(threshold_widths(), 1):
        gt.append([t, 1, 0, 0, 1, 1, 1, 1, 1.0])
        tr.append([t, 1, 0, 0, w, 1, 0.9, -1, -1])
    return _one("thresholds_exact", gt, tr, 32, THRESHOLDS_EXACT_EXPECT)


# ------------------------------------------------------------------------ degenerate_boxes
# Every frame has the normal pair gt 1 / tracker 11 on object 1 and a second pair gt 2 / tracker
# 12 on object 2, (x, y) = (200, 50), of which one box or both are degenerate.  (w, h):
DEGENERATE = [  # gt 2,     tracker 12
    ((10, 20), (0, 20)),     # tracker of zero width:      its area <= eps
    ((10, 20), (10, 0)),     # tracker of zero height
    ((10, 20), (-10, 20)),   # tracker of negative width:  area -200
    ((0, 20), (10, 20)),     # the same three on the gt side
    ((10, 0), (10, 20)),
    ((-10, 20), (10, 20)),
    ((0, 20), (0, 20)),      # two coinciding zero-area boxes: union <= eps -> 0 / 1
    ((0, 0), (0, 0)),
    ((-10, -20), (-10, -20)),  # area +200 from two negative sides: the clamped overlap is 0
]
# Every second pair has IoU 0: 9 TPs (object 1), 9 FNs (gt 2), 9 FPs (tracker 12); gt 1 is
# tracked in 9 / 9 frames (MT), gt 2 never (ML).  Identity: matching gt 2 with tracker 12 costs
# 9 + 9 like leaving both unmatched: the counts are the same either way.
DEGENERATE_EXPECT = {
    "HOTA": {"HOTA_TP_alpha": [9] * 19, "HOTA_FN_alpha": [9] * 19, "HOTA_FP_alpha": [9] * 19},
    "CLEAR": {"CLR_TP": 9, "CLR_FN": 9, "CLR_FP": 9, "IDSW": 0, "Frag": 0, "MT": 1, "PT": 0,
              "ML": 1, "CLR_Frames": 9},
    "Identity": {"IDTP": 9, "IDFN": 9, "IDFP": 9},
    "Count": {"Dets": 18, "GT_Dets": 18, "IDs": 2, "GT_IDs": 2}}


def _degenerate_boxes():
    gt, tr = [], []
    for t, ((gw, gh), (tw, th)) in enumerate(DEGENERATE, 1):
        gt += [[t, 1, 100, 50, 10, 20, 1, 1, 1.0], [t, 2, 200, 50, gw, gh, 1, 1, 1.0]]
        tr += [[t, 11, 100, 50, 10, 20, 0.9, -1, -1], [t, 12, 200, 50, tw, th, 0.9, -1, -1]]
    return _one("degenerate_boxes", gt, tr, len(DEGENERATE), DEGENERATE_EXPECT)


# ------------------------------------------------------------------- post_compaction_empty
# Frames that are empty on one side only after the preprocessing's compaction.  P: the pedestrian
# gt 1 on object 1; d8 / d6 / zm(k): a class-8 / class-6 / zero_marked = 0 class-1 gt row on
# object k; t11 / t12 / t13: tracker boxes exactly on objects 1 / 2 / 3.
#   frame  gt rows        tracker      MOT17 (kept gt, kept tr)        MOT20
#    1     P              t11          1, 1  TP                        the same
#    2     d8(2)          t13          0, 1  FP                        the same
#    3     d6(2)          t12 t13      0, 2  2 FP                      0, 1  FP (t12 removed)
#    4     zm(2)          t12          0, 1  FP (not a distractor)     the same
#    5     P d8(2) d8(3)  t12 t13      1, 0  FN, prev_t emptied        the same
#    6     d8(2) d8(3)    t12 t13      0, 0                            the same
#    7     P d6(2)        t11 t12      1, 2  TP (new fragment), FP     1, 1  TP (new fragment)
#    8     P              t11          1, 1  TP                        the same
#    9     P d6(2)        t12          1, 1  FN + FP, prev_t emptied   1, 0  FN, prev_t emptied
#                                            by a rebuild from no match
#   10     P              t11          1, 1  TP (new fragment)         the same
# gt 1 has 6 boxes, 4 matched (PT), frag_count 3 -> Frag 2; 14 tracker rows, 4 removed under
# MOT17 (frames 5, 6) and 3 more under MOT20 (t12 of frames 3, 7, 9); t12 of frame 4 keeps id 12
# alive in both.
POST_COMPACTION_EXPECT = {
    "MOT17": {
        "HOTA": {"HOTA_TP_alpha": [4] * 19, "HOTA_FN_alpha": [2] * 19, "HOTA_FP_alpha": [6] * 19},
        "CLEAR": {"CLR_TP": 4, "CLR_FN": 2, "CLR_FP": 6, "IDSW": 0, "Frag": 2, "MT": 0, "PT": 1,
                  "ML": 0, "CLR_Frames": 10},
        "Identity": {"IDTP": 4, "IDFN": 2, "IDFP": 6},
        "Count": {"Dets": 10, "GT_Dets": 6, "IDs": 3, "GT_IDs": 1}},
    "MOT20": {
        "HOTA": {"HOTA_TP_alpha": [4] * 19, "HOTA_FN_alpha": [2] * 19, "HOTA_FP_alpha": [3] * 19},
        "CLEAR": {"CLR_TP": 4, "CLR_FN": 2, "CLR_FP": 3, "IDSW": 0, "Frag": 2, "MT": 0, "PT": 1,
                  "ML": 0, "CLR_Frames": 10},
        "Identity": {"IDTP": 4, "IDFN": 2, "IDFP": 3},
        "Count": {"Dets": 7, "GT_Dets": 6, "IDs": 3, "GT_IDs": 1}}}


def _post_compaction_empty(benchmark):
    P = lambda t: gt_row(t, 1, 1)  # noqa: E731
    d8 = lambda t, k: gt_row(t, k, k, zm=0, cls=8)  # noqa: E731
    d6 = lambda t, k: gt_row(t, k, k, zm=0, cls=6)  # noqa: E731
    zm = lambda t, k: gt_row(t, k, k, zm=0, cls=1)  # noqa: E731
    tk = lambda t, k: tr_row(t, 10 + k, k)  # noqa: E731
    gt = [P(1), d8(2, 2), d6(3, 2), zm(4, 2), P(5), d8(5, 2), d8(5, 3), d8(6, 2), d8(6, 3),
          P(7), d6(7, 2), P(8), P(9), d6(9, 2), P(10)]
    tr = [tk(1, 1), tk(2, 3), tk(3, 2), tk(3, 3), tk(4, 2), tk(5, 2), tk(5, 3), tk(6, 2), tk(6, 3),
          tk(7, 1), tk(7, 2), tk(8, 1), tk(9, 2), tk(10, 1)]
    return _one(f"post_compaction_empty_{benchmark}", gt, tr, 10,
                POST_COMPACTION_EXPECT[benchmark], benchmark=benchmark)


# ----------------------------------------------------------------------------- wide_frames
# 10 x 20 boxes on a 100 px lattice, 40 sites to a row.  gt n (id n + 1) sits on site n; tracker
# box n (id 5001 + n) on the same site shifted right by n % 3 px: IoU 1, 180 / 220 or 160 / 240.
# Every tenth tracker box (n % 10 == 7) is moved onto an empty site beyond all gt instead: an FP,
# and its gt box an FN.  A pair is a TP up to alpha 0.65 (index 12) with any shift, up to 0.80
# (index 15) with a shift of 0 or 1, above that with shift 0 only.
LATTICE_W = 40


def _site(n, dx=0):
    return [100.0 * (n % LATTICE_W) + dx, 100.0 * (n // LATTICE_W), 10.0, 20.0]


def _lattice_frame(t, ng, nt):
    gt = [[t, n + 1, *_site(n), 1, 1, 1.0] for n in range(ng)]
    free = max(ng, nt)
    tr = [[t, 5001 + n, *(_site(free + n // 10) if n % 10 == 7 else _site(n, n % 3)), 0.9, -1, -1]
          for n in range(nt)]
    return gt, tr


def _lattice_tp(ng, nt):
    """HOTA_TP_alpha of one lattice frame, counted from the pattern: the pairs are the n below
    both counts that were not moved."""
    pairs = [n for n in range(min(ng, nt)) if n % 10 != 7]
    by_shift = [sum(1 for n in pairs if n % 3 <= s) for s in (0, 1, 2)]
    return [by_shift[2]] * 13 + [by_shift[1]] * 3 + [by_shift[0]] * 3


def _wide_expect(frames):
    tp = np.sum([_lattice_tp(ng, nt) for ng, nt in frames], axis=0)
    g, d = sum(f[0] for f in frames), sum(f[1] for f in frames)
    m = int(tp[0])  # (every pair's IoU is at least 2 / 3: CLEAR and Identity keep them all)
    return {"HOTA": {"HOTA_TP_alpha": [int(v) for v in tp], "HOTA_FN_alpha": [g - int(v) for v in tp],
                     "HOTA_FP_alpha": [d - int(v) for v in tp]},
            "CLEAR": {"CLR_TP": m, "CLR_FN": g - m, "CLR_FP": d - m, "IDSW": 0,
                      "CLR_Frames": len(frames)},
            "Identity": {"IDTP": m, "IDFN": g - m, "IDFP": d - m},
            "Count": {"Dets": d, "GT_Dets": g, "IDs": max(f[1] for f in frames),
                      "GT_IDs": max(f[0] for f in frames)}}


WIDE_A = ((257, 257), (320, 300), (1, 1))   # frames past the default 256 boxes, then one box
WIDE_B = ((1024, 1024),)                    # the largest frame a handle takes


def _wide_rows(frames):
    gt, tr = [], []
    for t, (ng, nt) in enumerate(frames, 1):
        g, r = _lattice_frame(t, ng, nt)
        gt += g
        tr += r
    return rows(gt), rows(tr)


def _wide_frames_512():
    g, t = _wide_rows(WIDE_A)
    return Case("wide_frames_512", {"A": g}, {"A": t}, {"A": 3}, "MOT17",
                {"A": _wide_expect(WIDE_A)}, 512)


def _wide_frames_1024():
    """Both sequences in one batch: the per-frame solver state is sized by the 1024-box frame
    while sequence A's last frame has one box."""
    ga, ta = _wide_rows(WIDE_A)
    gb, tb = _wide_rows(WIDE_B)
    return Case("wide_frames_1024", {"A": ga, "B": gb}, {"A": ta, "B": tb}, {"A": 3, "B": 1},
                "MOT17", {"A": _wide_expect(WIDE_A), "B": _wide_expect(WIDE_B)}, 1024)


# ---------------------------------------------------------------------------------- counts
# Frame counts around the 256 leaves and threads of the finishing kernels: two objects over T
# frames; tracker 11 follows gt 1 shifted by 1 px on odd frames (IoU 180 / 220: the per-alpha
# sums are not sums of ones), tracker 12 follows gt 2 exactly and is dropped on every frame that
# 7 divides (no T here ends on such a frame, so every drop ends a fragment: Frag = T // 7).
COUNT_FRAMES = (1, 255, 256, 257, 1025)


def _count_rows(T):
    gt = [gt_row(t, i, i) for t in range(1, T + 1) for i in (1, 2)]
    tr = []
    for t in range(1, T + 1):
        x, y, w, h = box(1, t)
        tr.append([t, 11, x + t % 2, y, w, h, 0.9, -1, -1])
        if t % 7:
            tr.append(tr_row(t, 12, 2))
    return rows(gt), rows(tr)


def _count_expect(T):
    drop, odd = T // 7, (T + 1) // 2
    tp = 2 * T - drop
    # 180 / 220 = 0.818.. is a TP up to alpha 0.80 (index 15); above that the odd frames' pairs
    # of gt 1 are not
    tpa = [tp] * 16 + [tp - odd] * 3
    return {"HOTA": {"HOTA_TP_alpha": tpa, "HOTA_FN_alpha": [2 * T - v for v in tpa],
                     "HOTA_FP_alpha": [tp - v for v in tpa]},
            "CLEAR": {"CLR_TP": tp, "CLR_FN": drop, "CLR_FP": 0, "IDSW": 0, "Frag": drop,
                      "CLR_Frames": T},
            "Identity": {"IDTP": tp, "IDFN": drop, "IDFP": 0},
            "Count": {"Dets": tp, "GT_Dets": 2 * T, "IDs": 2, "GT_IDs": 2}}


def _counts_frames():
    gt, tr, lengths, expect = {}, {}, {}, {}
    for T in COUNT_FRAMES:
        assert T % 7
        gt[f"T{T}"], tr[f"T{T}"] = _count_rows(T)
        lengths[f"T{T}"], expect[f"T{T}"] = T, _count_expect(T)
    return Case("counts_frames", gt, tr, lengths, "MOT17", expect, None)


# Sequence counts around the wave and the 256 threads of the combining kernel: S copies of a
# perfectly tracked three-frame, two-object sequence; copy c lacks tracker box c % 6 of its six
# (an FN), so COMBINED is not a multiple of one record.
COUNT_SEQS = (1, 65, 257)


def _counts_seqs(S):
    gt0, tr0 = [gt_row(t, i, i) for t in (1, 2, 3) for i in (1, 2)], \
        [tr_row(t, 10 + i, i) for t in (1, 2, 3) for i in (1, 2)]
    gt, tr, lengths, expect = {}, {}, {}, {}
    for c in range(S):
        n = f"C{c:03d}"
        gt[n], tr[n], lengths[n] = rows(gt0), rows(tr0[:c % 6] + tr0[c % 6 + 1:]), 3
        expect[n] = {"CLEAR": {"CLR_TP": 5, "CLR_FN": 1, "CLR_FP": 0, "IDSW": 0},
                     "Count": {"Dets": 5, "GT_Dets": 6, "IDs": 2, "GT_IDs": 2}}
    expect["COMBINED"] = {
        "HOTA": {"HOTA_TP_alpha": [5 * S] * 19, "HOTA_FN_alpha": [S] * 19, "HOTA_FP_alpha": [0] * 19},
        "CLEAR": {"CLR_TP": 5 * S, "CLR_FN": S, "CLR_FP": 0, "IDSW": 0, "CLR_Frames": 3 * S},
        "Identity": {"IDTP": 5 * S, "IDFN": S, "IDFP": 0},
        "Count": {"Dets": 5 * S, "GT_Dets": 6 * S, "IDs": 2 * S, "GT_IDs": 2 * S}}
    return Case(f"counts_seqs_{S}", gt, tr, lengths, "MOT17", expect, None)


BUILDERS = {}
for _c in _hand_cases():
    BUILDERS[_c.name] = (lambda c=_c: c)
BUILDERS.update({
    "frame_kinds": _frame_kinds,
    "thresholds": _thresholds,
    "thresholds_exact": _thresholds_exact,
    "degenerate_boxes": _degenerate_boxes,
    "post_compaction_empty_MOT17": lambda: _post_compaction_empty("MOT17"),
    "post_compaction_empty_MOT20": lambda: _post_compaction_empty("MOT20"),
    "wide_frames_512": _wide_frames_512,
    "wide_frames_1024": _wide_frames_1024,
    "counts_frames": _counts_frames,
})
for _s in COUNT_SEQS:
    BUILDERS[f"counts_seqs_{_s}"] = (lambda s=_s: _counts_seqs(s))
NAMES = tuple(BUILDERS)

_cases, _refs = {}, {}


def case(name):
    if name not in _cases:
        c = BUILDERS[name]()
        for d in (c.gt, c.tr):
            for a in d.values():
                a.setflags(write=False)
        _cases[name] = c
    return _cases[name]


def _freeze(x):
    if isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, np.ndarray):
        x.setflags(write=False)


def reference(name):
    """(the restatement's result of a case, its assignment gaps): computed once per process and
    shared, arrays read-only."""
    if name not in _refs:
        c = case(name)
        gaps = []
        want = R.evaluate_ref(*evaluation.prepare_inputs(c.gt, c.tr, c.lengths), c.benchmark, gaps)
        _freeze(want)
        _refs[name] = (want, tuple(gaps))
    return _refs[name]


def assert_expected(res, expect):
    """Every hand-written number of `expect`, exactly."""
    for seq, fams in expect.items():
        for fam, fields in fams.items():
            for k, v in fields.items():
                got = res[seq][fam][k]
                if isinstance(v, list):
                    assert got.dtype.kind == "i" and got.tolist() == v, (seq, fam, k, got, v)
                else:
                    assert isinstance(got, int) and got == v, (seq, fam, k, got, v)

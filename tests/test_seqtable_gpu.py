"""The six table engines through the shared path (engine._SeqTable over BxSeqTable) on the GPU:
set a range, read every sequence back, clear a sub-range, a refused call that changes nothing,
and grown().  The per-family tests/test_seqparams_*_gpu.py check what the entries do to the
tracking; this one checks that the six agree on the table itself."""
from dataclasses import replace

import pytest

pytestmark = pytest.mark.gpu

N_SEQ, CAPS, F = 5, dict(track_cap=32, det_cap=32), 20


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    from boxmot_amd import _native

    _native.load()
    return t


def cases():
    """name -> (make(params) -> engine, the engine's parameters, two entries, an entry the library
    refuses and the word its error carries)."""
    from boxmot_amd import engine as E

    def bot(kind):
        base = E.EngineParams(track_buffer=30, with_reid=kind == "botsort")
        return (lambda p: E.TableEngine(kind, N_SEQ, emb_dim=F, emb_f64=True, params=p, **CAPS),
                base, replace(base, match_thresh=0.6, track_buffer=2, frame_rate=10),
                replace(base, min_conf=0.3, track_thresh=0.35, new_track_thresh=0.4,
                        fuse_first_associate=True), replace(base, frame_rate=0), "frame_rate")

    oc, doc, hyb = E.OcsortParams(), E.DeepOcsortParams(), E.HybridsortParams()
    bst, ss = E.BoostParams(), E.SsParams()
    return {
        "ocsort": (lambda p: E.OcsortTableEngine(N_SEQ, params=p, **CAPS), oc,
                   replace(oc, max_age=5, delta_t=1, use_byte=True, asso_func="giou"),
                   replace(oc, det_thresh=0.4, inertia=0.3, Q_s_scaling=0.001),
                   replace(oc, delta_t=8), "delta_t"),
        "deepocsort": (lambda p: E.DeepOcsortTableEngine(N_SEQ, emb_dim=F, params=p, **CAPS), doc,
                       replace(doc, max_age=5, w_association_emb=0.75, aw_off=True),
                       replace(doc, iou_threshold=0.5, alpha_fixed_emb=0.9, asso_func="diou"),
                       replace(doc, delta_t=8), "delta_t"),
        "hybridsort": (lambda p: E.HybridsortTableEngine(N_SEQ, emb_dim=F, params=p, **CAPS), hyb,
                       replace(hyb, max_age=5, longterm_reid_weight=0.25),
                       replace(hyb, det_thresh=0.5, TCM_first_step_weight=1.0, delta_t=2),
                       replace(hyb, delta_t=0), "delta_t"),
        "bytetrack": bot("bytetrack"),
        "botsort": bot("botsort"),
        "boosttrack": (lambda p: E.BoostTableEngine(N_SEQ, emb_dim=F, params=p, **CAPS), bst,
                       replace(bst, max_age=90, use_rich_s=False, use_sb=False, lambda_iou=2.0),
                       replace(bst, min_hits=1, det_thresh=0.4, use_dlo_boost=False),
                       replace(bst, min_hits=-1), "min_hits"),
        "strongsort": (lambda p: E.SsTableEngine(N_SEQ, emb_dim=F, params=p, **CAPS), ss,
                       replace(ss, max_age=5, nn_budget=40, max_cos_dist=0.3),
                       replace(ss, n_init=1, ema_alpha=0.5, crowd_detection=False),
                       replace(ss, nn_budget=0), "nn_budget"),
    }


KINDS = ["ocsort", "deepocsort", "hybridsort", "bytetrack", "botsort", "boosttrack", "strongsort"]


@pytest.mark.parametrize("kind", KINDS)
def test_table_round_trip_through_the_shared_path(torch, kind):
    from boxmot_amd.engine import _SeqTable

    make, base, a, b, bad, word = cases()[kind]
    e = make(base)
    assert isinstance(e, _SeqTable)
    read = lambda x: [x.seq_params(q) for q in range(N_SEQ)]  # noqa: E731
    assert read(e) == [base] * N_SEQ
    e.set_seq_params(0, None)  # clearing an engine that never had a table is no error
    e.set_seq_params(1, [a, b, a])
    want = [base, a, b, a, base]
    assert read(e) == want and e._seq_over == {1: a, 2: b, 3: a}
    e.set_seq_params(2, None, nseq=1)
    want[2] = base
    assert read(e) == want and e._seq_over == {1: a, 3: a}
    # an entry the library refuses behind a valid one: neither is applied
    with pytest.raises(ValueError, match=word):
        e.set_seq_params(3, [b, bad])
    for seq0, n in ((N_SEQ - 1, 2), (-1, 1), (2, 2**31 - 1)):
        with pytest.raises(ValueError, match="range"):
            e.set_seq_params(seq0, None, nseq=n)
    assert read(e) == want and e._seq_over == {1: a, 3: a}
    g = e.grown(48, 48)
    assert type(g) is type(e) and (g.track_cap, g.det_cap) == (48, 48)
    assert read(g) == want and g._seq_over == e._seq_over
    g.set_seq_params(0, [b])  # the new engine's table is its own
    assert read(g) == [b] + want[1:] and read(e) == want
    assert e.status() == 0 and g.status() == 0
    g.close()
    e.close()

"""The shared per-sequence-parameter layer, host side, no GPU: engine._SeqTable on objects without
a handle, for all six table engines, and tune's sweep specs against the public sweeps."""
import ctypes as C
import inspect
from dataclasses import replace

import pytest

from boxmot_amd import engine as E
from boxmot_amd import tune

# table class, its prefix, what a handle-less object needs besides _h / n_seq / _L, its parameters,
# and a field (of the dataclass and the struct alike) with another value
TABLES = [
    (E.OcsortTableEngine, "bx_ocsort", {}, E.OcsortParams(), "max_age", 7),
    (E.DeepOcsortTableEngine, "bx_deepoc", {}, E.DeepOcsortParams(), "max_age", 7),
    (E.HybridsortTableEngine, "bx_hybrid", {}, E.HybridsortParams(), "max_age", 7),
    (E.TableEngine, "bx_engine", {"kind": "botsort"}, E.EngineParams(), "match_thresh", 0.5),
    (E.BoostTableEngine, "bx_boost", {}, E.BoostParams(), "max_age", 7),
    (E.SsTableEngine, "bx_ss", {}, E.SsParams(), "max_age", 7),
]
IDS = [t[0].__name__ for t in TABLES]


class FakeLib:
    """Records every call of a ``*_set_seq_params_host`` and returns ``rc``."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        def call(h, seq0, n, arr, stream):
            self.calls.append((name, h, seq0, n, arr, stream))
            return self.rc
        return call


def handleless(cls, more, params, lib, n_seq=6):
    e = cls.__new__(cls)
    e._h, e.n_seq, e.params, e._L = None, n_seq, params, lib
    for k, v in more.items():
        setattr(e, k, v)
    return e


@pytest.mark.parametrize("cls,prefix,more,params,field,value", TABLES, ids=IDS)
def test_set_seq_params_on_a_handleless_object(cls, prefix, more, params, field, value):
    lib = FakeLib()
    e = handleless(cls, more, params, lib)
    assert e._seq_over == {}  # (no __init__ ran: the mixin provides it)
    other = replace(params, **{field: value})
    e.set_seq_params(1, [params, other, params])
    name, h, seq0, n, arr, stream = lib.calls[-1]
    assert (name, h, seq0, n, stream) == (prefix + "_set_seq_params_host", None, 1, 3, None)
    assert isinstance(arr, cls._SEQ_STRUCT * 3)
    assert [getattr(x, field) for x in arr] == [getattr(params, field), value,
                                                getattr(params, field)]
    assert e._seq_over == {1: params, 2: other, 3: params}
    assert e._seq_over[2] is other  # as given, not a copy through the struct
    e.set_seq_params(2, None)  # every sequence from 2, a null array
    assert lib.calls[-1][2:5] == (2, e.n_seq - 2, None)
    assert e._seq_over == {1: params}
    e.set_seq_params(0, None, nseq=1)
    assert lib.calls[-1][2:5] == (0, 1, None) and e._seq_over == {1: params}
    e.set_seq_params(4, [])  # an empty list is a call of length 0
    assert lib.calls[-1][2:4] == (4, 0) and e._seq_over == {1: params}
    assert len(lib.calls) == 4


@pytest.mark.parametrize("cls,prefix,more,params,field,value", TABLES, ids=IDS)
def test_seq_over_follows_the_librarys_answer(cls, prefix, more, params, field, value):
    """Updated only after the library returned 0; untouched when it refused."""
    lib = FakeLib()
    e = handleless(cls, more, params, lib)
    e.set_seq_params(0, [params, params])
    lib.rc = 1  # BX_ERR_INVALID
    with pytest.raises(ValueError):
        e.set_seq_params(1, [replace(params, **{field: value})] * 3)
    with pytest.raises(ValueError):
        e.set_seq_params(0, None)
    assert len(lib.calls) == 3 and e._seq_over == {0: params, 1: params}


def test_track_buffer_none_takes_the_kinds_default():
    """bx_engine's entry: EngineParams.track_buffer None resolves as Engine.__init__ resolves it."""
    for kind, want in (("bytetrack", 25), ("botsort", 30)):
        lib = FakeLib()
        e = handleless(E.TableEngine, {"kind": kind}, E.EngineParams(), lib)
        e.set_seq_params(0, [E.EngineParams(), E.EngineParams(track_buffer=4)])
        assert [x.track_buffer for x in lib.calls[-1][4]] == [want, 4]


@pytest.mark.parametrize("cls,params,field", [
    (E.DeepOcsortTableEngine, E.DeepOcsortParams(), "embedding_off"),
    (E.BoostTableEngine, E.BoostParams(), "with_reid")])
def test_engine_wide_field_is_refused_before_the_library(cls, params, field):
    lib = FakeLib()
    e = handleless(cls, {}, params, lib)
    with pytest.raises(ValueError, match=f"{field} is engine-wide"):
        e.set_seq_params(0, [params, replace(params, **{field: not getattr(params, field)})])
    assert lib.calls == [] and e._seq_over == {}


def test_seq_params_reads_through_the_struct():
    """seq_params hands the library a struct of the class's type and maps it back."""
    class Lib:
        def bx_ocsort_seq_params_host(self, h, seq, ref):
            o = C.cast(ref, C.POINTER(E.OcsortTableEngine._SEQ_STRUCT)).contents
            o.max_age, o.delta_t, o.asso_kind = 11 + seq, 2, 0
            return 0

    base = E.OcsortParams(frame_w=640.0, frame_h=480.0)
    e = handleless(E.OcsortTableEngine, {}, base, Lib())
    got = e.seq_params(3)
    assert (got.max_age, got.delta_t, got.asso_func) == (14, 2, "iou")
    assert (got.frame_w, got.frame_h) == (640.0, 480.0)  # (the engine's: not in the table)


# ---------------------------------------------------------------------------- tune's specs
SUPPORTED = {"sweep": "SUPPORTED", "sweep_reid": "SUPPORTED_REID", "sweep_bot": "SUPPORTED_BOT",
             "sweep_boost": "SUPPORTED_BOOST", "sweep_strong": "SUPPORTED_STRONG"}


@pytest.mark.parametrize("kind", list(tune.GSI_DISPATCH))
def test_spec_matches_its_public_sweep(kind):
    name = tune.GSI_DISPATCH[kind]
    spec = tune._SPECS[name]
    assert spec.name == name and kind in spec.supported
    assert spec.supported == getattr(tune, SUPPORTED[name])
    public = getattr(tune, name)
    assert tune._PUBLIC[name] is public
    sig = inspect.signature(public).parameters
    keywords = {k for k, p in sig.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert keywords == set(public.__kwdefaults__) == spec.keywords - set(spec.extra)
    assert ("frame_sizes" in keywords) == spec.frame_sizes == (name in ("sweep", "sweep_reid"))
    assert ("warps" in keywords) == spec.warps == (name != "sweep")
    assert spec.extra == (("occlusion",) if name == "sweep_strong" else ())


def test_specs_cover_the_dispatch_table_and_no_copies_remain():
    assert set(tune._SPECS) == set(tune.GSI_DISPATCH.values()) == set(SUPPORTED)
    every = [k for s in tune._SPECS.values() for k in s.supported]
    assert sorted(every) == sorted(tune.GSI_DISPATCH)  # each tracker in exactly one spec
    for gone in ("_sweep", "_sweep_reid", "_sweep_bot", "_sweep_boost", "_sweep_strong",
                 "_resolve_strong"):
        assert not hasattr(tune, gone)
    assert "globals()" not in inspect.getsource(tune)
    # sweep_strong_device is sweep_strong's spec with its extra keyword
    sig = inspect.signature(tune.sweep_strong_device).parameters
    assert set(sig) - set(inspect.signature(tune.sweep_strong).parameters) == {"occlusion"}

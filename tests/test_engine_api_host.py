"""The public API of the engine handles, pinned: the six engine classes, ClassSplit and
SequenceFeeder expose exactly these public methods with exactly these signatures, whichever shared
base class implements them.  Importing boxmot_amd.engine needs no library until an engine is
constructed, so this runs without a device."""
import inspect

import pytest

import boxmot_amd.engine as E

# method name -> str(inspect.signature(...)), per class
API = {'BoostEngine': {'__init__': "(self, n_seq: 'int' = 1, track_cap: 'int' = 256, det_cap: 'int' = 256, "
                             "emb_dim: 'int' = 0, params: 'BoostParams | None' = None)",
                 'close': '(self)',
                 'counters': "(self, seq: 'int' = 0) -> 'dict'",
                 'frame_stats': "(self, seq0: 'int' = 0, nseq: 'int | None' = None) -> 'dict'",
                 'grown': '(self, track_cap: \'int\', det_cap: \'int\') -> "\'BoostEngine\'"',
                 'probe': "(self, stage) -> 'None'",
                 'probe_read': '(self)',
                 'reset': "(self, seq0: 'int' = 0, nseq: 'int | None' = None, stream=None)",
                 'set_id_count': "(self, seq: 'int', value: 'int')",
                 'slots_used': "(self, seq: 'int' = 0) -> 'int'",
                 'state_set': "(self, seq: 'int', ids, x=None, P=None) -> 'None'",
                 'status': "(self) -> 'int'",
                 'step': "(self, dets, det_off, embs, warps, out, out_count, seq0: 'int' = 0, nseq: 'int | "
                         "None' = None, stream=None)",
                 'tracks': "(self, seq: 'int' = 0) -> 'dict'",
                 'update_classes_host': "(self, seq: 'int', dets: 'np.ndarray', embs: 'np.ndarray | None' = "
                                        "None, warp: 'np.ndarray | None' = None, n_classes: 'int' = 80) -> "
                                        "'np.ndarray'",
                 'update_host': "(self, seq: 'int', dets: 'np.ndarray', embs: 'np.ndarray | None' = None, "
                                "warp: 'np.ndarray | None' = None) -> 'np.ndarray'"},
 'ClassSplit': {'__init__': "(self, n_seq: 'int', n_classes: 'int', emb_dim: 'int' = 0, row_cap: 'int' = "
                            "256, map_cap: 'int' = 4096, id0: 'int' = 1)",
                'close': '(self)',
                'id_count': "(self, seq: 'int' = 0) -> 'int'",
                'id_map': "(self, seq: 'int', cls: 'int') -> 'np.ndarray'",
                'merge': "(self, c_off, c_out, c_cnt, ids, det_off, out, out_count, seq0: 'int' = 0, nseq: "
                         "'int | None' = None, ids_stride: 'int' = 1, stream=None) -> 'None'",
                'reset': "(self, seq0: 'int' = 0, nseq: 'int | None' = None, stream=None) -> 'None'",
                'set_id_count': "(self, seq: 'int', value: 'int') -> 'None'",
                'split': "(self, dets, det_off, embs, o_dets, o_embs, o_off, o_src, nseq: 'int | None' = "
                         "None, stream=None) -> 'None'",
                'status': "(self) -> 'int'"},
 'DeepOcsortEngine': {'__init__': "(self, n_seq: 'int' = 1, track_cap: 'int' = 256, det_cap: 'int' = 256, "
                                  "emb_dim: 'int' = 512, params: 'DeepOcsortParams | None' = None)",
                      'classes': '(self)',
                      'classes_config': "(self, n_classes: 'int', map_cap: 'int') -> 'None'",
                      'close': '(self)',
                      'counters': "(self, seq: 'int' = 0) -> 'dict'",
                      'frame_stats': "(self, seq0: 'int' = 0, nseq: 'int | None' = None) -> 'dict'",
                      'grown': "(self, track_cap: 'int', det_cap: 'int', map_cap: 'int | None' = None) -> "
                               '"\'DeepOcsortEngine\'"',
                      'probe': "(self, stage) -> 'None'",
                      'probe_read': '(self)',
                      'reset': "(self, seq0: 'int' = 0, nseq: 'int | None' = None, stream=None)",
                      'set_frame_size': "(self, seq: 'int', w: 'float', h: 'float')",
                      'set_id_count': "(self, seq: 'int', value: 'int')",
                      'slots_used': "(self, seq: 'int' = 0) -> 'int'",
                      'state_set': "(self, seq: 'int', ids, x=None, P=None, emb=None) -> 'None'",
                      'status': "(self) -> 'int'",
                      'step': "(self, dets, det_off, embs, warps, out, out_count, seq0: 'int' = 0, nseq: "
                              "'int | None' = None, stream=None)",
                      'step_classes': "(self, dets, det_off, embs, warps, out, out_count, n_classes: 'int', "
                                      "seq0: 'int' = 0, nseq: 'int | None' = None, stream=None)",
                      'tracks': "(self, seq: 'int' = 0) -> 'dict'",
                      'update_classes_host': "(self, seq: 'int', n_classes: 'int', dets: 'np.ndarray', embs: "
                                             "'np.ndarray | None', id_count: 'int', warps: 'np.ndarray | "
                                             "None' = None)",
                      'update_host': "(self, seq: 'int', dets: 'np.ndarray', embs: 'np.ndarray | None' = "
                                     "None, warp: 'np.ndarray | None' = None) -> 'np.ndarray'"},
 'Engine': {'__init__': "(self, kind: 'str', n_seq: 'int' = 1, track_cap: 'int' = 1024, det_cap: 'int' = "
                        "384, emb_dim: 'int' = 0, emb_f64: 'bool' = False, params: 'EngineParams | None' = "
                        'None)',
            'class_tracks': "(self, seq: 'int', n_classes: 'int') -> 'list'",
            'close': '(self)',
            'counters': "(self, seq: 'int' = 0) -> 'dict'",
            'embdist_host': "(self, seq: 'int' = 0)",
            'force_assoc_build': "(self, mode: 'int') -> 'None'",
            'frame_stats': "(self, seq0: 'int' = 0, nseq: 'int' = None) -> 'dict'",
            'grown': '(self, track_cap: \'int\', det_cap: \'int\') -> "\'Engine\'"',
            'inputs_released': "(self, stream=None) -> 'None'",
            'lap_components': "(self, seq0: 'int' = 0, nseq: 'int | None' = None) -> 'dict'",
            'lap_ties': "(self, seq0: 'int' = 0, nseq: 'int | None' = None) -> 'int'",
            'probe': "(self, stage) -> 'None'",
            'probe_read': '(self)',
            'reset': "(self, seq0: 'int' = 0, nseq: 'int | None' = None, stream: 'int | None' = None)",
            'set_cosine_mode': "(self, mode: 'int') -> 'None'",
            'set_early_features': "(self, on: 'bool' = True) -> 'None'",
            'set_id_count': "(self, seq: 'int', value: 'int')",
            'set_lap_stats': "(self, on: 'bool' = True) -> 'None'",
            'set_overlap': "(self, on: 'bool' = True) -> 'None'",
            'slots_used': "(self, seq: 'int' = 0) -> 'int'",
            'state_set': "(self, seq: 'int', ids, mean=None, covariance=None) -> 'None'",
            'status': "(self) -> 'int'",
            'step': "(self, dets, det_off, embs=None, warps=None, out=None, out_count=None, seq0: 'int' = 0, "
                    "nseq: 'int | None' = None, stream=None)",
            'tracks': "(self, seq: 'int' = 0) -> 'dict'",
            'update_classes_host': "(self, seq: 'int', dets: 'np.ndarray', embs: 'np.ndarray | None' = None, "
                                   "warp: 'np.ndarray | None' = None, n_classes: 'int' = 80) -> 'np.ndarray'",
            'update_host': "(self, seq: 'int', dets: 'np.ndarray', embs: 'np.ndarray | None' = None, warp: "
                           "'np.ndarray | None' = None) -> 'np.ndarray'"},
 'HybridsortEngine': {'__init__': "(self, n_seq: 'int' = 1, track_cap: 'int' = 256, det_cap: 'int' = 256, "
                                  "emb_dim: 'int' = 512, params: 'HybridsortParams | None' = None)",
                      'classes': '(self)',
                      'classes_config': "(self, n_classes: 'int', map_cap: 'int') -> 'None'",
                      'close': '(self)',
                      'counters': "(self, seq: 'int' = 0) -> 'dict'",
                      'frame_stats': "(self, seq0: 'int' = 0, nseq: 'int | None' = None) -> 'dict'",
                      'grown': "(self, track_cap: 'int', det_cap: 'int', map_cap: 'int | None' = None) -> "
                               '"\'HybridsortEngine\'"',
                      'probe': "(self, stage) -> 'None'",
                      'probe_read': '(self)',
                      'reset': "(self, seq0: 'int' = 0, nseq: 'int | None' = None, stream=None)",
                      'set_frame_size': "(self, seq: 'int', w: 'float', h: 'float')",
                      'set_id_count': "(self, seq: 'int', value: 'int')",
                      'slots_used': "(self, seq: 'int' = 0) -> 'int'",
                      'state_load': "(self, seq: 'int', blob: 'np.ndarray') -> 'None'",
                      'state_save': "(self, seq: 'int' = 0) -> 'np.ndarray'",
                      'state_set': "(self, seq: 'int', ids, x=None, P=None) -> 'None'",
                      'status': "(self) -> 'int'",
                      'step': "(self, dets, det_off, embs, out, out_count, seq0: 'int' = 0, nseq: 'int | "
                              "None' = None, stream=None)",
                      'step_classes': "(self, dets, det_off, embs, out, out_count, n_classes: 'int', seq0: "
                                      "'int' = 0, nseq: 'int | None' = None, stream=None)",
                      'tracks': "(self, seq: 'int' = 0) -> 'dict'",
                      'update_classes_host': "(self, seq: 'int', n_classes: 'int', dets: 'np.ndarray', embs: "
                                             "'np.ndarray | None', id_count: 'int')",
                      'update_host': "(self, seq: 'int', dets: 'np.ndarray', embs: 'np.ndarray | None' = "
                                     "None) -> 'np.ndarray'"},
 'OcsortEngine': {'__init__': "(self, n_seq: 'int' = 1, track_cap: 'int' = 256, det_cap: 'int' = 256, "
                              "params: 'OcsortParams | None' = None)",
                  'close': '(self)',
                  'counters': "(self, seq: 'int' = 0) -> 'dict'",
                  'frame_stats': "(self, seq0: 'int' = 0, nseq: 'int | None' = None) -> 'dict'",
                  'grown': '(self, track_cap: \'int\', det_cap: \'int\') -> "\'OcsortEngine\'"',
                  'probe': "(self, on: 'bool' = True) -> 'None'",
                  'probe_read': '(self)',
                  'reset': "(self, seq0: 'int' = 0, nseq: 'int | None' = None, stream=None)",
                  'set_frame_size': "(self, seq: 'int', w: 'float', h: 'float')",
                  'set_id_count': "(self, seq: 'int', value: 'int')",
                  'slots_used': "(self, seq: 'int' = 0) -> 'int'",
                  'state_set': "(self, seq: 'int', ids, x=None, P=None) -> 'None'",
                  'status': "(self) -> 'int'",
                  'step': "(self, dets, det_off, out, out_count, seq0: 'int' = 0, nseq: 'int | None' = None, "
                          'stream=None)',
                  'tracks': "(self, seq: 'int' = 0) -> 'dict'",
                  'update_classes_host': "(self, seq0: 'int', n_classes: 'int', dets: 'np.ndarray', "
                                         "id_count: 'int')",
                  'update_host': "(self, seq: 'int', dets: 'np.ndarray') -> 'np.ndarray'"},
 'SequenceFeeder': {'__init__': "(self, dets, embs, tables, emb_dim: 'int', res_cap=None, guard_rows: 'int' "
                                '= 0)',
                    'append': "(self, t: 'int', stream=None) -> 'None'",
                    'close': '(self)',
                    'gather': "(self, t: 'int', stream=None) -> 'None'",
                    'raw_results': '(self)',
                    'read_run': "(self, t: 'int', r: 'int')",
                    'results': "(self) -> 'list'",
                    'status': "(self) -> 'int'",
                    'write_run': "(self, t: 'int', r: 'int', out, out_count) -> 'None'"},
 'SsEngine': {'__init__': "(self, n_seq: 'int' = 1, track_cap: 'int' = 256, det_cap: 'int' = 256, emb_dim: "
                          "'int' = 512, vec_cap: 'int' = 32, params: 'SsParams | None' = None)",
              'close': '(self)',
              'counters': "(self, seq: 'int' = 0) -> 'dict'",
              'frame_stats': "(self, seq0: 'int' = 0, nseq: 'int | None' = None) -> 'dict'",
              'grown': '(self, track_cap: \'int\', det_cap: \'int\') -> "\'SsEngine\'"',
              'last_features': "(self, seq: 'int', ids) -> 'np.ndarray'",
              'last_features_set': "(self, seq: 'int', ids, feats, normalize: 'bool' = True) -> 'None'",
              'lsap_stats': "(self, seq0: 'int' = 0, nseq: 'int | None' = None) -> 'dict'",
              'probe': "(self, stage) -> 'None'",
              'probe_read': '(self)',
              'reset': "(self, seq0: 'int' = 0, nseq: 'int | None' = None, stream=None)",
              'set_lsap_mode': "(self, fast: 'bool') -> 'None'",
              'slots_used': "(self, seq: 'int' = 0) -> 'int'",
              'state_set': "(self, seq: 'int', ids, mean=None, covariance=None) -> 'None'",
              'status': "(self) -> 'int'",
              'step': "(self, dets, det_off, embs, warps, out, out_count, seq0: 'int' = 0, nseq: 'int | "
                      "None' = None, stream=None)",
              'track_attrs': "(self, seq: 'int' = 0) -> 'dict'",
              'track_attrs_set': "(self, seq: 'int', ids, quality=None, conf=None, max_age=None) -> 'None'",
              'tracks': "(self, seq: 'int' = 0) -> 'dict'",
              'update_host': "(self, seq: 'int', dets: 'np.ndarray', embs: 'np.ndarray', warp: 'np.ndarray | "
                             "None' = None) -> 'np.ndarray'"}}


def _public(cls) -> dict:
    return {m: str(inspect.signature(v)) for m, v in inspect.getmembers(cls)
            if callable(v) and (m == "__init__" or not m.startswith("_"))}


@pytest.mark.parametrize("name", sorted(API))
def test_public_methods_and_signatures(name):
    got = _public(getattr(E, name))
    assert sorted(got) == sorted(API[name])
    assert got == API[name]


def test_stage_names():
    assert E.DeepOcsortEngine.STAGES == ["embcost", "frame", "feature"]
    assert E.HybridsortEngine.STAGES == ["dist", "frame", "feature"]
    assert E.BoostEngine.STAGES == ["embcost", "frame", "feature"]
    assert len(E.Engine.STAGES) == 9 and len(E.SsEngine.STAGES) == 9

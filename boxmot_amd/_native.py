"""ctypes binding of libbxassoc.so (include/bxassoc.h).

The HIP library is the product: there is no CPU fallback.  Importing this module never needs a
GPU, but any call into the engine on a machine without the built library or without a HIP
device raises ``NativeUnavailable`` — loudly, so a silent eager/CPU path can never stand in.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
REPO = PKG.parent
CSRC = PKG / "csrc"
LIB_DIR = PKG / "lib"
LIB_PATH = LIB_DIR / "libbxassoc.so"
HEADER = REPO / "include" / "bxassoc.h"
HEADER_OCS = REPO / "include" / "bxocsort.h"
HEADER_BOOST = REPO / "include" / "bxboost.h"
HEADER_SS = REPO / "include" / "bxstrongsort.h"
HEADER_DEEPOC = REPO / "include" / "bxdeepocsort.h"
HEADER_HYBRID = REPO / "include" / "bxhybridsort.h"
HEADER_IO = REPO / "include" / "bxio.h"
HEADER_GSI = REPO / "include" / "bxgsi.h"
HEADER_FEED = REPO / "include" / "bxfeed.h"
HEADER_CLASSES = REPO / "include" / "bxclasses.h"
HEADER_EVAL = REPO / "include" / "bxeval.h"
HEADER_CMC = REPO / "include" / "bxcmc.h"
HEADER_REID = REPO / "include" / "bxreid.h"
HEADER_SOF = REPO / "include" / "bxsof.h"
HEADER_DET = REPO / "include" / "bxdet.h"

HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    # numpy-identical rounding: no FMA contraction, IEEE f32 division/sqrt
    "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
    # MFMA accumulators in the VGPR form: the compiler otherwise copies the StrongSort NN
    # kernel's accumulator tiles between VGPRs and AGPRs around every k-block
    "-mllvm", "-amdgpu-mfma-vgpr-form=1",
]
SOURCES = ["bx_engine.hip", "bx_ops.hip", "bx_ocsort.hip", "bx_nn.hip", "bx_boost.hip",
           "bx_strongsort.hip", "bx_deepocsort.hip", "bx_hybridsort.hip", "bx_gsi.hip", "bx_feed.hip",
           "bx_classes.hip", "bx_eval.hip", "bx_cmc.hip", "bx_reid.hip", "bx_sof.hip",
           "bx_io.cpp", "bx_boost_tab.hip", "bx_strongsort_tab.hip", "bx_strongsort_occ.hip",
           "bx_det.hip"]


class NativeUnavailable(RuntimeError):
    pass


def _deps(src: Path, seen=None) -> list:
    """src and the in-tree headers it includes (transitively)."""
    import re

    seen = set() if seen is None else seen
    if src in seen or not src.exists():
        return []
    seen.add(src)
    out = [src]
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', src.read_text(), re.M):
        for d in (src.parent, REPO / "include"):
            if (d / inc).exists():
                out += _deps((d / inc).resolve(), seen)
                break
    return out


def _toolchain_stamp(hipcc: str, flags: list) -> str:
    """Hash of the compile flags and the compiler's version: objects built under another stamp
    are stale even when their sources did not change."""
    import hashlib

    try:
        ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
    except OSError:
        ver = ""
    return hashlib.sha256(("\0".join(flags) + "\0" + ver).encode()).hexdigest()[:16]


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile the HIP extension for gfx950 in-tree (boxmot_amd/lib/libbxassoc.so): one object per
    translation unit (compiled in parallel, and only when it or a header it includes changed, or
    the flags / compiler did), then one link.  Temporary outputs carry the process id, so two
    processes building at once never replace each other's half-written file."""
    from concurrent.futures import ThreadPoolExecutor

    objdir = LIB_DIR / "obj"
    objdir.mkdir(parents=True, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # BX_HIPCC_EXTRA: extra compile flags for a debug build (e.g. -DBX_CHECK: device-side bounds
    # checks latched as engine errors); part of the toolchain stamp, so switching rebuilds
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + os.environ.get("BX_HIPCC_EXTRA", "").split()
    link_flags = [f for f in HIPCC_FLAGS if f.startswith("--offload-arch")] + ["-shared", "-fPIC"]
    stamp_file = objdir / "toolchain.stamp"
    stamp = _toolchain_stamp(hipcc, flags)
    if not stamp_file.exists() or stamp_file.read_text().strip() != stamp:
        force = True
    stale = []
    objs = []
    for s in SOURCES:
        src = CSRC / s
        obj = objdir / (s + ".o")
        objs.append(obj)
        if force or not obj.exists() or any(d.stat().st_mtime > obj.stat().st_mtime
                                            for d in _deps(src)):
            stale.append((src, obj))

    def compile_one(so):
        src, obj = so
        tmp = obj.with_suffix(f".o.{os.getpid()}.tmp")
        r = subprocess.run([hipcc, *flags, "-c", "-o", str(tmp), str(src)], capture_output=True,
                           text=True)
        if r.returncode != 0:
            tmp.unlink(missing_ok=True)
            raise RuntimeError(f"hipcc failed on {src.name}:\n{r.stderr}")
        if verbose and r.stderr:
            print(r.stderr)
        os.replace(tmp, obj)

    if stale:
        with ThreadPoolExecutor(max_workers=min(len(stale), os.cpu_count() or 1)) as ex:
            list(ex.map(compile_one, stale))
        stamp_file.write_text(stamp + "\n")
    if not stale and LIB_PATH.exists() and all(
            o.stat().st_mtime <= LIB_PATH.stat().st_mtime for o in objs):
        return LIB_PATH
    LIB_DIR.mkdir(exist_ok=True)
    tmp = LIB_PATH.with_suffix(f".so.{os.getpid()}.tmp")
    r = subprocess.run([hipcc, *link_flags, "-o", str(tmp), *[str(o) for o in objs]],
                       capture_output=True, text=True)
    if r.returncode != 0:
        tmp.unlink(missing_ok=True)
        raise RuntimeError(f"hipcc link failed:\n{r.stderr}")
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


class BxConfig(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("n_seq", C.c_int32), ("track_cap", C.c_int32),
        ("det_cap", C.c_int32), ("emb_dim", C.c_int32), ("emb_f64", C.c_int32),
        ("min_conf", C.c_double), ("track_thresh", C.c_double), ("match_thresh", C.c_double),
        ("track_buffer", C.c_int32), ("frame_rate", C.c_int32),
        ("track_high_thresh", C.c_double), ("track_low_thresh", C.c_double),
        ("new_track_thresh", C.c_double), ("proximity_thresh", C.c_double),
        ("appearance_thresh", C.c_double),
        ("fuse_first_associate", C.c_int32), ("with_reid", C.c_int32),
    ]


class BxOcsortConfig(C.Structure):
    _fields_ = [
        ("n_seq", C.c_int32), ("track_cap", C.c_int32), ("det_cap", C.c_int32),
        ("min_conf", C.c_double), ("det_thresh", C.c_double), ("asso_threshold", C.c_double),
        ("inertia", C.c_double), ("q_xy_scaling", C.c_double), ("q_s_scaling", C.c_double),
        ("max_age", C.c_int32), ("min_hits", C.c_int32), ("delta_t", C.c_int32),
        ("use_byte", C.c_int32), ("asso_kind", C.c_int32), ("frame_w", C.c_double),
        ("frame_h", C.c_double),
    ]


class BxOcsortSeqParams(C.Structure):
    _fields_ = [
        ("min_conf", C.c_double), ("det_thresh", C.c_double), ("asso_threshold", C.c_double),
        ("inertia", C.c_double), ("q_xy_scaling", C.c_double), ("q_s_scaling", C.c_double),
        ("max_age", C.c_int32), ("min_hits", C.c_int32), ("delta_t", C.c_int32),
        ("use_byte", C.c_int32), ("asso_kind", C.c_int32),
    ]


class BxEngineSeqParams(C.Structure):
    _fields_ = [
        ("min_conf", C.c_double), ("track_thresh", C.c_double),
        ("track_high_thresh", C.c_double), ("track_low_thresh", C.c_double),
        ("new_track_thresh", C.c_double), ("proximity_thresh", C.c_double),
        ("appearance_thresh", C.c_double), ("fuse_first_associate", C.c_int32),
        ("match_thresh", C.c_double), ("track_buffer", C.c_int32), ("frame_rate", C.c_int32),
    ]


class BxBoostConfig(C.Structure):
    _fields_ = [
        ("n_seq", C.c_int32), ("track_cap", C.c_int32), ("det_cap", C.c_int32),
        ("emb_dim", C.c_int32), ("max_age", C.c_int32), ("min_hits", C.c_int32),
        ("det_thresh", C.c_double), ("iou_threshold", C.c_double), ("min_box_area", C.c_double),
        ("aspect_ratio_thresh", C.c_double), ("lambda_iou", C.c_double),
        ("lambda_mhd", C.c_double), ("lambda_shape", C.c_double), ("dlo_boost_coef", C.c_double),
        ("use_ecc", C.c_int32), ("use_dlo_boost", C.c_int32), ("use_duo_boost", C.c_int32),
        ("s_sim_corr", C.c_int32), ("use_rich_s", C.c_int32), ("use_sb", C.c_int32),
        ("use_vt", C.c_int32), ("with_reid", C.c_int32),
    ]


class BxBoostSeqParams(C.Structure):
    _fields_ = [
        ("max_age", C.c_int32), ("min_hits", C.c_int32),
        ("det_thresh", C.c_double), ("iou_threshold", C.c_double), ("min_box_area", C.c_double),
        ("aspect_ratio_thresh", C.c_double), ("lambda_iou", C.c_double),
        ("lambda_mhd", C.c_double), ("lambda_shape", C.c_double), ("dlo_boost_coef", C.c_double),
        ("use_ecc", C.c_int32), ("use_dlo_boost", C.c_int32), ("use_duo_boost", C.c_int32),
        ("s_sim_corr", C.c_int32), ("use_rich_s", C.c_int32), ("use_sb", C.c_int32),
        ("use_vt", C.c_int32),
    ]


class BxDeepocConfig(C.Structure):
    _fields_ = [
        ("n_seq", C.c_int32), ("track_cap", C.c_int32), ("det_cap", C.c_int32),
        ("emb_dim", C.c_int32), ("det_thresh", C.c_double), ("iou_threshold", C.c_double),
        ("inertia", C.c_double), ("q_xy_scaling", C.c_double), ("q_s_scaling", C.c_double),
        ("w_association_emb", C.c_double), ("alpha_fixed_emb", C.c_double),
        ("aw_param", C.c_double), ("max_age", C.c_int32), ("min_hits", C.c_int32),
        ("delta_t", C.c_int32), ("embedding_off", C.c_int32), ("aw_off", C.c_int32),
        ("asso_kind", C.c_int32), ("frame_w", C.c_double), ("frame_h", C.c_double),
    ]


class BxHybridConfig(C.Structure):
    _fields_ = [
        ("n_seq", C.c_int32), ("track_cap", C.c_int32), ("det_cap", C.c_int32),
        ("emb_dim", C.c_int32), ("det_thresh", C.c_double), ("iou_threshold", C.c_double),
        ("inertia", C.c_double), ("longterm_reid_weight", C.c_double),
        ("tcm_first_step_weight", C.c_double), ("max_age", C.c_int32), ("min_hits", C.c_int32),
        ("delta_t", C.c_int32), ("asso_kind", C.c_int32), ("frame_w", C.c_double),
        ("frame_h", C.c_double),
    ]


class BxDeepocSeqParams(C.Structure):
    _fields_ = [
        ("det_thresh", C.c_double), ("iou_threshold", C.c_double), ("inertia", C.c_double),
        ("q_xy_scaling", C.c_double), ("q_s_scaling", C.c_double),
        ("w_association_emb", C.c_double), ("alpha_fixed_emb", C.c_double),
        ("aw_param", C.c_double), ("max_age", C.c_int32), ("min_hits", C.c_int32),
        ("delta_t", C.c_int32), ("aw_off", C.c_int32), ("asso_kind", C.c_int32),
    ]


class BxHybridSeqParams(C.Structure):
    _fields_ = [
        ("det_thresh", C.c_double), ("iou_threshold", C.c_double), ("inertia", C.c_double),
        ("longterm_reid_weight", C.c_double), ("tcm_first_step_weight", C.c_double),
        ("max_age", C.c_int32), ("min_hits", C.c_int32), ("delta_t", C.c_int32),
        ("asso_kind", C.c_int32),
    ]


class BxSsConfig(C.Structure):
    _fields_ = [
        ("n_seq", C.c_int32), ("track_cap", C.c_int32), ("det_cap", C.c_int32),
        ("emb_dim", C.c_int32), ("vec_cap", C.c_int32), ("min_conf", C.c_double),
        ("max_cos_dist", C.c_double), ("max_iou_dist", C.c_double), ("max_age", C.c_int32),
        ("n_init", C.c_int32), ("nn_budget", C.c_int32), ("mc_lambda", C.c_double),
        ("ema_alpha", C.c_double), ("conf_thresh_high", C.c_double),
        ("conf_thresh_low", C.c_double), ("id_preservation_weight", C.c_double),
        ("crowd_detection", C.c_int32), ("born_confirmed", C.c_int32),
    ]


class BxSsSeqParams(C.Structure):
    _fields_ = [
        ("min_conf", C.c_double), ("max_cos_dist", C.c_double), ("max_iou_dist", C.c_double),
        ("max_age", C.c_int32), ("n_init", C.c_int32), ("nn_budget", C.c_int32),
        ("mc_lambda", C.c_double), ("ema_alpha", C.c_double), ("conf_thresh_high", C.c_double),
        ("conf_thresh_low", C.c_double), ("id_preservation_weight", C.c_double),
        ("crowd_detection", C.c_int32), ("born_confirmed", C.c_int32),
    ]


class BxSofParams(C.Structure):
    _fields_ = [
        ("max_corners", C.c_int32), ("win_size", C.c_int32), ("max_level", C.c_int32),
        ("max_iter", C.c_int32), ("quality_level", C.c_double), ("eps", C.c_double),
        ("threshold", C.c_double), ("scale", C.c_double),
    ]


# every symbol include/*.h declares (checked by tests/test_native_abi.py)
EXPORTS = [
    "bx_last_error", "bx_device_count", "bx_engine_create", "bx_engine_destroy",
    "bx_engine_reset", "bx_engine_step", "bx_engine_update_host", "bx_engine_status",
    "bx_engine_counters_host", "bx_engine_set_id_count", "bx_engine_tracks_host", "bx_engine_class_tracks_host",
    "bx_engine_state_set_host", "bx_ocsort_state_set_host", "bx_boost_state_set_host",
    "bx_ss_state_set_host",
    "bx_engine_probe", "bx_engine_probe_read", "bx_engine_set_overlap", "bx_engine_frame_stats_host",
    "bx_iou_batch", "bx_pairwise_cost", "bx_aw_max_metric", "bx_fuse_score", "bx_embedding_distance", "bx_kf_initiate",
    "bx_kf_multi_predict", "bx_kf_update", "bx_kf_gating_distance", "bx_linear_assignment", "bx_lapjv",
    "bx_linear_assignment_ex", "bx_engine_lap_ties_host", "bx_engine_lap_components_host", "bx_engine_set_lap_stats",
    "bx_engine_force_assoc_build", "bx_legacy_lap_pair", "bx_engine_set_early_features",
    "bx_engine_inputs_released", "bx_engine_set_cosine_mode", "bx_engine_embdist_host",
    "bx_engine_copy_state", "bx_engine_slots_used_host", "bx_ocsort_copy_state",
    "bx_engine_set_seq_params_host", "bx_engine_seq_params_host",
    "bx_boost_copy_state", "bx_ss_copy_state",
    "bx_boost_set_seq_params_host", "bx_boost_seq_params_host",
    "bx_ss_set_seq_params_host", "bx_ss_seq_params_host",
    "bx_ss_set_occlusion_host", "bx_ss_occlusion_host", "bx_ss_occlusion_buffer_host",
    "bx_pyset_order_host",
    "bx_nn_cosine_distance", "bx_ocsort_create", "bx_ocsort_destroy", "bx_ocsort_reset", "bx_ocsort_step",
    "bx_ocsort_update_host", "bx_ocsort_status", "bx_ocsort_counters_host",
    "bx_ocsort_set_id_count", "bx_ocsort_set_frame_size", "bx_ocsort_tracks_host", "bx_ocsort_probe", "bx_ocsort_probe_read",
    "bx_ocsort_frame_stats_host", "bx_ocsort_set_seq_params_host", "bx_ocsort_seq_params_host",
    "bx_boost_create", "bx_boost_destroy", "bx_boost_reset",
    "bx_boost_step", "bx_boost_update_host", "bx_boost_status", "bx_boost_counters_host",
    "bx_boost_set_id_count", "bx_boost_tracks_host", "bx_boost_frame_stats_host",
    "bx_boost_probe", "bx_boost_probe_read", "bx_ss_create", "bx_ss_destroy", "bx_ss_reset",
    "bx_ss_step", "bx_ss_update_host", "bx_ss_status", "bx_ss_counters_host",
    "bx_ss_tracks_host", "bx_ss_frame_stats_host", "bx_ss_probe", "bx_ss_probe_read",
    "bx_ss_set_lsap_mode", "bx_ss_lsap_stats_host", "bx_ss_lsap_op",
    "bx_txt_shape", "bx_txt_read", "bx_mot_format", "bx_mot_write",
    "bx_engine_update_classes_host", "bx_ocsort_update_classes_host",
    "bx_boost_update_classes_host", "bx_kf_xysr_initiate", "bx_kf_xysr_predict",
    "bx_kf_xysr_update", "bx_kf_boost_initiate", "bx_kf_boost_predict", "bx_kf_boost_update",
    "bx_kf_boost_mh_dist", "bx_ss_track_attrs_host", "bx_ss_track_attrs_set_host",
    "bx_ss_last_feature_host", "bx_ss_last_feature_set_host",
    "bx_deepoc_create", "bx_deepoc_destroy", "bx_deepoc_reset", "bx_deepoc_step",
    "bx_deepoc_update_host", "bx_deepoc_copy_state", "bx_deepoc_status",
    "bx_deepoc_counters_host", "bx_deepoc_set_id_count", "bx_deepoc_set_frame_size",
    "bx_deepoc_tracks_host", "bx_deepoc_state_set_host", "bx_deepoc_frame_stats_host",
    "bx_deepoc_probe", "bx_deepoc_probe_read", "bx_deepoc_embcost",
    "bx_deepoc_set_seq_params_host", "bx_deepoc_seq_params_host",
    "bx_hybrid_set_seq_params_host", "bx_hybrid_seq_params_host",
    "bx_feed_create_shared", "bx_feed_create_shared_fmt", "bx_feed_device_bytes",
    "bx_hybrid_create", "bx_hybrid_destroy", "bx_hybrid_reset", "bx_hybrid_step",
    "bx_hybrid_update_host", "bx_hybrid_copy_state", "bx_hybrid_status",
    "bx_hybrid_counters_host", "bx_hybrid_set_id_count", "bx_hybrid_set_frame_size",
    "bx_hybrid_tracks_host", "bx_hybrid_state_set_host", "bx_hybrid_state_bytes",
    "bx_hybrid_state_save_host", "bx_hybrid_state_load_host", "bx_hybrid_cosdist",
    "bx_hybrid_bank_mean",
    "bx_gsi_plan_workspace_bytes", "bx_gsi_interpolate_plan", "bx_gsi_interpolate",
    "bx_gsi_workspace_bytes", "bx_gsi_smooth", "bx_gsi_run_host",
    "bx_gsi_device_plan", "bx_gsi_device_run", "bx_gsi_device_free",
    "bx_feed_create", "bx_feed_destroy", "bx_feed_upload_host", "bx_feed_shape",
    "bx_feed_frame_runs", "bx_feed_run", "bx_feed_gather", "bx_feed_append", "bx_feed_status",
    "bx_feed_result_rows", "bx_feed_results_host", "bx_feed_results_device",
    "bx_feed_read_run_host", "bx_feed_write_run_host",
    "bx_classes_create", "bx_classes_destroy", "bx_classes_shape", "bx_classes_scratch",
    "bx_classes_split", "bx_classes_merge", "bx_classes_state", "bx_classes_reset",
    "bx_classes_status", "bx_classes_id_count_host", "bx_classes_set_id_count",
    "bx_classes_map_host", "bx_classes_copy_state",
    "bx_deepoc_step_classes", "bx_deepoc_classes_config", "bx_deepoc_classes",
    "bx_deepoc_update_classes_host", "bx_hybrid_step_classes", "bx_hybrid_classes_config",
    "bx_hybrid_classes", "bx_hybrid_update_classes_host", "bx_hybrid_probe",
    "bx_hybrid_probe_read",
    "bx_hybrid_set_ecc_host", "bx_hybrid_ecc_host", "bx_hybrid_step_cmc",
    "bx_hybrid_update_host_cmc", "bx_hybrid_step_classes_cmc",
    "bx_hybrid_update_classes_host_cmc",
    "bx_eval_create", "bx_eval_destroy", "bx_eval_capacity", "bx_eval_run_host",
    "bx_eval_set_gt_host", "bx_eval_run_device",
    "bx_ecc_create", "bx_ecc_destroy", "bx_ecc_reset", "bx_ecc_work_size", "bx_ecc_apply",
    "bx_ecc_apply_host", "bx_ecc_status", "bx_ecc_state_host",
    "bx_ecc_chain_reserve", "bx_ecc_apply_chain", "bx_ecc_apply_chain_host",
    "bx_reid_crops", "bx_reid_normalize",
    "bx_sof_create", "bx_sof_destroy", "bx_sof_reset", "bx_sof_levels", "bx_sof_apply",
    "bx_sof_apply_host", "bx_sof_status", "bx_sof_pyramid_bytes", "bx_sof_state_host",
    "bx_sof_points_host",
    "bx_sof_chain_reserve", "bx_sof_apply_chain", "bx_sof_apply_chain_host",
    "bx_det_letterbox", "bx_det_scratch_bytes", "bx_det_postprocess",
]

_vp, _ip, _dp, _fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float)

_SIGS = {
    "bx_last_error": ([], C.c_char_p),
    "bx_device_count": ([_ip], C.c_int),
    "bx_engine_create": ([C.POINTER(BxConfig), C.POINTER(C.c_void_p)], C.c_int),
    "bx_engine_destroy": ([_vp], C.c_int),
    "bx_engine_reset": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_engine_step": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_engine_update_host": ([_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _ip, _vp], C.c_int),
    "bx_engine_status": ([_vp, _ip], C.c_int),
    "bx_engine_probe": ([_vp, C.c_int], C.c_int),
    "bx_engine_set_overlap": ([_vp, C.c_int], C.c_int),
    "bx_engine_set_early_features": ([_vp, C.c_int], C.c_int),
    "bx_engine_probe_read": ([_vp, _dp, _ip], C.c_int),
    "bx_engine_frame_stats_host": ([_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "bx_engine_counters_host": ([_vp, C.c_int, _ip, _ip, _ip, _ip], C.c_int),
    "bx_engine_set_id_count": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_engine_tracks_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ip,
                               _ip], C.c_int),
    "bx_engine_class_tracks_host": ([_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp], C.c_int),
    "bx_iou_batch": ([_vp, C.c_int, _vp, C.c_int, _vp, _vp], C.c_int),
    "bx_pairwise_cost": ([C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_double,
                          C.c_double, _vp, _vp], C.c_int),
    "bx_txt_shape": ([C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)], C.c_int),
    "bx_txt_read": ([C.c_char_p, _vp, C.c_int64, C.c_int32], C.c_int),
    "bx_mot_format": ([_vp, C.c_int64, C.c_int32, C.c_int32, _vp], C.c_int),
    "bx_mot_write": ([C.c_char_p, _vp, C.c_int64, C.c_int32], C.c_int),
    "bx_aw_max_metric": ([_vp, C.c_int, C.c_int, C.c_double, C.c_double, _vp, _vp], C.c_int),
    "bx_fuse_score": ([_vp, C.c_int, C.c_int, _vp, _vp], C.c_int),
    "bx_embedding_distance": ([_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp], C.c_int),
    "bx_kf_initiate": ([C.c_int, C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_kf_multi_predict": ([C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_kf_update": ([C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_kf_gating_distance": ([C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp], C.c_int),
    "bx_linear_assignment": ([_vp, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp], C.c_int),
    "bx_linear_assignment_ex": ([_vp, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp], C.c_int),
    "bx_engine_lap_ties_host": ([_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "bx_engine_lap_components_host": ([_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "bx_engine_set_lap_stats": ([_vp, C.c_int], C.c_int),
    "bx_engine_force_assoc_build": ([_vp, C.c_int], C.c_int),
    "bx_legacy_lap_pair": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_engine_inputs_released": ([_vp, _vp], C.c_int),
    "bx_engine_set_cosine_mode": ([_vp, C.c_int], C.c_int),
    "bx_engine_embdist_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _ip], C.c_int),
    "bx_engine_copy_state": ([_vp, _vp], C.c_int),
    "bx_engine_set_seq_params_host": ([_vp, C.c_int, C.c_int, C.POINTER(BxEngineSeqParams), _vp],
                                      C.c_int),
    "bx_engine_seq_params_host": ([_vp, C.c_int, C.POINTER(BxEngineSeqParams)], C.c_int),
    "bx_ocsort_copy_state": ([_vp, _vp], C.c_int),
    "bx_boost_copy_state": ([_vp, _vp], C.c_int),
    "bx_boost_set_seq_params_host": ([_vp, C.c_int, C.c_int, C.POINTER(BxBoostSeqParams), _vp],
                                     C.c_int),
    "bx_boost_seq_params_host": ([_vp, C.c_int, C.POINTER(BxBoostSeqParams)], C.c_int),
    "bx_ss_copy_state": ([_vp, _vp], C.c_int),
    "bx_ss_set_seq_params_host": ([_vp, C.c_int, C.c_int, C.POINTER(BxSsSeqParams), _vp], C.c_int),
    "bx_ss_seq_params_host": ([_vp, C.c_int, C.POINTER(BxSsSeqParams)], C.c_int),
    "bx_ss_set_occlusion_host": ([_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp], C.c_int),
    "bx_ss_occlusion_host": ([_vp, C.c_int, _ip, _dp, _ip, _ip], C.c_int),
    "bx_ss_occlusion_buffer_host": ([_vp, C.c_int, C.c_int, _vp, _ip], C.c_int),
    "bx_pyset_order_host": ([_vp, C.c_int, _vp, _ip], C.c_int),
    "bx_engine_slots_used_host": ([_vp, C.c_int, _ip], C.c_int),
    "bx_lapjv": ([_vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp], C.c_int),
    "bx_nn_cosine_distance": ([_vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp,
                               _vp], C.c_int),
    "bx_ocsort_create": ([C.POINTER(BxOcsortConfig), C.POINTER(C.c_void_p)], C.c_int),
    "bx_ocsort_destroy": ([_vp], C.c_int),
    "bx_ocsort_reset": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_ocsort_step": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_ocsort_update_host": ([_vp, C.c_int, _vp, C.c_int, _vp, _ip, _vp], C.c_int),
    "bx_ocsort_status": ([_vp, _ip], C.c_int),
    "bx_ocsort_counters_host": ([_vp, C.c_int, _ip, _ip, _ip], C.c_int),
    "bx_ocsort_set_id_count": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_ocsort_set_frame_size": ([_vp, C.c_int, C.c_double, C.c_double, _vp], C.c_int),
    "bx_ocsort_tracks_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _ip], C.c_int),
    "bx_ocsort_probe": ([_vp, C.c_int], C.c_int),
    "bx_ocsort_frame_stats_host": ([_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "bx_ocsort_probe_read": ([_vp, _dp, _ip], C.c_int),
    "bx_ocsort_set_seq_params_host": ([_vp, C.c_int, C.c_int, C.POINTER(BxOcsortSeqParams), _vp],
                                      C.c_int),
    "bx_ocsort_seq_params_host": ([_vp, C.c_int, C.POINTER(BxOcsortSeqParams)], C.c_int),
    "bx_boost_create": ([C.POINTER(BxBoostConfig), C.POINTER(C.c_void_p)], C.c_int),
    "bx_boost_destroy": ([_vp], C.c_int),
    "bx_boost_reset": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_boost_step": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_boost_update_host": ([_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _ip, _vp], C.c_int),
    "bx_boost_status": ([_vp, _ip], C.c_int),
    "bx_boost_counters_host": ([_vp, C.c_int, _ip, _ip, _ip], C.c_int),
    "bx_boost_set_id_count": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_boost_tracks_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _ip], C.c_int),
    "bx_boost_frame_stats_host": ([_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "bx_boost_probe": ([_vp, C.c_int], C.c_int),
    "bx_boost_probe_read": ([_vp, _dp, _ip], C.c_int),
    "bx_ss_create": ([C.POINTER(BxSsConfig), C.POINTER(C.c_void_p)], C.c_int),
    "bx_ss_destroy": ([_vp], C.c_int),
    "bx_ss_reset": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_ss_step": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_ss_update_host": ([_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _ip, _vp], C.c_int),
    "bx_ss_status": ([_vp, _ip], C.c_int),
    "bx_ss_counters_host": ([_vp, C.c_int, _ip, _ip, _ip, _ip], C.c_int),
    "bx_ss_tracks_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _ip], C.c_int),
    "bx_engine_state_set_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_ocsort_state_set_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_boost_state_set_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_ss_state_set_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_ss_frame_stats_host": ([_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "bx_ss_set_lsap_mode": ([_vp, C.c_int], C.c_int),
    "bx_ss_lsap_op": ([_vp, C.c_int, C.c_int, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp],
                      C.c_int),
    "bx_ss_lsap_stats_host": ([_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "bx_ss_probe": ([_vp, C.c_int], C.c_int),
    "bx_ss_probe_read": ([_vp, _dp, _ip], C.c_int),
    "bx_engine_update_classes_host": ([_vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _ip,
                                       _vp], C.c_int),
    "bx_ocsort_update_classes_host": ([_vp, C.c_int, C.c_int, _vp, C.c_int, _ip, _vp, _ip, _vp],
                                      C.c_int),
    "bx_boost_update_classes_host": ([_vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _ip,
                                      _vp], C.c_int),
    "bx_kf_xysr_initiate": ([C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_kf_xysr_predict": ([C.c_int, _vp, _vp, C.c_double, C.c_double, _vp], C.c_int),
    "bx_kf_xysr_update": ([C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_kf_boost_initiate": ([C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_kf_boost_predict": ([C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_kf_boost_update": ([C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_kf_boost_mh_dist": ([C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_ss_track_attrs_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _ip], C.c_int),
    "bx_ss_track_attrs_set_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_ss_last_feature_host": ([_vp, C.c_int, C.c_int, _vp, _vp], C.c_int),
    "bx_ss_last_feature_set_host": ([_vp, C.c_int, C.c_int, _vp, _vp, C.c_int], C.c_int),
    "bx_deepoc_create": ([C.POINTER(BxDeepocConfig), C.POINTER(C.c_void_p)], C.c_int),
    "bx_deepoc_destroy": ([_vp], C.c_int),
    "bx_deepoc_reset": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_deepoc_step": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_deepoc_update_host": ([_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _ip, _vp], C.c_int),
    "bx_deepoc_copy_state": ([_vp, _vp], C.c_int),
    "bx_deepoc_status": ([_vp, _ip], C.c_int),
    "bx_deepoc_counters_host": ([_vp, C.c_int, _ip, _ip, _ip], C.c_int),
    "bx_deepoc_set_id_count": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_deepoc_set_frame_size": ([_vp, C.c_int, C.c_double, C.c_double, _vp], C.c_int),
    "bx_deepoc_tracks_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _ip], C.c_int),
    "bx_deepoc_state_set_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_deepoc_frame_stats_host": ([_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "bx_deepoc_probe": ([_vp, C.c_int], C.c_int),
    "bx_deepoc_probe_read": ([_vp, _dp, _ip], C.c_int),
    "bx_deepoc_embcost": ([C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_deepoc_set_seq_params_host": ([_vp, C.c_int, C.c_int, C.POINTER(BxDeepocSeqParams), _vp],
                                      C.c_int),
    "bx_deepoc_seq_params_host": ([_vp, C.c_int, C.POINTER(BxDeepocSeqParams)], C.c_int),
    "bx_hybrid_set_seq_params_host": ([_vp, C.c_int, C.c_int, C.POINTER(BxHybridSeqParams), _vp],
                                      C.c_int),
    "bx_hybrid_seq_params_host": ([_vp, C.c_int, C.POINTER(BxHybridSeqParams)], C.c_int),
    "bx_hybrid_create": ([C.POINTER(BxHybridConfig), C.POINTER(C.c_void_p)], C.c_int),
    "bx_hybrid_destroy": ([_vp], C.c_int),
    "bx_hybrid_reset": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_hybrid_step": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_hybrid_update_host": ([_vp, C.c_int, _vp, C.c_int, _vp, _vp, _ip, _vp], C.c_int),
    "bx_hybrid_copy_state": ([_vp, _vp], C.c_int),
    "bx_hybrid_status": ([_vp, _ip], C.c_int),
    "bx_hybrid_counters_host": ([_vp, C.c_int, _ip, _ip, _ip], C.c_int),
    "bx_hybrid_set_id_count": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_hybrid_set_frame_size": ([_vp, C.c_int, C.c_double, C.c_double, _vp], C.c_int),
    "bx_hybrid_tracks_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ip],
                              C.c_int),
    "bx_hybrid_state_set_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_hybrid_state_bytes": ([_vp, C.POINTER(C.c_size_t)], C.c_int),
    "bx_hybrid_state_save_host": ([_vp, C.c_int, _vp, C.c_size_t], C.c_int),
    "bx_hybrid_state_load_host": ([_vp, C.c_int, _vp, C.c_size_t], C.c_int),
    "bx_hybrid_cosdist": ([C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_hybrid_bank_mean": ([C.c_int, C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "bx_gsi_plan_workspace_bytes": ([C.c_int64, C.POINTER(C.c_size_t)], C.c_int),
    "bx_gsi_interpolate_plan": ([_vp, _vp, C.c_int64, C.c_int, C.c_int, _vp, C.c_size_t, _vp,
                                 _vp], C.c_int),
    "bx_gsi_interpolate": ([_vp, C.c_int64, C.c_int, _vp, _vp, _vp, C.c_int64, _vp, _vp],
                           C.c_int),
    "bx_gsi_workspace_bytes": ([_vp, C.c_int, C.c_int, C.POINTER(C.c_size_t)], C.c_int),
    "bx_gsi_smooth": ([_vp, C.c_int, _vp, C.c_int, C.c_double, C.c_int, _vp, C.c_size_t, _vp,
                       _vp, _vp], C.c_int),
    "bx_gsi_run_host": ([_vp, C.c_int64, C.c_int, C.c_int, C.c_double, _vp, C.c_int64,
                         C.POINTER(C.c_int64), _vp], C.c_int),
    "bx_gsi_device_plan": ([_vp, C.c_int64, _vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_int64),
                            C.POINTER(C.c_void_p), _vp], C.c_int),
    "bx_gsi_device_run": ([_vp, C.c_double, C.c_int, _vp, C.c_int64, _vp, _vp, _vp], C.c_int),
    "bx_gsi_device_free": ([_vp], C.c_int),
    "bx_feed_create": ([C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                        C.POINTER(C.c_void_p)], C.c_int),
    "bx_feed_create_shared": ([C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp,
                               C.POINTER(C.c_void_p)], C.c_int),
    "bx_feed_create_shared_fmt": ([C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp,
                                   C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "bx_feed_device_bytes": ([_vp, C.POINTER(C.c_int64)], C.c_int),
    "bx_feed_destroy": ([_vp], C.c_int),
    "bx_feed_upload_host": ([_vp, C.c_int, _vp, _vp], C.c_int),
    "bx_feed_shape": ([_vp, _ip, _ip], C.c_int),
    "bx_feed_frame_runs": ([_vp, C.c_int, _ip], C.c_int),
    "bx_feed_run": ([_vp, C.c_int, C.c_int, _ip, _ip, _ip] + [C.POINTER(C.c_void_p)] * 5, C.c_int),
    "bx_feed_gather": ([_vp, C.c_int, _vp], C.c_int),
    "bx_feed_append": ([_vp, C.c_int, _vp], C.c_int),
    "bx_feed_status": ([_vp, _ip], C.c_int),
    "bx_feed_result_rows": ([_vp, C.POINTER(C.c_int64)], C.c_int),
    "bx_feed_results_host": ([_vp, _vp, _vp, _vp], C.c_int),
    "bx_feed_results_device": ([_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                C.POINTER(C.c_int64)], C.c_int),
    "bx_feed_read_run_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_feed_write_run_host": ([_vp, C.c_int, C.c_int, _vp, _vp], C.c_int),
    "bx_classes_create": ([C.c_int] * 6 + [C.POINTER(C.c_void_p)], C.c_int),
    "bx_classes_destroy": ([_vp], C.c_int),
    "bx_classes_shape": ([_vp, _ip, _ip, _ip, _ip, _ip, _ip], C.c_int),
    "bx_classes_scratch": ([_vp] + [C.POINTER(C.c_void_p)] * 6, C.c_int),
    "bx_classes_split": ([_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_classes_merge": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp],
                         C.c_int),
    "bx_classes_state": ([_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)], C.c_int),
    "bx_classes_reset": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_classes_status": ([_vp, _ip], C.c_int),
    "bx_classes_id_count_host": ([_vp, C.c_int, _ip], C.c_int),
    "bx_classes_set_id_count": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_classes_map_host": ([_vp, C.c_int, C.c_int, C.c_int, _vp, _ip], C.c_int),
    "bx_classes_copy_state": ([_vp, _vp], C.c_int),
    "bx_deepoc_step_classes": ([_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
                               C.c_int),
    "bx_deepoc_classes_config": ([_vp, C.c_int, C.c_int], C.c_int),
    "bx_deepoc_classes": ([_vp, C.POINTER(C.c_void_p)], C.c_int),
    "bx_deepoc_update_classes_host": ([_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _ip, _vp,
                                       _ip, _vp], C.c_int),
    "bx_hybrid_step_classes": ([_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp],
                               C.c_int),
    "bx_hybrid_probe": ([_vp, C.c_int], C.c_int),
    "bx_hybrid_probe_read": ([_vp, _dp, _ip], C.c_int),
    "bx_hybrid_classes_config": ([_vp, C.c_int, C.c_int], C.c_int),
    "bx_hybrid_classes": ([_vp, C.POINTER(C.c_void_p)], C.c_int),
    "bx_hybrid_update_classes_host": ([_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _ip, _vp, _ip,
                                       _vp], C.c_int),
    "bx_hybrid_set_ecc_host": ([_vp, C.c_int, C.c_int, _vp], C.c_int),
    "bx_hybrid_ecc_host": ([_vp, C.c_int, _ip, _ip], C.c_int),
    "bx_hybrid_step_cmc": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_hybrid_update_host_cmc": ([_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _ip, _vp],
                                  C.c_int),
    "bx_hybrid_step_classes_cmc": ([_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp], C.c_int),
    "bx_hybrid_update_classes_host_cmc": ([_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _ip,
                                           _vp, _ip, _vp], C.c_int),
    "bx_eval_create": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "bx_eval_destroy": ([_vp], C.c_int),
    "bx_eval_capacity": ([_vp, _ip, _ip, _ip, _ip], C.c_int),
    "bx_eval_run_host": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_eval_set_gt_host": ([_vp, C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_eval_run_device": ([_vp, C.c_int, C.c_int, _vp, C.c_int64, _vp, _vp, _vp, _vp], C.c_int),
    "bx_ecc_create": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "bx_ecc_destroy": ([_vp], C.c_int),
    "bx_ecc_reset": ([_vp, C.c_int, _vp], C.c_int),
    "bx_ecc_work_size": ([C.c_int, C.c_int, C.c_double, _ip, _ip], C.c_int),
    "bx_ecc_apply": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_double,
                      C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_ecc_apply_host": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_double,
                           C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_ecc_chain_reserve": ([_vp, C.c_int], C.c_int),
    "bx_ecc_apply_chain": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int,
                            C.c_double, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_ecc_apply_chain_host": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int,
                                 C.c_double, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp],
                                C.c_int),
    "bx_ecc_status": ([_vp, _ip], C.c_int),
    "bx_ecc_state_host": ([_vp, C.c_int, _ip, _ip, _ip, _vp, _vp, _vp], C.c_int),
    "bx_reid_crops": ([_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]
                      + [C.c_float] * 6 + [C.c_int, _vp, _vp, _vp], C.c_int),
    "bx_reid_normalize": ([_vp, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, C.c_int, _vp], C.c_int),
    "bx_sof_create": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "bx_sof_destroy": ([_vp], C.c_int),
    "bx_sof_reset": ([_vp, C.c_int, _vp], C.c_int),
    "bx_sof_levels": ([C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip], C.c_int),
    "bx_sof_apply": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.POINTER(BxSofParams),
                      _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_sof_apply_host": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp,
                           C.POINTER(BxSofParams), _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_sof_status": ([_vp, _ip], C.c_int),
    "bx_sof_pyramid_bytes": ([_vp, C.POINTER(C.c_size_t)], C.c_int),
    "bx_sof_state_host": ([_vp, C.c_int, _ip, _ip, _ip, _ip, _vp, _ip, _vp, _vp], C.c_int),
    "bx_sof_points_host": ([_vp, C.c_int, _ip, _vp, _vp, _vp, _vp, _vp, _ip], C.c_int),
    "bx_sof_chain_reserve": ([_vp, C.c_int], C.c_int),
    "bx_sof_apply_chain": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp,
                            C.POINTER(BxSofParams), _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_sof_apply_chain_host": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp,
                                 C.POINTER(BxSofParams), _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "bx_det_letterbox": ([_vp] + [C.c_int] * 7 + [C.c_double] * 6 + [C.c_int, _vp, _vp], C.c_int),
    "bx_det_scratch_bytes": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)], C.c_int),
    "bx_det_postprocess": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_float,
                            C.c_float, _vp, _vp, C.c_int, C.c_int, C.c_int] + [_vp] * 7, C.c_int),
}

_lib = None


def load(path: Path | None = None):
    """Load libbxassoc.so (raises NativeUnavailable when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    # BX_LIB_PATH: load a diagnostic build (e.g. the -DBX_PHASE_TIMING stamps library)
    p = Path(path) if path else Path(os.environ.get("BX_LIB_PATH", LIB_PATH))
    if not p.exists():
        raise NativeUnavailable(
            f"{p} is missing: build the HIP extension first (python -c 'import __graft_entry__ "
            "as g; g.build()' or boxmot_amd._native.build())")
    L = C.CDLL(str(p))
    for name, (args, res) in _SIGS.items():
        fn = getattr(L, name, None)
        if fn is None and not path and "BX_LIB_PATH" in os.environ:
            continue  # (an older diagnostic build for an A/B: entry points it predates stay unset)
        if fn is None:
            raise NativeUnavailable(f"{p} does not export {name}: rebuild the HIP extension")
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


STATUS = {0: "ok", 1: "invalid argument", 2: "capacity exceeded", 3: "track slots exhausted",
          4: "HIP error", 5: "no HIP device", 6: "shape mismatch"}


def check(rc: int, what: str = ""):
    if rc == 0:
        return
    msg = load().bx_last_error().decode(errors="replace")
    text = f"{what}: {STATUS.get(rc, rc)} ({msg})"
    if rc == 5:
        raise NativeUnavailable(text)
    if rc in (1, 2, 6):
        raise ValueError(text)
    raise RuntimeError(text)


def device_count() -> int:
    n = C.c_int(0)
    load().bx_device_count(C.byref(n))
    return n.value

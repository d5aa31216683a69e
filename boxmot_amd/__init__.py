"""boxmot_amd — MI355X-native per-frame association engine for BoxMOT trackers.

Drop-in surface: ``create_tracker``, ``get_tracker_config``, ``ByteTrack``, ``BotSort``, ``OcSort``, ``BoostTrack``, ``StrongSort``, ``DeepOcSort``, ``HybridSort`` (and their per_class forms
``DeepOcSortPerClass``, ``HybridSortPerClass``) with the
reference's ``update(dets, img, embs) -> [M, 8]`` contract.  The numerics run in libbxassoc.so
(HIP, gfx950); ``boxmot_amd.engine.Engine`` (``TableEngine``: per-sequence parameters) / ``OcsortEngine`` (``OcsortTableEngine``: per-sequence parameters) / ``BoostEngine`` (``BoostTableEngine``: per-sequence parameters) / ``SsEngine`` (``SsTableEngine``: per-sequence parameters) / ``DeepOcsortEngine`` / ``HybridsortEngine`` expose the batched many-sequence API.
``gsi`` / ``linear_interpolation`` / ``gaussian_smooth`` are the GSI post-processing of MOT result files; ``gsi_device`` applies it to result rows in device memory.
``evaluate_mot`` / ``mot_summary`` are the HOTA / CLEAR / Identity evaluation of MOT result files.
``ECC`` / ``EccBatch`` / ``SOF`` / ``SofBatch`` / ``get_cmc_method`` are the camera-motion
compensation from images; ``EccChain`` / ``warp_table`` and ``SofChain`` / ``sof_warp_table`` run
many consecutive frames of a camera per call, for the many-sequence file flow
(``motio.run_sequences(images=..., cmc=...)``).
``tune.grid`` / ``tune.sweep`` run a hyper-parameter sweep (K configs x S sequences) as one batched OCSort engine; ``tune.sweep_reid`` does it for DeepOCSort / HybridSort, ``tune.sweep_bot`` for ByteTrack / BoT-SORT, ``tune.sweep_boost`` for BoostTrack and ``tune.sweep_strong`` for StrongSort; ``tune.sweep_gsi`` runs any of them with GSI applied before the rows are scored or written.
``ReidFrontEnd`` / ``crop_batch`` / ``normalize_features`` are the ReID front end around the caller's network.
``DetFrontEnd`` / ``letterbox`` / ``postprocess`` are the detector front end around the caller's network: letterbox in, score filter, batched NMS and rescale out.
"""
from .cmc import (MOTION_AFFINE, MOTION_EUCLIDEAN, MOTION_HOMOGRAPHY, MOTION_TRANSLATION, ECC,
                  EccBatch, EccChain, SOF, SofBatch, SofChain, get_cmc_method, sof_warp_table,
                  warp_table)
from . import tune
from .det import DetFrontEnd, letterbox, postprocess
from .evaluation import evaluate_mot, evaluate_mot_device, mot_summary
from .postprocessing import gaussian_smooth, gsi, gsi_device, linear_interpolation
from .reid import ReidFrontEnd, crop_batch, normalize_features
from .tracker_zoo import create_tracker, get_tracker_config
from .trackers import (BoostTrack, BotSort, ByteTrack, DeepOcSort, DeepOcSortPerClass,
                       HybridSort, HybridSortPerClass, OcSort, StrongSort)

__version__ = "0.1.0"
__all__ = ["create_tracker", "get_tracker_config", "ByteTrack", "BotSort", "OcSort",
           "BoostTrack", "StrongSort", "DeepOcSort", "HybridSort", "gsi", "linear_interpolation",
           "gaussian_smooth", "gsi_device", "DeepOcSortPerClass", "HybridSortPerClass", "evaluate_mot",
           "evaluate_mot_device",
           "mot_summary", "ECC", "EccBatch", "EccChain", "warp_table", "SOF", "SofBatch", "SofChain",
           "sof_warp_table", "get_cmc_method", "MOTION_TRANSLATION",
           "MOTION_EUCLIDEAN", "MOTION_AFFINE", "MOTION_HOMOGRAPHY", "ReidFrontEnd",
           "crop_batch", "normalize_features", "DetFrontEnd", "letterbox", "postprocess", "tune",
           "__version__"]

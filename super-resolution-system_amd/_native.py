"""ctypes binding of include/sr_hip.h (libsrhip.so) -- the only way the Python host code
reaches the GPU.  There is deliberately no CPU fallback: if the library or a device is missing,
the compute entry points raise (SrNativeError), they never route through oracle/.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SR_LIB_PATH") or os.path.join(_HERE, "libsrhip.so")   # SR_LIB_PATH: an experiment build

SR_OK = 0
SR_ERR_INVALID_ARG, SR_ERR_SHAPE, SR_ERR_OOM, SR_ERR_HIP, SR_ERR_COMM, SR_ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6
PAD_MODES = {"mirror": 0, "replicate": 1, "reflect": 2, "constant": 3}
WEIGHT_TYPES = {"linear": 0, "cosine": 1, "sigmoid": 2, "ones": 3}
SSIM_MODES = {"uniform": 0, "gauss": 1, "simple": 2}
SR_U8, SR_F32, SR_F64 = 0, 1, 2
# sr_poisson_max_side(): the longest side sr_poisson_clone_u8 solves (sr_fft_max_len() / 2 + 1); tests/test_poisson_host.py
# holds it against the library's answer
POISSON_MAX_SIDE = 16385


class SrNativeError(RuntimeError):
    """HIP / library failure (SR_ERR_HIP, SR_ERR_OOM, SR_ERR_COMM, SR_ERR_UNSUPPORTED)."""


class SrShapeError(ValueError):
    """SR_ERR_SHAPE: the reference raises cv2.error / ValueError for these."""


class Xfer(C.Structure):
    _fields_ = [("peer", C.c_int), ("d_ptr", C.c_void_p), ("bytes", C.c_uint64)]


class TileRect(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class MergeTile(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("x", "y", "src_w", "src_h", "out_w", "out_h",
                                        "ov_t", "ov_b", "ov_l", "ov_r")]


class SeamRecord(C.Structure):
    _fields_ = [("tile", C.c_int), ("x", C.c_int), ("y", C.c_int), ("pad", C.c_int), ("score", C.c_double)]


class AssessSums(C.Structure):
    _fields_ = [("sse", C.c_double), ("ssim_uniform", C.c_double), ("ssim_gauss", C.c_double),
                ("ssim_simple", C.c_double)]


ASSESS_SSE, ASSESS_UNIFORM7, ASSESS_GAUSS11, ASSESS_SIMPLE, ASSESS_ALL = 1, 2, 4, 8, 15


class QualityCell(C.Structure):
    _fields_ = [("sse", C.c_uint64), ("ssim_uniform", C.c_double), ("ssim_gauss", C.c_double), ("ssim_simple", C.c_double)]


class MsSsimLevel(C.Structure):
    """sr_ms_ssim_level (include/sr_hip.h)."""
    _fields_ = [("sum_lcs", C.c_double), ("sum_cs", C.c_double), ("count", C.c_uint64)]


class BenchSums(C.Structure):
    """sr_bench_sums (include/sr_hip.h)."""
    _fields_ = [("sse", C.c_double), ("ssim_sum", C.c_double), ("n_elems", C.c_uint64), ("n_map", C.c_uint64)]


class VifScale(C.Structure):
    """sr_vif_scale (include/sr_hip.h)."""
    _fields_ = [("num", C.c_double), ("den", C.c_double), ("count", C.c_uint64)]


class GmsdSums(C.Structure):
    """sr_gmsd_sums (include/sr_hip.h)."""
    _fields_ = [("sum_d", C.c_double), ("sum_d2", C.c_double), ("count", C.c_uint64)]


class FsimSums(C.Structure):
    """sr_fsim_sums (include/sr_hip.h)."""
    _fields_ = [("sum_s", C.c_double), ("sum_sc", C.c_double), ("sum_pcm", C.c_double), ("count", C.c_uint64),
                ("F", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("reserved", C.c_int32)]


class VsiSums(C.Structure):
    """sr_vsi_sums (include/sr_hip.h)."""
    _fields_ = [("sum_s", C.c_double), ("sum_w", C.c_double), ("count", C.c_uint64),
                ("F", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("reserved", C.c_int32),
                ("a_range", C.c_double * 2 * 2), ("b_range", C.c_double * 2 * 2), ("vs_range", C.c_double * 2 * 2)]


VSI_GRID = 256
DELTA_E_BINS = 2048


class DeltaESums(C.Structure):
    """sr_delta_e_sums (include/sr_hip.h)."""
    _fields_ = [("count", C.c_uint64), ("sum", C.c_double), ("sum2", C.c_double), ("max", C.c_double),
                ("hist", C.c_uint64 * DELTA_E_BINS)]


class DeltaECell(C.Structure):
    """sr_delta_e_cell (include/sr_hip.h)."""
    _fields_ = [("sum", C.c_double), ("max", C.c_double)]


class HaarPsiSums(C.Structure):
    """sr_haarpsi_sums (include/sr_hip.h)."""
    _fields_ = [("num", C.c_double * 3), ("den", C.c_double * 3), ("channels", C.c_int32), ("reserved", C.c_int32),
                ("count", C.c_uint64)]


class HaarPsiCell(C.Structure):
    """sr_haarpsi_cell (include/sr_hip.h)."""
    _fields_ = [("num", C.c_double), ("den", C.c_double)]


class MserParams(C.Structure):
    """sr_mser_params (include/sr_hip.h)."""
    _fields_ = [("delta", C.c_int), ("min_area", C.c_int), ("max_area", C.c_int), ("max_variation", C.c_double),
                ("min_diversity", C.c_double)]


MSER_REGION_FIELDS = ("polarity", "level", "area", "x0", "y0", "x1", "y1", "seed", "S")
MSER_NODE_FIELDS = ("level", "area", "x0", "y0", "x1", "y1", "seed", "parent_level", "parent_seed")
# sr_mser_region / sr_mser_node (include/sr_hip.h) as structured dtypes: nine int32 each
MSER_REGION_DTYPE = np.dtype([(f, np.int32) for f in MSER_REGION_FIELDS])
MSER_NODE_DTYPE = np.dtype([(f, np.int32) for f in MSER_NODE_FIELDS])
MSER_DARK, MSER_BRIGHT, MSER_BOTH = 1, 2, 3               # polarity_mask bits


class CascadeInfo(C.Structure):
    """sr_cascade_info (include/sr_hip.h)."""
    _fields_ = [(k, C.c_int) for k in ("feature_type", "win_w", "win_h", "n_stages", "n_stumps", "n_features", "old_layout",
                                      "stage_type", "max_tree_nodes", "tilted", "max_rects", "max_cat_count")]


class CascadeParams(C.Structure):
    """sr_cascade_params (include/sr_hip.h)."""
    _fields_ = [("scale_factor", C.c_double), ("min_neighbors", C.c_int), ("min_w", C.c_int), ("min_h", C.c_int),
                ("max_w", C.c_int), ("max_h", C.c_int)]


class CascadeScale(C.Structure):
    """sr_cascade_scale (include/sr_hip.h)."""
    _fields_ = [("f", C.c_double)] + [(k, C.c_int) for k in ("win_w", "win_h", "sw", "sh", "step", "nx", "ny")]


SR_CASCADE_MAX_SCALES = 128
CASCADE_RECT_DTYPE = np.dtype([(f, np.int32) for f in ("x", "y", "w", "h")])      # sr_tile_rect


# enum sr_haarpsi_convention (include/sr_hip.h)
HAARPSI_MATLAB, HAARPSI_PYTHON = 0, 1
HAARPSI_CONVENTIONS = {"matlab": HAARPSI_MATLAB, "python": HAARPSI_PYTHON}
# enum sr_delta_e_formula (include/sr_hip.h)
DELTA_E_2000, DELTA_E_76 = 0, 1
DELTA_E_FORMULAS = {"ciede2000": DELTA_E_2000, "cie76": DELTA_E_76}
VIF_SCALES = 4
# enum sr_bench_mode (include/sr_hip.h)
BENCH_CHANNELS, BENCH_Y, BENCH_Y_ROUND = 0, 1, 2
# enum sr_imresize_out (include/sr_hip.h) and the element type each writes
IMRESIZE_U8, IMRESIZE_F32, IMRESIZE_F64 = 0, 1, 2
IMRESIZE_DTYPES = {IMRESIZE_U8: np.uint8, IMRESIZE_F32: np.float32, IMRESIZE_F64: np.float64}
IMRESIZE_MAX_TAPS = 66


class NiqeMoments(C.Structure):
    """sr_niqe_moments (include/sr_hip.h)."""
    _fields_ = [("n_neg", C.c_uint64), ("n_pos", C.c_uint64), ("ssq_neg", C.c_double), ("ssq_pos", C.c_double), ("sabs", C.c_double)]


class NiqeBlock(C.Structure):
    """sr_niqe_block (include/sr_hip.h)."""
    _fields_ = [("x", NiqeMoments * 5), ("sum_sigma", C.c_double)]


# the same records as NumPy structured arrays
NIQE_MOMENTS = np.dtype([("n_neg", "<u8"), ("n_pos", "<u8"), ("ssq_neg", "<f8"), ("ssq_pos", "<f8"), ("sabs", "<f8")])
NIQE_RECORD = np.dtype([("x", NIQE_MOMENTS, (5,)), ("sum_sigma", "<f8")])
NIQE_BLOCK, NIQE_FEATURES = 96, 36
# sr_brisque_record (include/sr_hip.h): one per scale
BRISQUE_RECORD = np.dtype([("n", "<u8"), ("x", NIQE_MOMENTS, (5,))])
BRISQUE_FEATURES, BRISQUE_MIN_SIDE = 36, 16

MS_SSIM_MAX_LEVELS = 5
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


# metric bits of sr_commercial_u8 (include/sr_hip.h)
(CM_LAPG, CM_NOISE, CM_SOBEL, CM_MSCN, CM_TEX, CM_LAB, CM_SKIN, CM_RGB, CM_BLOCKS, CM_REGIONS, CM_CANNY,
 CM_HF) = (1 << i for i in range(12))


class ResNetDesc(C.Structure):
    """sr_resnet_desc (include/sr_hip.h)."""
    _fields_ = [("n_feat", C.c_int), ("n_blocks", C.c_int), ("scale", C.c_int), ("long_skip", C.c_int), ("conv_hr", C.c_int),
                ("bilinear_base", C.c_int), ("a_head", C.c_float), ("a_up", C.c_float), ("a_hr", C.c_float),
                ("res_scale", C.c_float), ("mean", C.c_float * 3), ("range", C.c_float)]


class RrdbDesc(C.Structure):
    """sr_rrdb_desc (include/sr_hip.h)."""
    _fields_ = [("n_feat", C.c_int), ("n_grow", C.c_int), ("n_blocks", C.c_int), ("scale", C.c_int), ("slope", C.c_float),
                ("res_scale", C.c_float)]


class RcanDesc(C.Structure):
    """sr_rcan_desc (include/sr_hip.h)."""
    _fields_ = [("n_feat", C.c_int), ("n_squeeze", C.c_int), ("n_groups", C.c_int), ("n_blocks", C.c_int), ("scale", C.c_int),
                ("res_scale", C.c_float), ("mean", C.c_float * 3), ("range", C.c_float)]


class SwinirDesc(C.Structure):
    """sr_swinir_desc (include/sr_hip.h)."""
    _fields_ = [("n_feat", C.c_int), ("n_heads", C.c_int), ("n_hidden", C.c_int), ("n_groups", C.c_int), ("depth", C.c_int),
                ("scale", C.c_int), ("upsampler", C.c_int), ("mean", C.c_float * 3), ("range", C.c_float)]


class Swin2srDesc(C.Structure):
    """sr_swin2sr_desc (include/sr_hip.h)."""
    _fields_ = [("n_feat", C.c_int), ("n_heads", C.c_int), ("n_hidden", C.c_int), ("n_groups", C.c_int), ("depth", C.c_int),
                ("scale", C.c_int), ("upsampler", C.c_int), ("mean", C.c_float * 3), ("range", C.c_float), ("mask_value", C.c_float)]


class HatDesc(C.Structure):
    """sr_hat_desc (include/sr_hip.h)."""
    _fields_ = [("n_feat", C.c_int), ("n_heads", C.c_int), ("n_hidden", C.c_int), ("n_mid", C.c_int), ("n_squeeze", C.c_int),
                ("n_groups", C.c_int), ("depth", C.c_int), ("scale", C.c_int), ("conv_scale", C.c_float), ("mean", C.c_float * 3),
                ("range", C.c_float)]


class ProfRecord(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_double), ("launches", C.c_int64)]


_lib = None
_lib_lock = threading.Lock()

# name -> (restype, argtypes); every symbol include/sr_hip.h declares
_vp, _i, _i64, _sz, _dbl = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_double
_pi = C.POINTER(C.c_int)
SIGNATURES = {
    "sr_version": (_i, []),
    "sr_source_digest": (C.c_char_p, []),
    "sr_last_error": (C.c_char_p, []),
    "sr_device_count": (_i, [_pi]),
    "sr_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "sr_ctx_create_on_stream": (_i, [_i, _vp, C.POINTER(_vp)]),
    "sr_ctx_destroy": (_i, [_vp]),
    "sr_ctx_sync": (_i, [_vp]),
    "sr_ctx_num_cu": (_i, [_vp, _pi]),
    "sr_dev_alloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "sr_dev_free": (_i, [_vp, _vp]),
    "sr_memcpy_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "sr_memcpy_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "sr_memcpy_d2d": (_i, [_vp, _vp, _vp, _sz]),
    "sr_memset_d": (_i, [_vp, _vp, _i, _sz]),
    "sr_prof_enable": (_i, [_vp, _i]),
    "sr_prof_select": (_i, [_vp, C.c_char_p]),
    "sr_prof_reset": (_i, [_vp]),
    "sr_prof_get": (_i, [_vp, C.POINTER(ProfRecord), _i, _pi]),
    "sr_tile_plan": (_i, [_i, _i, _i, _i, _pi, _pi, _i]),
    "sr_tile_overlaps": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _pi]),
    "sr_tile_neighbors": (_i, [_pi, _i, _i, _i, _pi]),
    "sr_target_size": (_i, [_i, _i, _i, _pi, _pi]),
    "sr_weight_lut": (_i, [_i, _i, C.POINTER(C.c_float)]),
    "sr_tile_extract_pad": (_i, [_vp, _vp, _i, _i, _i, _i64, _pi, _i, _i, _i, _vp]),
    "sr_tile_extract": (_i, [_vp, _vp, _i, _i, _i, _i64, _pi, _i, C.POINTER(_vp), C.POINTER(_i64)]),
    "sr_pyr_down": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sr_pyr_up": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i]),
    "sr_pyr_up_sub": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "sr_pyr_up_add": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "sr_blend_plan_create": (_i, [_vp, C.POINTER(TileRect), _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "sr_blend_plan_destroy": (_i, [_vp]),
    "sr_strip_tile_rows": (_i, [C.POINTER(TileRect), _i, _i, _i, _i, _i, _pi]),
    "sr_pyramid_halo": (_i, [_i, _pi, _pi]),
    "sr_comm_unique_id": (_i, [_vp]),
    "sr_comm_init": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "sr_comm_wrap": (_i, [_vp, C.POINTER(_vp)]),
    "sr_comm_info": (_i, [_vp, _pi, _pi]),
    "sr_comm_destroy": (_i, [_vp]),
    "sr_comm_exchange": (_i, [_vp, _vp, C.POINTER(Xfer), _i, C.POINTER(Xfer), _i]),
    "sr_comm_exchange_tile_rows": (_i, [_vp, _vp, C.POINTER(TileRect), _i, _i, _pi, _pi, C.POINTER(_vp), C.POINTER(_i64),
                                        C.POINTER(_vp)]),
    "sr_comm_allreduce_f64": (_i, [_vp, _vp, _vp, _i]),
    "sr_laplacian_blend_sharded": (_i, [_vp, _vp, _vp, C.POINTER(TileRect), _i, _i, _pi, _pi, C.POINTER(_vp), C.POINTER(_i64),
                                        C.POINTER(_vp), _vp, _i64]),
    "sr_sharded_tile_bases": (_i, [C.POINTER(TileRect), _i, _i, _i, _i, _pi, _pi, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_vp),
                                   C.POINTER(_vp)]),
    "sr_exchange_xfers": (_i, [C.POINTER(TileRect), _i, _i, _i, _i, _pi, _pi, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_vp),
                               C.POINTER(Xfer), _i, _pi, C.POINTER(Xfer), _i, _pi]),
    "sr_strip_bounds": (_i, [C.POINTER(TileRect), _i, _i, _i, _i, _i, _pi]),
    "sr_exchange_plan": (_i, [C.POINTER(TileRect), _i, _i, _i, _i, _i, _i, _i, _i, _pi, _pi, _pi, _pi]),
    "sr_blend_plan_tile_rows": (_i, [_vp, _i, _pi, _pi]),
    "sr_blend_plan_workspace_bytes": (_i, [_vp, C.POINTER(_sz)]),
    "sr_blend_plan_g1_format": (_i, [_vp, _i, C.POINTER(_i)]),
    "sr_blend_plan_march_items": (_i, [_vp, _i, C.POINTER(C.c_int32), _i64, C.POINTER(_i64)]),
    "sr_laplacian_blend": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i64), _vp, _i64, _vp]),
    "sr_weighted_blend": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i64), _vp, _i64, _vp]),
    "sr_blend_pyramids": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i64), _pi, _i, _i]),
    "sr_blend_gather": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i64), _vp, _i64, _vp]),
    "sr_laplacian_fusion_host": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(TileRect), _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sr_weighted_fusion_host": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(TileRect), _i, _i, _i, _i, _i, _vp, _vp]),
    "sr_feather_merge": (_i, [_vp, C.POINTER(MergeTile), _i, C.POINTER(_vp), C.POINTER(_i64), _i, _vp, _i64, _i, _i]),
    "sr_feather_merge_dt": (_i, [_vp, _i, C.POINTER(MergeTile), _i, C.POINTER(_vp), C.POINTER(_i64), _i, _vp, _i64, _i, _i]),
    "sr_gradient_fusion": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(TileRect), _i, _i, _i, _i, _vp, _i64, _vp]),
    "sr_gradient_stats_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(C.c_uint64), C.POINTER(_dbl)]),
    "sr_tile_ssim_sums_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(TileRect), C.POINTER(_vp), C.POINTER(_i64), _i, _i,
                                  C.POINTER(C.c_uint64)]),
    "sr_commercial_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, C.POINTER(TileRect), _pi, _i, C.POINTER(_i64),
                              C.POINTER(_dbl)]),
    "sr_fft_max_len": (_i, []),
    "sr_fft_c2c": (_i, [_vp, _vp, _vp, _i64, _i]),
    "sr_saliency_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp]),
    "sr_local_entropy_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "sr_forbidden_map": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(TileRect), _i, _vp]),
    "sr_rect_counts_u8": (_i, [_vp, _vp, _i64, _i, _i, C.POINTER(TileRect), _i, C.POINTER(C.c_uint64)]),
    "sr_poisson_max_side": (_i, []),
    "sr_poisson_clone_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i, _i, _i, _vp, _i64]),
    "sr_gaussian_blur15_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _i64]),
    "sr_region_ssim_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, C.POINTER(_dbl)]),
    "sr_resize_linear_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _i64, _i, _i]),
    "sr_sse_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i64, C.POINTER(C.c_uint64)]),
    "sr_sse_u8_async": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i64, _vp]),
    "sr_psnr_from_sse": (_dbl, [C.c_uint64, C.c_uint64, _dbl]),
    "sr_seam_scan": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(TileRect), C.POINTER(_vp), C.POINTER(_i64), _i, _i, _i, _i,
                          _dbl, C.POINTER(SeamRecord), _i, _pi]),
    "sr_sse_f32": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i64, C.POINTER(_dbl)]),
    "sr_weighted_blend_custom": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_vp), C.POINTER(_i64), _vp, _i64, _vp]),
    "sr_ssim_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _dbl, _i, _i, C.POINTER(_dbl), C.POINTER(C.c_uint64)]),
    "sr_ssim_float": (_i, [_vp, _i, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _dbl, _i, _i, C.POINTER(_dbl), C.POINTER(C.c_uint64)]),
    "sr_ssim_u8_async": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _dbl, _i, _i, _vp, C.POINTER(C.c_uint64)]),
    "sr_assess_u8_async": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _dbl, _i, _i, _i, _vp]),
    "sr_assess_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _dbl, _i, _i, _i, C.POINTER(AssessSums)]),
    "sr_assess_resized_u8_async": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, _dbl, _i, _vp]),
    "sr_assess_resized_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, _dbl, _i, C.POINTER(AssessSums)]),
    "sr_ssim_count": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_uint64)]),
    "sr_quality_map_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _dbl, _pi, _i, _pi, _i, _i, C.POINTER(QualityCell)]),
    "sr_quality_map_counts": (_i, [_i, _i, _i, _pi, _i, _pi, _i, C.POINTER(C.c_uint64)]),
    "sr_ms_ssim_plan": (_i, [_i, _i, _i, _pi, _pi, C.POINTER(C.c_uint64), C.POINTER(_sz)]),
    "sr_ms_ssim_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _dbl, _i, C.POINTER(MsSsimLevel)]),
    "sr_ms_ssim_value": (_dbl, [C.POINTER(MsSsimLevel), _i, C.POINTER(_dbl)]),
    "sr_ms_ssim_planes": (_i, [_vp, _i, _vp, _vp]),
    "sr_bench_plan": (_i, [_i, _i, _i, _i, _i, _pi, _pi, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_sz)]),
    "sr_bench_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _dbl, C.POINTER(BenchSums)]),
    "sr_vif_plan": (_i, [_i, _i, _i, _i, _i, _pi, _pi, C.POINTER(C.c_uint64), C.POINTER(_sz)]),
    "sr_vif_window": (_i, [_i, C.POINTER(_dbl)]),
    "sr_vif_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, C.POINTER(VifScale)]),
    "sr_vif_value": (_dbl, [C.POINTER(VifScale), _i]),
    "sr_gmsd_plan": (_i, [_i, _i, _i, _i, _i, _pi, _pi, C.POINTER(C.c_uint64), C.POINTER(_sz)]),
    "sr_gmsd_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, C.POINTER(GmsdSums)]),
    "sr_gmsd_value": (_dbl, [C.POINTER(GmsdSums)]),
    "sr_fsim_plan": (_i, [_i, _i, _i, _pi, _pi, _pi, C.POINTER(_sz)]),
    "sr_fsim_filters": (_i, [_i, _i, C.POINTER(_dbl), C.POINTER(_dbl), C.POINTER(_dbl), C.POINTER(_dbl), C.POINTER(_dbl)]),
    "sr_fsim_pool_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, C.POINTER(C.c_int64)]),
    "sr_fsim_pc_f64": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(_dbl), C.POINTER(_dbl)]),
    "sr_fsim_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, C.POINTER(FsimSums)]),
    "sr_fsim_value": (_i, [C.POINTER(FsimSums), C.POINTER(_dbl), C.POINTER(_dbl)]),
    "sr_fsim_chroma_weight": (_dbl, [_dbl, _dbl]),
    "sr_vsi_plan": (_i, [_i, _i, _i, _pi, _pi, _pi, C.POINTER(_sz)]),
    "sr_vsi_filter": (_i, [C.POINTER(_dbl), C.POINTER(_dbl)]),
    "sr_vsi_resize_weights": (_i, [_i, _i, _i, _pi, C.POINTER(_dbl), C.POINTER(C.c_int32)]),
    "sr_vsi_pool_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, C.POINTER(C.c_int64)]),
    "sr_vsi_saliency_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(_dbl), C.POINTER(_dbl), C.POINTER(_dbl)]),
    "sr_vsi_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, C.POINTER(VsiSums)]),
    "sr_vsi_value": (_dbl, [C.POINTER(VsiSums)]),
    "sr_vsi_chroma_weight": (_dbl, [_dbl]),
    "sr_vsi_host_u8": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, C.POINTER(VsiSums)]),
    "sr_delta_e_plan": (_i, [_i, _i, _i, _i, _i, _pi, _pi, C.POINTER(C.c_uint64), _pi, C.POINTER(_sz)]),
    "sr_delta_e_table": (_i, [C.POINTER(_dbl)]),
    "sr_delta_e_lab_u8": (_i, [_i, _i, _i, C.POINTER(_dbl)]),
    "sr_delta_e_pair": (_i, [C.POINTER(_dbl), C.POINTER(_dbl), _i, C.POINTER(_dbl)]),
    "sr_delta_e_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _vp, _i64, C.POINTER(DeltaESums)]),
    "sr_delta_e_cells_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _pi, _i, _pi, _i, C.POINTER(DeltaECell)]),
    "sr_delta_e_mean": (_dbl, [C.POINTER(DeltaESums)]),
    "sr_delta_e_rms": (_dbl, [C.POINTER(DeltaESums)]),
    "sr_delta_e_percentile": (_dbl, [C.POINTER(DeltaESums), _dbl]),
    "sr_delta_e_fraction_at_least": (_i, [C.POINTER(DeltaESums), _dbl, C.POINTER(_dbl)]),
    "sr_mser_default_params": (_i, [C.POINTER(MserParams)]),
    "sr_mser_plan": (_i, [_i, _i, C.POINTER(MserParams), C.POINTER(_sz), C.POINTER(_i64)]),
    "sr_mser_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(MserParams), _i, _vp, _i64, C.POINTER(_i64)]),
    "sr_mser_tree_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp, _i64, C.POINTER(_i64)]),
    "sr_mser_last_regions": (_i, [_vp, _vp, _i64, C.POINTER(_i64)]),
    "sr_mser_workspace": (_i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    "sr_mser_host_u8": (_i, [_vp, _i64, _i, _i, _i, C.POINTER(MserParams), _i, _vp, _i64, C.POINTER(_i64)]),
    "sr_mser_tree_host_u8": (_i, [_vp, _i64, _i, _i, _i, _i, _vp, _i64, C.POINTER(_i64)]),
    "sr_mser_text_boxes": (_i, [_vp, _i64, _i, C.POINTER(TileRect), C.POINTER(_i64)]),
    "sr_cascade_create": (_i, [C.POINTER(CascadeInfo)] + [_vp] * 9 + [C.POINTER(_vp)]),
    "sr_cascade_destroy": (_i, [_vp]),
    "sr_cascade_desc": (_i, [_vp, C.POINTER(CascadeInfo)]),
    "sr_cascade_default_params": (_i, [C.POINTER(CascadeParams)]),
    "sr_cascade_plan": (_i, [_vp, _i, _i, C.POINTER(CascadeParams), C.POINTER(CascadeScale), _i, C.POINTER(_i), C.POINTER(_sz),
                             C.POINTER(_i64)]),
    "sr_cascade_u8": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, C.POINTER(CascadeParams), _vp, _i64, C.POINTER(_i64)]),
    "sr_cascade_last_candidates": (_i, [_vp, _vp, _i64, C.POINTER(_i64)]),
    "sr_cascade_group": (_i, [_vp, _i64, _i, _vp, C.POINTER(_i64)]),
    "sr_cascade_plane_u8": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, C.POINTER(CascadeParams), _i, _vp]),
    "sr_cascade_stage_map_u8": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _vp, _i64, C.POINTER(_i64)]),
    "sr_cascade_workspace": (_i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    "sr_cascade_host_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(CascadeParams), _vp, _i64, C.POINTER(_i64)]),
    "sr_cascade_plane_host_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(CascadeParams), _i, _vp]),
    "sr_cascade_stage_map_host_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp, _i64, C.POINTER(_i64)]),
    "sr_haarpsi_plan": (_i, [_i, _i, _i, _i, _i, _i, _pi, _pi, C.POINTER(C.c_uint64), _pi, C.POINTER(_sz)]),
    "sr_haarpsi_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, C.POINTER(HaarPsiSums)]),
    "sr_haarpsi_cells_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, _pi, _i, _pi, _i, C.POINTER(HaarPsiCell)]),
    "sr_haarpsi_value": (_dbl, [C.POINTER(HaarPsiSums)]),
    "sr_haarpsi_cell_value": (_dbl, [_dbl, _dbl]),
    "sr_haarpsi_host_u8": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, C.POINTER(HaarPsiSums)]),
    "sr_niqe_plan": (_i, [_i, _i, _i, _i, _pi, _pi, _pi, _pi, C.POINTER(_sz)]),
    "sr_niqe_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "sr_niqe_half_plane": (_i, [_vp, _vp]),
    "sr_niqe_features": (_i, [_vp, _i64, _vp]),
    "sr_niqe_fit": (_i, [_vp, _vp, _vp, _i, _dbl, _vp, _vp, C.POINTER(_i64)]),
    "sr_niqe_score": (_dbl, [_vp, _i64, _vp, _vp]),
    "sr_brisque_plan": (_i, [_i, _i, _i, _i, _pi, _pi, _pi, _pi, C.POINTER(_sz)]),
    "sr_brisque_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "sr_brisque_half_plane": (_i, [_vp, _vp]),
    "sr_brisque_features": (_i, [_vp, _vp]),
    "sr_brisque_score": (_dbl, [_vp, _vp, _vp, _i64, _dbl, _dbl, _vp, _vp, _dbl, _dbl]),
    "sr_rgb2gray_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _i64]),
    "sr_imresize_size": (_i, [_i, _dbl]),
    "sr_imresize_weights": (_i, [_i, _i, _dbl, _i, _i, _pi, _vp, _vp]),
    "sr_imresize_plan": (_i, [_i, _i, _i, _dbl, _dbl, _i, _i, _i, _pi, _pi, _pi, _pi, _pi, C.POINTER(_sz), C.POINTER(_sz)]),
    "sr_imresize_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _dbl, _dbl, _i, _i, _vp, _i64, _i, _i]),
    "sr_resize_cubic_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _i64, _i, _i]),
    "sr_resize_cubic_window_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i64]),
    "sr_gray_moments_u8": (_i, [_vp, _vp, _i, _i64, _i64, _i, _i, _i, _i, C.POINTER(C.c_uint64)]),
    "sr_histogram_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(C.c_uint64)]),
    "sr_color_table_class": (_i, [C.POINTER(C.c_float), _i, _i, C.POINTER(_i)]),
    "sr_color_correct_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(C.c_float), _i, _i, C.c_float, _vp, _i64]),
    "sr_encode_tiff_lzw": (_i, [_vp, _i, _i, _i, _i64, C.c_char_p, _i]),
    "sr_encode_png": (_i, [_vp, _i, _i, _i, _i64, _i, C.c_char_p, _i]),
    "sr_encode_jpeg": (_i, [_vp, _i, _i, _i, _i64, _i, C.c_char_p, _i]),
    "sr_lpips_create": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), _i, C.POINTER(_vp), _i, _vp, _vp, C.POINTER(_vp)]),
    "sr_lpips_destroy": (_i, [_vp]),
    "sr_lpips_layer_sizes": (_i, [_i, _i, _i, _pi]),
    "sr_lpips_tile_count": (_i, [_i, _i, _i, _pi]),
    "sr_lpips_tile_plan": (_i, [_i, _i, _i, _i, _i, _pi, _pi, C.POINTER(_i64)]),
    "sr_lpips_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, C.POINTER(_dbl)]),
    "sr_dists_create": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _vp, C.POINTER(_vp)]),
    "sr_dists_destroy": (_i, [_vp]),
    "sr_dists_tile_count": (_i, [_i, _i, _i, _pi]),
    "sr_dists_tile_plan": (_i, [_i, _i, _i, _i, _pi, _pi, C.POINTER(_i64)]),
    "sr_dists_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, _vp]),
    "sr_dists_l2pool_f32": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sr_dists_layer_sizes": (_i, [_i, _i, _pi]),
    "sr_dists_score": (_i, [_vp, _vp, _vp, _vp, C.POINTER(_dbl), _vp, _vp]),
    "sr_srnet_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "sr_srnet_destroy": (_i, [_vp]),
    "sr_srnet_plan": (_i, [_i, _i, _i, _i, _i, _i, _pi, _pi, C.POINTER(_sz)]),
    "sr_srnet_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_srnet_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_resnet_create": (_i, [_vp, C.POINTER(ResNetDesc), C.POINTER(_vp), C.POINTER(_vp), _i, C.POINTER(_vp)]),
    "sr_resnet_destroy": (_i, [_vp]),
    "sr_resnet_plan": (_i, [C.POINTER(ResNetDesc), _i, _i, _i, _pi, _pi, C.POINTER(_sz)]),
    "sr_resnet_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_resnet_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_rrdb_create": (_i, [_vp, C.POINTER(RrdbDesc), C.POINTER(_vp), C.POINTER(_vp), _i, C.POINTER(_vp)]),
    "sr_rrdb_destroy": (_i, [_vp]),
    "sr_rrdb_plan": (_i, [C.POINTER(RrdbDesc), _i, _i, _i, _i, _pi, _pi, _pi, C.POINTER(_sz)]),
    "sr_rrdb_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_rrdb_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_rcan_create": (_i, [_vp, C.POINTER(RcanDesc), C.POINTER(_vp), C.POINTER(_vp), _i, C.POINTER(_vp)]),
    "sr_rcan_destroy": (_i, [_vp]),
    "sr_rcan_plan": (_i, [C.POINTER(RcanDesc), _i, _i, _i, _pi, _pi, C.POINTER(_sz)]),
    "sr_rcan_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_rcan_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_rcan_attention_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sr_swinir_create": (_i, [_vp, C.POINTER(SwinirDesc), C.POINTER(_vp), C.POINTER(_vp), _i, C.POINTER(_vp)]),
    "sr_swinir_destroy": (_i, [_vp]),
    "sr_swinir_plan": (_i, [C.POINTER(SwinirDesc), _i, _i, _i, _pi, _pi, _pi, _pi, C.POINTER(_sz)]),
    "sr_swinir_rel_index": (_i, [_vp, _i]),
    "sr_swinir_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_swinir_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_swinir_fill_workspace": (_i, [_vp, _i, _i, _i, _i]),
    "sr_swinir_layernorm_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _vp, _vp, _vp, _i64, _i64]),
    "sr_swinir_attention_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp, _vp, _i64, _i64]),
    "sr_d4_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _i64]),
    "sr_d4_acc_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp, _i64]),
    "sr_ens_finish_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _i64]),
    "sr_ens_finish_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _i64]),
    "sr_ens_plan": (_i, [_i, _i, _i, _i, _pi, C.POINTER(_sz)]),
    "sr_srnet_ens_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_srnet_ens_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_resnet_ens_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_resnet_ens_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_rrdb_ens_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i, _i]),
    "sr_rrdb_ens_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i, _i]),
    "sr_rcan_ens_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_rcan_ens_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_swinir_ens_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_swinir_ens_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_hat_create": (_i, [_vp, C.POINTER(HatDesc), C.POINTER(_vp), C.POINTER(_vp), _i, _vp, C.POINTER(_vp)]),
    "sr_hat_destroy": (_i, [_vp]),
    "sr_hat_plan": (_i, [C.POINTER(HatDesc), _i, _i, _i, _pi, _pi, _pi, _pi, C.POINTER(_sz)]),
    "sr_hat_rel_index": (_i, [_vp, _i]),
    "sr_hat_oca_index": (_i, [_vp, _i]),
    "sr_hat_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_hat_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_hat_fill_workspace": (_i, [_vp, _i, _i, _i, _i]),
    "sr_hat_attention_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp, _vp, _i64, _i64]),
    "sr_hat_oca_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _i64]),
    "sr_hat_ens_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_hat_ens_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_swin2sr_create": (_i, [_vp, C.POINTER(Swin2srDesc), C.POINTER(_vp), C.POINTER(_vp), _i, C.POINTER(_vp)]),
    "sr_swin2sr_destroy": (_i, [_vp]),
    "sr_swin2sr_plan": (_i, [C.POINTER(Swin2srDesc), _i, _i, _i, _pi, _pi, _pi, _pi, C.POINTER(_sz)]),
    "sr_swin2sr_cpb_bias": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "sr_swin2sr_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_swin2sr_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i]),
    "sr_swin2sr_fill_workspace": (_i, [_vp, _i, _i, _i, _i]),
    "sr_swin2sr_attention_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp, _vp, C.c_float, _vp, _i64, _i64]),
    "sr_swin2sr_layernorm_add_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64]),
    "sr_swin2sr_ens_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
    "sr_swin2sr_ens_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _i, _i]),
}


def _preload_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels ship their own libamdhip64.so (SONAME
    libamdhip64.so.7, like /opt/rocm's); if libsrhip.so pulled in the system copy first and torch is
    imported later, two HIP/HSA runtimes would fight over the device ("No HIP GPUs are available").
    Loading torch's copy by path first makes both resolve to the same object (glibc matches our NEEDED
    entry by SONAME and torch's by inode).  Without torch installed the system runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def _preload_rccl() -> None:
    """One RCCL per process, and the one PyTorch was built against: libtorch_hip.so needs "librccl.so" and would adopt
    whichever copy the process already holds, so before sr_comm.cpp binds RCCL (dlopen; a held copy wins) the wheel's own
    copy is loaded by path.  Without torch installed the ROCm copy is used.  RTLD_LOCAL on purpose: librccl.so drags in
    librocm_smi64.so, whose statics libamd_smi.so (loaded later by torch's device queries) re-defines -- with the symbols
    global both copies destroyed the same objects at exit (double free, seen in the full GPU suite)."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "librccl.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand)
        except OSError:
            pass


def load():
    """Load libsrhip.so, rebuilding it first when it is missing or older than csrc/ / include/ (the .so is git-ignored
    and travels with the tree, so an edited source must never meet yesterday's binary).  Raises SrNativeError."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        _preload_hip_runtime()
        import importlib.util
        spec = importlib.util.spec_from_file_location("_sr_build", os.path.join(_HERE, "_build.py"))
        bld = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bld)
        if not os.environ.get("SR_LIB_PATH"):
            try:
                if bld._stale():                       # missing, or not built from these sources / flags: never run a stale binary silently
                    bld.build_native()
            except Exception as exc:  # noqa: BLE001
                raise SrNativeError(f"libsrhip.so is missing or older than its sources and could not be rebuilt: {exc}") from exc
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as exc:
            raise SrNativeError(f"cannot load {LIB_PATH}: {exc}") from exc
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def last_error() -> str:
    return load().sr_last_error().decode("utf-8", "replace")


def check(rc: int) -> None:
    if rc == SR_OK:
        return
    msg = last_error()
    if rc == SR_ERR_INVALID_ARG:
        raise ValueError(msg)
    if rc == SR_ERR_SHAPE:
        raise SrShapeError(msg)
    if rc == SR_ERR_OOM:
        raise MemoryError(msg)
    raise SrNativeError(f"[sr {rc}] {msg}")


def device_count() -> int:
    n = C.c_int(0)
    rc = load().sr_device_count(C.byref(n))
    return n.value if rc == SR_OK else 0


# ------------------------------------------------------------------------------------------
# host-only bookkeeping wrappers
# ------------------------------------------------------------------------------------------
def tile_plan(image_w: int, image_h: int, block: int, overlap_px: int) -> List[Tuple[int, int, int, int]]:
    lib = load()
    n = C.c_int(0)
    check(lib.sr_tile_plan(image_w, image_h, block, overlap_px, C.byref(n), None, 0))
    buf = (C.c_int * (4 * n.value))()
    check(lib.sr_tile_plan(image_w, image_h, block, overlap_px, C.byref(n), buf, n.value))
    return [tuple(buf[4 * i: 4 * i + 4]) for i in range(n.value)]


def tile_overlaps(x, y, w, h, image_w, image_h, block, overlap_px) -> Tuple[int, int, int, int]:
    out = (C.c_int * 4)()
    check(load().sr_tile_overlaps(x, y, w, h, image_w, image_h, block, overlap_px, out))
    return tuple(out)


def tile_neighbors(xywh: Sequence[Tuple[int, int, int, int]], block: int, overlap_px: int):
    n = len(xywh)
    flat = (C.c_int * (4 * n))(*[v for t in xywh for v in t])
    out = (C.c_int * (4 * n))()
    check(load().sr_tile_neighbors(flat, n, block, overlap_px, out))
    return [tuple(out[4 * i: 4 * i + 4]) for i in range(n)]


def target_size(width: int, height: int, preset_mp: int) -> Tuple[int, int]:
    w, h = C.c_int(0), C.c_int(0)
    check(load().sr_target_size(width, height, preset_mp, C.byref(w), C.byref(h)))
    return w.value, h.value


def weight_lut(fw: int, weight_type: str) -> np.ndarray:
    out = np.empty(fw + 1, dtype=np.float32)
    check(load().sr_weight_lut(fw, WEIGHT_TYPES[weight_type], out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def strip_tile_rows(rects_xywh, levels: int, canvas_h: int, row_begin: int, row_end: int):
    """Host-only: tile-local input rows [(r0, r1)] every tile must supply for canvas rows [row_begin,row_end)."""
    n = len(rects_xywh)
    rects = (TileRect * n)(*[TileRect(int(x), int(y), int(w), int(h)) for (x, y, w, h) in rects_xywh])
    out = (C.c_int * (2 * n))()
    check(load().sr_strip_tile_rows(rects, n, int(levels), int(canvas_h), int(row_begin), int(row_end), out))
    return [(out[2 * i], out[2 * i + 1]) for i in range(n)]


_JPEG_EXT = (".jpg", ".jpeg", ".jpe", ".jfif")


def write_image(arr: np.ndarray, path: str, threads: int = 0, png_level: int = 3, jpeg_quality: int = 95) -> str:
    """Stage 5 of the pipeline (main.py:399-404) with the native multi-threaded writers: .tif / .tiff -> TIFF-LZW,
    .png -> PNG (compress_level 3), .jpg / .jpeg / .jpe / .jfif -> JPEG quality 95.  Any other extension goes to Pillow's
    ``save(path, quality=95)`` -- the reference's own else-branch (main.py:403), which picks the format from the extension
    (.bmp, .webp, ...) and raises for an unknown one -- never a JPEG stream under another name.  arr: HxW or HxWxC uint8.
    Returns the format."""
    a = np.ascontiguousarray(arr)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError("write_image expects an HxW or HxWxC uint8 array")
    h, w = a.shape[:2]
    cn = a.shape[2] if a.ndim == 3 else 1
    lib, p, low = load(), os.fsencode(path), str(path).lower()
    ptr = a.ctypes.data_as(C.c_void_p)
    if low.endswith(".tif") or low.endswith(".tiff"):
        check(lib.sr_encode_tiff_lzw(ptr, h, w, cn, w * cn, p, threads))
        return "TIFF"
    if low.endswith(".png"):
        check(lib.sr_encode_png(ptr, h, w, cn, w * cn, png_level, p, threads))
        return "PNG"
    if low.endswith(_JPEG_EXT):
        if cn == 4:
            raise OSError("cannot write mode RGBA as JPEG")             # what Pillow raises (main.py:403 would propagate it)
        check(lib.sr_encode_jpeg(ptr, h, w, cn, w * cn, jpeg_quality, p, threads))
        return "JPEG"
    from PIL import Image
    img = Image.fromarray(a if cn != 1 else a.reshape(h, w))
    img.save(path, quality=jpeg_quality)                               # ValueError for an unknown extension, like the reference
    return (img.format or os.path.splitext(low)[1].lstrip(".")).upper()


OWNER_POLICIES = {"balanced": 0, "roundrobin": 1, "locality": 2}


def _rects(rects_xywh):
    n = len(rects_xywh)
    return n, (TileRect * max(n, 1))(*[TileRect(int(x), int(y), int(w), int(h)) for (x, y, w, h) in rects_xywh])


def strip_bounds(rects_xywh, levels: int, canvas_h: int, canvas_w: int, world: int) -> List[int]:
    """Host-only: work-balanced, even strip boundaries (sr_strip_bounds)."""
    n, rects = _rects(rects_xywh)
    out = (C.c_int * (world + 1))()
    check(load().sr_strip_bounds(rects, n, int(levels), int(canvas_h), int(canvas_w), int(world), out))
    return list(out)


def exchange_plan(rects_xywh, cn: int, levels: int, canvas_h: int, canvas_w: int, world: int, metric_halo: int,
                  owner_policy: str = "balanced"):
    """Host-only: (bounds, rows per rank, need[r][t] = (r0, r1), owners) of the strip exchange (sr_exchange_plan)."""
    n, rects = _rects(rects_xywh)
    bounds, rows = (C.c_int * (world + 1))(), (C.c_int * (2 * world))()
    need, owner = (C.c_int * (2 * world * n))(), (C.c_int * n)()
    check(load().sr_exchange_plan(rects, n, int(cn), int(levels), int(canvas_h), int(canvas_w), int(world), int(metric_halo),
                                  OWNER_POLICIES[owner_policy], bounds, rows, need, owner))
    return (list(bounds), [(rows[2 * r], rows[2 * r + 1]) for r in range(world)],
            [[(need[(r * n + t) * 2], need[(r * n + t) * 2 + 1]) for t in range(n)] for r in range(world)], list(owner))


def pyramid_halo(levels: int) -> Tuple[int, int]:
    """Host-only: worst-case (rows below, rows above) a strip reads of a tile beyond its own rows."""
    a, b = C.c_int(0), C.c_int(0)
    check(load().sr_pyramid_halo(int(levels), C.byref(a), C.byref(b)))
    return a.value, b.value


def color_table_class(glut: np.ndarray, terms: int = 64) -> int:
    """Host-only: how the first stage of the guided filter may sum a guide table (cn x 256 float32) -- 1 whole numbers
    (32-bit sliding sums), 2 box sums of `terms` values exact in fp64 (sliding fp64 sums), 0 ordered sums."""
    g = np.ascontiguousarray(glut, dtype=np.float32).reshape(-1, 256)
    cls = C.c_int(-1)
    check(load().sr_color_table_class(g.ctypes.data_as(C.POINTER(C.c_float)), int(g.shape[0]), int(terms), C.byref(cls)))
    return cls.value


def ssim_count(h: int, w: int, mode: str, row_begin: int = 0, row_end: Optional[int] = None) -> int:
    n = C.c_uint64(0)
    check(load().sr_ssim_count(h, w, SSIM_MODES[mode], row_begin, h if row_end is None else row_end, C.byref(n)))
    return n.value


def _edge_array(edges, name: str):
    """An edge list as a C int array; anything that is not a flat list of at least two whole numbers is a ValueError."""
    e = np.asarray(edges)
    if e.ndim != 1 or e.size < 2 or e.dtype.kind not in "iu":
        raise ValueError(f"{name}: need a flat list of at least two integer edges")
    if e.min() < -2 ** 31 or e.max() >= 2 ** 31:
        raise ValueError(f"{name}: edge out of range")
    return (C.c_int * e.size)(*[int(v) for v in e]), int(e.size) - 1


def quality_map_counts(h: int, w: int, mode: str, x_edges, y_edges) -> np.ndarray:
    """Host-only: (gh, gw) uint64 numbers of valid SSIM-map samples of `mode` per cell of the separable grid
    (sr_quality_map_counts).  ValueError for edges that are not strictly increasing from 0 to w / h."""
    xe, gw = _edge_array(x_edges, "x_edges")
    ye, gh = _edge_array(y_edges, "y_edges")
    out = np.zeros((gh, gw), dtype=np.uint64)
    check(load().sr_quality_map_counts(int(h), int(w), SSIM_MODES[mode], xe, gw, ye, gh,
                                       out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out


def _whole(v, name: str) -> int:
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"{name} must be a whole number, got {v!r}")
    return int(v)


def ms_ssim_plan(h: int, w: int, levels: int = 5) -> dict:
    """Host only (sr_ms_ssim_plan): the per-level sizes [(h_j, w_j)], the per-level map sample counts and the bytes of context
    scratch of an MS-SSIM call.  ValueError for levels outside 1..5, SrShapeError (a ValueError) naming the minimum side for
    an image too small for that many levels."""
    h, w, levels = _whole(h, "h"), _whole(w, "w"), _whole(levels, "levels")
    n = max(1, min(levels, MS_SSIM_MAX_LEVELS))
    lh, lw, cnt, nbytes = (C.c_int * n)(), (C.c_int * n)(), (C.c_uint64 * n)(), C.c_size_t(0)
    check(load().sr_ms_ssim_plan(h, w, levels, lh, lw, cnt, C.byref(nbytes)))
    return {"sizes": [(lh[j], lw[j]) for j in range(n)], "counts": [int(cnt[j]) for j in range(n)],
            "scratch_bytes": int(nbytes.value)}


def _ms_ssim_weights(weights, levels: int):
    if weights is None:
        return None
    wt = [float(v) for v in weights]
    if len(wt) != levels:
        raise ValueError(f"ms_ssim: {levels} levels need {levels} weights, got {len(wt)}")
    if not all(np.isfinite(wt)):
        raise ValueError("ms_ssim: weights must be finite")
    return (C.c_double * levels)(*wt)


def ms_ssim_value(levels_out, weights=None) -> float:
    """Host only (sr_ms_ssim_value): prod_{j < L-1} max(CS_j, 0)^w_j * max(S_{L-1}, 0)^w_{L-1} of per-level records
    [(sum_lcs, sum_cs, count)]; weights: L numbers, default Wang's."""
    recs = [(float(a), float(b), int(n)) for (a, b, n) in levels_out]
    n = len(recs)
    if n < 1 or n > MS_SSIM_MAX_LEVELS:
        raise ValueError(f"ms_ssim_value: levels must be 1 .. {MS_SSIM_MAX_LEVELS} (got {n})")
    if any(r[2] < 1 for r in recs):
        raise ValueError("ms_ssim_value: a level without samples")
    arr = (MsSsimLevel * n)(*[MsSsimLevel(*r) for r in recs])
    v = float(load().sr_ms_ssim_value(arr, n, _ms_ssim_weights(weights, n)))
    if v != v:
        raise ValueError(last_error())
    return v


def bench_plan(h: int, w: int, cn: int, crop_border: int = 0, mode: int = BENCH_Y) -> dict:
    """Host only (sr_bench_plan): the cropped size, the element and map sample counts and the bytes of context scratch of an
    SR-benchmark PSNR / SSIM call.  ValueError for cn not 1 or 3, an unknown mode, a Y mode on one channel or a negative
    crop_border; SrShapeError (a ValueError) naming the minimum for a side below 11 after the crop."""
    h, w, cn, crop_border, mode = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn"), (crop_border, "crop_border"),
                                                             (mode, "mode")))
    ch, cw, ne, nm, nbytes = C.c_int(0), C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
    check(load().sr_bench_plan(h, w, cn, crop_border, mode, C.byref(ch), C.byref(cw), C.byref(ne), C.byref(nm), C.byref(nbytes)))
    return {"size": (ch.value, cw.value), "n_elems": int(ne.value), "n_map": int(nm.value), "scratch_bytes": int(nbytes.value)}


def bench_values(sums: dict, data_range: float = 255.0) -> Tuple[float, float]:
    """(psnr, ssim) of a bench_u8 record: 10 log10(R^2 / (sse / n_elems)), inf for sse == 0, and ssim_sum / n_map."""
    sse = sums["sse"]
    psnr = float("inf") if sse == 0 else 10.0 * math.log10(float(data_range) * float(data_range) / (sse / sums["n_elems"]))
    return psnr, sums["ssim_sum"] / sums["n_map"]


def vif_plan(h: int, w: int, cn: int, crop_border: int = 0, mode: int = BENCH_Y) -> dict:
    """Host only (sr_vif_plan): the plane sizes [(h_s, w_s)] and map sample counts of VIF's four scales and the bytes of context
    scratch of a call.  ValueError for cn not 1 or 3, an unknown mode, a Y mode on one channel, SR_BENCH_CHANNELS on three or a
    negative crop_border; SrShapeError (a ValueError) naming the minimum for a side below 41 after the crop."""
    h, w, cn, crop_border, mode = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn"), (crop_border, "crop_border"),
                                                             (mode, "mode")))
    sh, sw, cnt, nbytes = (C.c_int * VIF_SCALES)(), (C.c_int * VIF_SCALES)(), (C.c_uint64 * VIF_SCALES)(), C.c_size_t(0)
    check(load().sr_vif_plan(h, w, cn, crop_border, mode, sh, sw, cnt, C.byref(nbytes)))
    return {"sizes": [(sh[s], sw[s]) for s in range(VIF_SCALES)], "counts": [int(cnt[s]) for s in range(VIF_SCALES)],
            "scratch_bytes": int(nbytes.value)}


def vif_window(scale: int) -> np.ndarray:
    """Host only (sr_vif_window): the N = 17, 9, 5, 3 normalised 1-D taps of scale 1 .. 4.  ValueError for another scale."""
    scale = _whole(scale, "scale")
    taps = (C.c_double * 17)()
    check(load().sr_vif_window(scale, taps))
    return np.array(taps[:(16 >> (scale - 1)) + 1], np.float64)


def vif_value(scales) -> float:
    """Host only (sr_vif_value): sum num_s / sum den_s of the four (num, den, count) records of vif_u8; NaN for a flat
    reference (every den 0).  ValueError for anything but four records."""
    scales = list(scales)
    if len(scales) != VIF_SCALES:
        raise ValueError(f"vif_value: need the {VIF_SCALES} scale records of vif_u8 (got {len(scales)})")
    arr = (VifScale * VIF_SCALES)(*[VifScale(float(n), float(d), int(c)) for n, d, c in scales])
    return float(load().sr_vif_value(arr, VIF_SCALES))


def gmsd_plan(h: int, w: int, cn: int, crop_border: int = 0, mode: int = BENCH_Y) -> dict:
    """Host only (sr_gmsd_plan): the half-size map, its sample count and the bytes of context scratch of a GMSD call.
    ValueError as vif_plan; SrShapeError naming the minimum for a side below 4 after the crop."""
    h, w, cn, crop_border, mode = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn"), (crop_border, "crop_border"),
                                                             (mode, "mode")))
    mh, mw, cnt, nbytes = C.c_int(0), C.c_int(0), C.c_uint64(0), C.c_size_t(0)
    check(load().sr_gmsd_plan(h, w, cn, crop_border, mode, C.byref(mh), C.byref(mw), C.byref(cnt), C.byref(nbytes)))
    return {"size": (mh.value, mw.value), "count": int(cnt.value), "scratch_bytes": int(nbytes.value)}


def gmsd_value(sums: dict) -> float:
    """Host only (sr_gmsd_value): the deviation sqrt((sum_d2 - sum_d^2 / n) / (n - 1)) of a gmsd_u8 record.  ValueError for
    fewer than 2 samples."""
    rec = GmsdSums(float(sums["sum_d"]), float(sums["sum_d2"]), int(sums["count"]))
    v = float(load().sr_gmsd_value(C.byref(rec)))
    if v != v:
        raise ValueError(last_error())
    return v


def fsim_plan(h: int, w: int, cn: int) -> dict:
    """Host only (sr_fsim_plan): F, the pooled size and the bytes of context workspace of an FSIM call.  ValueError for cn not
    1, 3 or 4; SrShapeError (a ValueError) naming the minimum for a side below 16; SrNativeError naming the cap for a pooled
    side above 2048."""
    h, w, cn = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn")))
    f, rows, cols, nbytes = C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    check(load().sr_fsim_plan(h, w, cn, C.byref(f), C.byref(rows), C.byref(cols), C.byref(nbytes)))
    return {"F": f.value, "size": (rows.value, cols.value), "workspace_bytes": int(nbytes.value)}


def fsim_filters(rows: int, cols: int) -> dict:
    """Host only (sr_fsim_filters): {'log_gabor': [4, rows, cols], 'spread': [4, rows, cols], 'em', 's2', 'sij': [4]} of a
    pooled size, the planes as the transform indexes them (DC first).  SrShapeError for a side below 16, SrNativeError above
    2048."""
    rows, cols = _whole(rows, "rows"), _whole(cols, "cols")
    if rows < 1 or cols < 1:
        raise ValueError("fsim_filters: need rows, cols >= 1")
    lg, sp = np.zeros((4, rows, cols), np.float64), np.zeros((4, rows, cols), np.float64)
    em, s2, sij = np.zeros(4, np.float64), np.zeros(4, np.float64), np.zeros(4, np.float64)
    dp = C.POINTER(C.c_double)
    check(load().sr_fsim_filters(rows, cols, lg.ctypes.data_as(dp), sp.ctypes.data_as(dp), em.ctypes.data_as(dp),
                                 s2.ctypes.data_as(dp), sij.ctypes.data_as(dp)))
    return {"log_gabor": lg, "spread": sp, "em": em, "s2": s2, "sij": sij}


def fsim_value(sums: dict) -> Tuple[float, float]:
    """Host only (sr_fsim_value): (FSIM, FSIMc) of an fsim_u8 record; NaN for a flat pair."""
    rec = FsimSums(float(sums["sum_s"]), float(sums["sum_sc"]), float(sums["sum_pcm"]), int(sums.get("count", 0)), 0, 0, 0, 0)
    a, b = C.c_double(0.0), C.c_double(0.0)
    check(load().sr_fsim_value(C.byref(rec), C.byref(a), C.byref(b)))
    return float(a.value), float(b.value)


def fsim_chroma_weight(s_i: float, s_q: float) -> float:
    """Host only (sr_fsim_chroma_weight): Re((s_i s_q)^0.03) as the score kernel forms it."""
    return float(load().sr_fsim_chroma_weight(float(s_i), float(s_q)))


def vsi_plan(h: int, w: int, cn: int) -> dict:
    """Host only (sr_vsi_plan): F, the pooled size and the bytes of context workspace of a VSI call.  ValueError for cn not 1,
    3 or 4; SrShapeError (a ValueError) naming the minimum for a side below 16; SrNativeError for cn = 1 (VSI is defined for
    colour images) and, naming the cap, for F above 256."""
    h, w, cn = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn")))
    f, rows, cols, nbytes = C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    check(load().sr_vsi_plan(h, w, cn, C.byref(f), C.byref(rows), C.byref(cols), C.byref(nbytes)))
    return {"F": f.value, "size": (rows.value, cols.value), "workspace_bytes": int(nbytes.value)}


def vsi_filter() -> dict:
    """Host only (sr_vsi_filter): {'lg': [256, 256] (DC first), 'sd': [256, 256]} of the SDSP grid."""
    lg, sd = np.zeros((VSI_GRID, VSI_GRID), np.float64), np.zeros((VSI_GRID, VSI_GRID), np.float64)
    dp = C.POINTER(C.c_double)
    check(load().sr_vsi_filter(lg.ctypes.data_as(dp), sd.ctypes.data_as(dp)))
    return {"lg": lg, "sd": sd}


def vsi_resize_weights(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """Host only (sr_vsi_resize_weights): (w [n_out, taps] float64, idx [n_out, taps] int32, reflected and 0-based) of one
    axis of the triangle resize n_in -> n_out (imresize 'bilinear', antialiased when it shrinks)."""
    n_in, n_out = _whole(n_in, "n_in"), _whole(n_out, "n_out")
    taps = C.c_int(0)
    check(load().sr_vsi_resize_weights(n_in, n_out, 0, C.byref(taps), None, None))
    w, idx = np.zeros((n_out, taps.value), np.float64), np.zeros((n_out, taps.value), np.int32)
    check(load().sr_vsi_resize_weights(n_in, n_out, taps.value, C.byref(taps), w.ctypes.data_as(C.POINTER(C.c_double)),
                                       idx.ctypes.data_as(C.POINTER(C.c_int32))))
    return w, idx


def _vsi_dict(rec: "VsiSums") -> dict:
    rng = lambda f: np.array([[f[0][0], f[0][1]], [f[1][0], f[1][1]]], np.float64)
    return {"sum_s": rec.sum_s, "sum_w": rec.sum_w, "count": int(rec.count), "F": int(rec.F), "size": (int(rec.rows), int(rec.cols)),
            "a_range": rng(rec.a_range), "b_range": rng(rec.b_range), "vs_range": rng(rec.vs_range)}


def vsi_value(sums: dict) -> float:
    """Host only (sr_vsi_value): sum_s / sum_w of a vsi record; NaN for 0 / 0 or a NaN sum."""
    rec = VsiSums()
    rec.sum_s, rec.sum_w = float(sums["sum_s"]), float(sums["sum_w"])
    return float(load().sr_vsi_value(C.byref(rec)))


def vsi_chroma_weight(s_c: float) -> float:
    """Host only (sr_vsi_chroma_weight): Re(s_c^0.02) as the score kernel forms it."""
    return float(load().sr_vsi_chroma_weight(float(s_c)))


def vsi_host(a: np.ndarray, b: np.ndarray) -> dict:
    """Host only (sr_vsi_host_u8): the float64 restatement of VSI on two u8 host arrays (H x W x 3 / 4; any row stride,
    channels dense) -> the record of Context.vsi.  ValueError as vsi_plan and for shapes that differ."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("vsi_host: need u8 images")
    if a.shape != b.shape or a.ndim not in (2, 3):
        raise ValueError(f"vsi_host: need two H x W x C images of one shape, got {a.shape} vs {b.shape}")
    cn = a.shape[2] if a.ndim == 3 else 1
    arrs = []
    for v in (a, b):
        dense = v.strides[-1] == 1 and (v.ndim == 2 or v.strides[1] == cn) and v.strides[0] >= v.shape[1] * cn
        arrs.append(v if dense else np.ascontiguousarray(v))
    rec = VsiSums()
    check(load().sr_vsi_host_u8(C.c_void_p(arrs[0].ctypes.data), int(arrs[0].strides[0]), C.c_void_p(arrs[1].ctypes.data),
                                int(arrs[1].strides[0]), int(a.shape[0]), int(a.shape[1]), int(cn), C.byref(rec)))
    return _vsi_dict(rec)


def delta_e_formula(formula) -> int:
    """'ciede2000' / 'cie76' (or the enum value) -> enum sr_delta_e_formula.  ValueError for another name; another number goes
    through to the library, which refuses it (SR_ERR_UNSUPPORTED)."""
    if isinstance(formula, str):
        if formula not in DELTA_E_FORMULAS:
            raise ValueError(f"delta E: unknown formula {formula!r}: {sorted(DELTA_E_FORMULAS)} are built (no CIE94, no CMC)")
        return DELTA_E_FORMULAS[formula]
    return _whole(formula, "formula")


def delta_e_plan(h: int, w: int, cn: int, crop_border: int = 0, formula=DELTA_E_2000) -> dict:
    """Host only (sr_delta_e_plan): the cropped size, the pixel count, the blocks of the sums launch and the bytes of context
    scratch of a call.  ValueError for cn not 1, 3 or 4, a negative crop_border or h, w < 1; SrShapeError (a ValueError) for a
    crop that leaves nothing; SrNativeError (SR_ERR_UNSUPPORTED) for an unknown formula."""
    h, w, cn, crop_border = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn"), (crop_border, "crop_border")))
    ch, cw, cnt, blocks, nbytes = C.c_int(0), C.c_int(0), C.c_uint64(0), C.c_int(0), C.c_size_t(0)
    check(load().sr_delta_e_plan(h, w, cn, crop_border, delta_e_formula(formula), C.byref(ch), C.byref(cw), C.byref(cnt),
                                 C.byref(blocks), C.byref(nbytes)))
    return {"size": (ch.value, cw.value), "count": int(cnt.value), "blocks": blocks.value, "scratch_bytes": int(nbytes.value)}


def delta_e_table() -> np.ndarray:
    """Host only (sr_delta_e_table): the 256 linear values of the sRGB bytes."""
    out = np.zeros(256, np.float64)
    check(load().sr_delta_e_table(out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def delta_e_lab(r: int, g: int, b: int) -> np.ndarray:
    """Host only (sr_delta_e_lab_u8): scikit-image's rgb2lab of one uint8 pixel -> [L, a, b].  ValueError outside 0 .. 255."""
    out = (C.c_double * 3)()
    check(load().sr_delta_e_lab_u8(_whole(r, "r"), _whole(g, "g"), _whole(b, "b"), out))
    return np.array(out[:], np.float64)


def delta_e_pair(lab1, lab2, formula=DELTA_E_2000) -> float:
    """Host only (sr_delta_e_pair): the difference of two Lab triples by `formula`, in float64."""
    l1, l2 = (np.asarray(v, np.float64).ravel() for v in (lab1, lab2))
    if l1.size != 3 or l2.size != 3:
        raise ValueError("delta_e_pair: need two Lab triples")
    out = C.c_double(0.0)
    check(load().sr_delta_e_pair((C.c_double * 3)(*l1), (C.c_double * 3)(*l2), delta_e_formula(formula), C.byref(out)))
    return float(out.value)


def _delta_e_record(sums: dict) -> "DeltaESums":
    hist = np.asarray(sums["hist"])
    if hist.shape != (DELTA_E_BINS,):
        raise ValueError(f"delta E record: the histogram must have {DELTA_E_BINS} bins")
    rec = DeltaESums(int(sums["count"]), float(sums["sum"]), float(sums["sum2"]), float(sums["max"]))
    C.memmove(rec.hist, np.ascontiguousarray(hist, dtype=np.uint64).ctypes.data, DELTA_E_BINS * 8)
    return rec


def delta_e_mean_rms(sums: dict) -> Tuple[float, float]:
    """Host only (sr_delta_e_mean, sr_delta_e_rms) of a delta_e_u8 record.  ValueError for an empty record."""
    rec = _delta_e_record(sums)
    m, r = float(load().sr_delta_e_mean(C.byref(rec))), float(load().sr_delta_e_rms(C.byref(rec)))
    if m != m or r != r:
        raise ValueError(last_error())
    return m, r


def delta_e_percentile(sums: dict, p: float) -> float:
    """Host only (sr_delta_e_percentile): the LOWER edge j / 16 of the histogram bin that holds the p-th percentile, p in
    (0, 100]; the true percentile lies in [j / 16, (j + 1) / 16).  ValueError for another p or an empty record."""
    rec = _delta_e_record(sums)
    v = float(load().sr_delta_e_percentile(C.byref(rec), float(p)))
    if v != v:
        raise ValueError(last_error())
    return v


def delta_e_fraction(sums: dict, t: float) -> float:
    """Host only (sr_delta_e_fraction_at_least): the fraction of pixels with dE >= t, exact from the histogram, for t a
    multiple of 1 / 16 in [0, 128).  ValueError for any other t."""
    rec = _delta_e_record(sums)
    out = C.c_double(0.0)
    check(load().sr_delta_e_fraction_at_least(C.byref(rec), float(t), C.byref(out)))
    return float(out.value)


def haarpsi_convention(convention) -> int:
    """'matlab' / 'python' (or the enum value) -> enum sr_haarpsi_convention.  ValueError for another name; another number
    goes through to the library, which refuses it."""
    if isinstance(convention, str):
        if convention not in HAARPSI_CONVENTIONS:
            raise ValueError(f"HaarPSI: unknown convention {convention!r}: {sorted(HAARPSI_CONVENTIONS)} are built")
        return HAARPSI_CONVENTIONS[convention]
    return _whole(convention, "convention")


def _haarpsi_switches(crop_border, subsample, convention) -> Tuple[int, int, int]:
    if not isinstance(subsample, (bool, np.bool_)):
        subsample = _whole(subsample, "subsample")
    return _whole(crop_border, "crop_border"), int(subsample), haarpsi_convention(convention)


def haarpsi_plan(h: int, w: int, cn: int, crop_border: int = 0, subsample=True, convention=HAARPSI_MATLAB) -> dict:
    """Host only (sr_haarpsi_plan): the sample map, its count, the blocks of the launch and the bytes of context scratch of a
    HaarPSI call.  ValueError for cn not 1, 3 or 4, a negative crop_border, h or w < 1, another subsample or convention;
    SrShapeError (a ValueError) naming the minimum for a side below 2 after the crop."""
    h, w, cn = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn")))
    crop_border, subsample, convention = _haarpsi_switches(crop_border, subsample, convention)
    mh, mw, cnt, blocks, nbytes = C.c_int(0), C.c_int(0), C.c_uint64(0), C.c_int(0), C.c_size_t(0)
    check(load().sr_haarpsi_plan(h, w, cn, crop_border, subsample, convention, C.byref(mh), C.byref(mw), C.byref(cnt),
                                 C.byref(blocks), C.byref(nbytes)))
    return {"size": (mh.value, mw.value), "count": int(cnt.value), "blocks": blocks.value, "scratch_bytes": int(nbytes.value)}


def _haarpsi_dict(rec: "HaarPsiSums") -> dict:
    n = int(rec.channels)
    return {"num": np.array(rec.num[:n], np.float64), "den": np.array(rec.den[:n], np.float64), "channels": n,
            "count": int(rec.count)}


def haarpsi_value(sums: dict) -> float:
    """Host only (sr_haarpsi_value): (ln(x / (1 - x)) / 4.2)^2 with x = sum num / sum den of a haarpsi record; NaN when every
    weight is 0 (a black pair).  ValueError for a record of other than 2 or 3 channels."""
    num, den = (np.asarray(sums[k], np.float64).ravel() for k in ("num", "den"))
    if num.size != den.size or num.size not in (2, 3):
        raise ValueError("haarpsi_value: need a record of 2 or 3 channels")
    rec = HaarPsiSums()
    for k in range(num.size):
        rec.num[k], rec.den[k] = float(num[k]), float(den[k])
    rec.channels, rec.count = int(num.size), int(sums.get("count", 0))
    return float(load().sr_haarpsi_value(C.byref(rec)))


def haarpsi_cell_value(num: float, den: float) -> float:
    """Host only (sr_haarpsi_cell_value): the value of one cell's sums; NaN for den == 0."""
    return float(load().sr_haarpsi_cell_value(float(num), float(den)))


def haarpsi_host(a: np.ndarray, b: np.ndarray, crop_border: int = 0, subsample=True, convention=HAARPSI_MATLAB) -> dict:
    """Host only (sr_haarpsi_host_u8): the float64 restatement of HaarPSI on two u8 host arrays (H x W, or H x W x 1 / 3 / 4;
    any row stride, channels dense) -> {'num', 'den', 'channels', 'count'}.  ValueError as haarpsi_plan and for shapes that
    differ."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("haarpsi_host: need u8 images")
    if a.shape != b.shape or a.ndim not in (2, 3):
        raise ValueError(f"haarpsi_host: need two H x W or H x W x C images of one shape, got {a.shape} vs {b.shape}")
    cn = a.shape[2] if a.ndim == 3 else 1
    arrs = []
    for v in (a, b):
        dense = v.strides[-1] == 1 and (v.ndim == 2 or v.strides[1] == cn) and v.strides[0] >= v.shape[1] * cn
        arrs.append(v if dense else np.ascontiguousarray(v))
    crop_border, subsample, convention = _haarpsi_switches(crop_border, subsample, convention)
    rec = HaarPsiSums()
    check(load().sr_haarpsi_host_u8(C.c_void_p(arrs[0].ctypes.data), int(arrs[0].strides[0]), C.c_void_p(arrs[1].ctypes.data),
                                    int(arrs[1].strides[0]), int(a.shape[0]), int(a.shape[1]), int(cn), crop_border, subsample,
                                    convention, C.byref(rec)))
    return _haarpsi_dict(rec)


def mser_params(delta=None, min_area=None, max_area=None, max_variation=None, min_diversity=None) -> "MserParams":
    """sr_mser_default_params with the given fields replaced (None: the default).  ValueError for a count that is not a whole
    number; the ranges are the library's to refuse (NotImplementedError from mser_plan and every call)."""
    p = MserParams()
    check(load().sr_mser_default_params(C.byref(p)))
    for name, v in (("delta", delta), ("min_area", min_area), ("max_area", max_area)):
        if v is not None:
            if isinstance(v, bool) or int(v) != v or not (-2 ** 31 <= int(v) < 2 ** 31):
                raise ValueError(f"mser: {name} must be a whole number, got {v!r}")
            setattr(p, name, int(v))
    if max_variation is not None:
        p.max_variation = float(max_variation)
    if min_diversity is not None:
        p.min_diversity = float(min_diversity)
    return p


def _mser_polarity_mask(polarity_mask) -> int:
    if isinstance(polarity_mask, bool) or polarity_mask not in (MSER_DARK, MSER_BRIGHT, MSER_BOTH):
        raise ValueError(f"mser: polarity_mask must be 1 (dark), 2 (bright) or 3 (both), got {polarity_mask!r}")
    return int(polarity_mask)


def mser_plan(h: int, w: int, params: Optional["MserParams"] = None) -> dict:
    """Host only (sr_mser_plan) -> {'workspace_bytes', 'node_cap'}.  ValueError for h or w < 1; NotImplementedError for every
    refusal of the definition (more than 2^24 pixels, delta outside 1..255, min_area < 1, max_area < min_area, a negative or
    NaN max_variation / min_diversity)."""
    params = params if params is not None else mser_params()
    ws, cap = _sz(0), _i64(0)
    _check_unsupported(load().sr_mser_plan(int(h), int(w), C.byref(params), C.byref(ws), C.byref(cap)))
    return {"workspace_bytes": int(ws.value), "node_cap": int(cap.value)}


def _mser_host_image(img, what: str):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3, 4)) or img.size == 0:
        raise ValueError(f"{what}: need a u8 H x W or H x W x 1 / 3 / 4 image")
    cn = img.shape[2] if img.ndim == 3 else 1
    dense = img.strides[-1] == 1 and (img.ndim == 2 or img.strides[1] == cn) and img.strides[0] >= img.shape[1] * cn
    return (img if dense else np.ascontiguousarray(img)), cn


MSER_FIRST_CAP = 65536            # records of a first buffer: 2.3 MB; text pages stay far below it


def _mser_fetch(call, dtype, cap: int, again=None) -> np.ndarray:
    """call(buffer, cap, count) once with room for cap records; when the count is larger, again(buffer, count, count) (default:
    the same call, which computes everything a second time) fills a buffer of the whole count."""
    out = np.zeros(max(int(cap), 1), dtype=dtype)
    n = _i64(0)
    _check_unsupported(call(C.c_void_p(out.ctypes.data), int(out.shape[0]), C.byref(n)))
    if n.value > out.shape[0]:
        out = np.zeros(int(n.value), dtype=dtype)
        _check_unsupported((again or call)(C.c_void_p(out.ctypes.data), int(out.shape[0]), C.byref(n)))
    return out[:n.value].copy()


def mser_host(img: np.ndarray, params: Optional["MserParams"] = None, polarity_mask: int = MSER_BOTH) -> np.ndarray:
    """Host only (sr_mser_host_u8): the restatement of the MSER definition on a u8 host array -> the regions as a structured
    array (MSER_REGION_DTYPE) in output order.  One run for up to MSER_FIRST_CAP regions; above that the restatement (which
    keeps nothing between calls) runs a second time with room for all of them."""
    img, cn = _mser_host_image(img, "mser_host")
    params = params if params is not None else mser_params()
    mask = _mser_polarity_mask(polarity_mask)
    lib = load()
    return _mser_fetch(lambda buf, cap, n: lib.sr_mser_host_u8(C.c_void_p(img.ctypes.data), int(img.strides[0]), int(img.shape[0]),
                                                               int(img.shape[1]), cn, C.byref(params), mask, buf, cap, n),
                       MSER_REGION_DTYPE, MSER_FIRST_CAP)


def mser_tree_host(img: np.ndarray, polarity: int = 0) -> np.ndarray:
    """Host only (sr_mser_tree_host_u8): the whole node table of one polarity (0 dark, 1 bright) in (level, seed) order
    (MSER_NODE_DTYPE).  The first buffer holds a node per pixel up to 2^20 nodes (one run); a larger table takes a second run
    with the count the first one reported."""
    img, cn = _mser_host_image(img, "mser_tree_host")
    if polarity not in (0, 1):
        raise ValueError(f"mser_tree_host: polarity must be 0 or 1, got {polarity!r}")
    lib = load()
    return _mser_fetch(lambda buf, cap, n: lib.sr_mser_tree_host_u8(C.c_void_p(img.ctypes.data), int(img.strides[0]),
                                                                    int(img.shape[0]), int(img.shape[1]), cn, int(polarity), buf,
                                                                    cap, n),
                       MSER_NODE_DTYPE, min(int(img.shape[0]) * int(img.shape[1]), 1 << 20))


def mser_text_boxes(regions: np.ndarray, image_w: int) -> List[Tuple[int, int, int, int]]:
    """Host only (sr_mser_text_boxes): the (x, y, w, h) boxes of tiling_module.py:231-235 in region order, duplicates kept."""
    regions = np.ascontiguousarray(regions, dtype=MSER_REGION_DTYPE)
    n = int(regions.shape[0])
    rects = (TileRect * max(n, 1))()
    m = _i64(0)
    check(load().sr_mser_text_boxes(C.c_void_p(regions.ctypes.data), n, int(image_w), rects, C.byref(m)))
    return [(rects[i].x, rects[i].y, rects[i].w, rects[i].h) for i in range(m.value)]


def cascade_params(scale_factor=None, min_neighbors=None, min_size=None, max_size=None) -> "CascadeParams":
    """sr_cascade_default_params (1.1, 4, no minimum, the image) with the given fields replaced; sizes are (w, h) as in
    cv2.  ValueError for a count that is not a whole number; the ranges are the library's to refuse."""
    p = CascadeParams()
    check(load().sr_cascade_default_params(C.byref(p)))
    if scale_factor is not None:
        p.scale_factor = float(scale_factor)
    ints = [("min_neighbors", min_neighbors)]
    for name, size in (("min", min_size), ("max", max_size)):
        if size is not None:
            if len(size) != 2:
                raise ValueError(f"cascade: {name}_size must be (w, h), got {size!r}")
            ints += [(f"{name}_w", size[0]), (f"{name}_h", size[1])]
    for name, v in ints:
        if v is not None:
            if isinstance(v, bool) or int(v) != v or not (-2 ** 31 <= int(v) < 2 ** 31):
                raise ValueError(f"cascade: {name} must be a whole number, got {v!r}")
            setattr(p, name, int(v))
    return p


def _cascade_rects(buf: np.ndarray) -> np.ndarray:
    return buf.view(np.int32).reshape(-1, 4)


def cascade_group(cands, min_neighbors: int = 4) -> np.ndarray:
    """Host only (sr_cascade_group): OpenCV's groupRectangles(cands, min_neighbors, 0.2) as the definition states it ->
    int32 [m, 4] boxes (x, y, w, h).  NotImplementedError for a negative min_neighbors."""
    c = np.ascontiguousarray(np.asarray(cands, dtype=np.int32).reshape(-1, 4))
    out = np.zeros((max(len(c), 1), 4), np.int32)
    m = _i64(0)
    _check_unsupported(load().sr_cascade_group(C.c_void_p(c.ctypes.data), len(c), int(min_neighbors), C.c_void_p(out.ctypes.data),
                                               C.byref(m)))
    return out[:m.value].copy()


CASCADE_FIRST_CAP = 65536         # candidates of a first buffer (1 MB); a face image stays far below it


class CascadeModel:
    """sr_cascade: a checked and packed cascade (host only; the tables go to the GPU with every call).  ``tables`` is what
    tiling_module.load_cascade returns.  Every model refusal of the definition (include/sr_hip.h, "Cascade") is raised here
    as NotImplementedError."""

    def __init__(self, tables: dict):
        t = tables
        haar = t["feature_type"] == "HAAR"
        if t["feature_type"] not in ("LBP", "HAAR"):
            raise NotImplementedError(f"cascade: feature type {t['feature_type']!r} is neither LBP nor HAAR (HOG cascades are not built)")
        f32 = lambda k: np.ascontiguousarray(t[k], dtype=np.float32) if t.get(k) is not None else None   # noqa: E731
        i32 = lambda k: np.ascontiguousarray(t[k], dtype=np.int32) if t.get(k) is not None else None     # noqa: E731
        arrs = [f32("stage_thresholds"), i32("stage_counts"), i32("stump_feature"), f32("stump_threshold"), f32("stump_leaves"),
                i32("stump_subsets"), i32("feature_nrects"), i32("feature_rects"), f32("feature_weights")]
        n_stages, n_stumps = len(arrs[0]), len(arrs[2])
        n_feat = 0 if arrs[7] is None else arrs[7].size // (12 if haar else 4)
        want = [n_stages, n_stages, n_stumps, n_stumps if haar else None, 2 * n_stumps, None if haar else 8 * n_stumps,
                n_feat if haar else None, (12 if haar else 4) * n_feat, 3 * n_feat if haar else None]
        for a, n, name in zip(arrs, want, ("stage_thresholds", "stage_counts", "stump_feature", "stump_threshold", "stump_leaves",
                                          "stump_subsets", "feature_nrects", "feature_rects", "feature_weights")):
            if n is not None and (0 if a is None else a.size) != n:
                raise ValueError(f"cascade: table {name} has {0 if a is None else a.size} entries, expected {n}")
        info = CascadeInfo(1 if haar else 0, int(t["window"][0]), int(t["window"][1]), n_stages, n_stumps, n_feat,
                           int(t.get("old_layout", 0)), int(t.get("stage_type", 0)), int(t.get("max_tree_nodes", 1)),
                           int(t.get("tilted", 0)), int(t.get("max_rects", 0)), int(t.get("max_cat_count", 256)))
        self._keep = arrs
        h = C.c_void_p()
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None                   # noqa: E731
        _check_unsupported(load().sr_cascade_create(C.byref(info), *[ptr(a) for a in arrs], C.byref(h)))
        self.handle = h
        self.feature_type, self.window = t["feature_type"], (info.win_w, info.win_h)
        self.n_stages, self.n_stumps, self.n_features = n_stages, n_stumps, n_feat

    def info(self) -> dict:
        d = CascadeInfo()
        check(load().sr_cascade_desc(self.handle, C.byref(d)))
        return {k: getattr(d, k) for k, _ in CascadeInfo._fields_}

    def plan(self, h: int, w: int, params: Optional["CascadeParams"] = None) -> dict:
        """Host only (sr_cascade_plan) -> {'scales': [dict per scale], 'workspace_bytes', 'positions'}.  NotImplementedError
        for every refusal of the arguments."""
        params = params if params is not None else cascade_params()
        sc = (CascadeScale * SR_CASCADE_MAX_SCALES)()
        n, ws, pos = _i(0), _sz(0), _i64(0)
        _check_unsupported(load().sr_cascade_plan(self.handle, int(h), int(w), C.byref(params), sc, SR_CASCADE_MAX_SCALES, C.byref(n),
                                                  C.byref(ws), C.byref(pos)))
        return {"scales": [{k: getattr(sc[i], k) for k, _ in CascadeScale._fields_} for i in range(n.value)],
                "workspace_bytes": int(ws.value), "positions": int(pos.value)}

    def host(self, img: np.ndarray, params: Optional["CascadeParams"] = None) -> np.ndarray:
        """Host only (sr_cascade_host_u8): the raw candidates int32 [n, 4] (x, y, w, h) in canonical order."""
        img, cn = _mser_host_image(img, "cascade_host")
        params = params if params is not None else cascade_params()
        lib = load()
        return _cascade_rects(_mser_fetch(lambda buf, cap, n: lib.sr_cascade_host_u8(
            self.handle, C.c_void_p(img.ctypes.data), int(img.strides[0]), int(img.shape[0]), int(img.shape[1]), cn, C.byref(params),
            buf, cap, n), CASCADE_RECT_DTYPE, CASCADE_FIRST_CAP))

    def plane_host(self, img: np.ndarray, k: int, params: Optional["CascadeParams"] = None) -> np.ndarray:
        """Host only (sr_cascade_plane_host_u8): the scaled plane of scale k of the plan."""
        img, cn = _mser_host_image(img, "cascade_plane_host")
        params = params if params is not None else cascade_params()
        scales = self.plan(img.shape[0], img.shape[1], params)["scales"]
        if not 0 <= int(k) < len(scales):
            raise ValueError(f"cascade_plane_host: scale {k} of {len(scales)}")
        out = np.zeros((scales[k]["sh"], scales[k]["sw"]), np.uint8)
        _check_unsupported(load().sr_cascade_plane_host_u8(self.handle, C.c_void_p(img.ctypes.data), int(img.strides[0]),
                                                           int(img.shape[0]), int(img.shape[1]), cn, C.byref(params), int(k),
                                                           C.c_void_p(out.ctypes.data)))
        return out

    def map_shape(self, h: int, w: int, step: int) -> Tuple[int, int]:
        if step not in (1, 2):
            raise ValueError(f"cascade: step must be 1 or 2, got {step!r}")
        if w < self.window[0] or h < self.window[1]:
            return 0, 0
        return (h - self.window[1]) // step + 1, (w - self.window[0]) // step + 1

    def stage_map_host(self, img: np.ndarray, step: int = 1) -> np.ndarray:
        """Host only (sr_cascade_stage_map_host_u8): int32 [ny, nx], the number of stages each window of the gray plane
        itself passes."""
        img, cn = _mser_host_image(img, "cascade_stage_map_host")
        ny, nx = self.map_shape(img.shape[0], img.shape[1], step)
        out = np.zeros(max(ny * nx, 1), np.int32)
        n = _i64(0)
        _check_unsupported(load().sr_cascade_stage_map_host_u8(self.handle, C.c_void_p(img.ctypes.data), int(img.strides[0]),
                                                               int(img.shape[0]), int(img.shape[1]), cn, int(step),
                                                               C.c_void_p(out.ctypes.data), ny * nx, C.byref(n)))
        assert n.value == ny * nx
        return out[:ny * nx].reshape(ny, nx)

    def close(self):
        if getattr(self, "handle", None):
            load().sr_cascade_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def imresize_size(n: int, scale: float) -> int:
    """Host only (sr_imresize_size): MATLAB's output length ceil(n * scale), evaluated in double as written.  ValueError for
    n < 1, SrNativeError (SR_ERR_UNSUPPORTED) naming the range for a scale outside [1/16, 16]."""
    m = load().sr_imresize_size(_whole(n, "n"), float(scale))
    if m < 0:
        check(m)
    return int(m)


def imresize_geometry(h: int, w: int, scale=None, output_shape=None) -> Tuple[float, float, int, int]:
    """The two forms of imresize's size argument -> (scale_y, scale_x, dh, dw): a scalar `scale` (both axes use it, sides
    ceil(n * scale)) or `output_shape` = (dh, dw) (the axis scales are dh / h and dw / w).  ValueError for both or neither."""
    if (scale is None) == (output_shape is None):
        raise ValueError("imresize: give exactly one of scale and output_shape")
    h, w = _whole(h, "h"), _whole(w, "w")
    if h < 1 or w < 1:
        raise ValueError(f"imresize: sides must be >= 1 (got {h} x {w})")
    if scale is not None:
        scale = float(scale)
        return scale, scale, imresize_size(h, scale), imresize_size(w, scale)
    if len(output_shape) != 2:
        raise ValueError(f"imresize: output_shape must be (dh, dw), got {output_shape!r}")
    dh, dw = _whole(output_shape[0], "dh"), _whole(output_shape[1], "dw")
    if dh < 1 or dw < 1:
        raise ValueError(f"imresize: sides must be >= 1 (got {dh} x {dw})")
    return dh / h, dw / w, dh, dw


def imresize_weights(n_in: int, n_out: int, scale: float, antialias: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """Host only (sr_imresize_weights): (w[n_out, taps] float64, idx[n_out, taps] int32) of one axis -- the normalised weights
    and the reflected 0-based indices, without the taps that are zero for every output."""
    n_in, n_out = _whole(n_in, "n_in"), _whole(n_out, "n_out")
    taps = C.c_int(0)
    check(load().sr_imresize_weights(n_in, n_out, float(scale), 1 if antialias else 0, 0, C.byref(taps), None, None))
    w, idx = np.zeros((n_out, taps.value), dtype=np.float64), np.zeros((n_out, taps.value), dtype=np.int32)
    check(load().sr_imresize_weights(n_in, n_out, float(scale), 1 if antialias else 0, taps.value, C.byref(taps),
                                     w.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)))
    return w, idx


def imresize_plan(h: int, w: int, cn: int, scale_y: float, scale_x: float, dh: int, dw: int, antialias: bool = True) -> dict:
    """Host only (sr_imresize_plan): the pass order ('vertical' or 'horizontal' first), the tap counts, the output tile of one
    workgroup, its LDS bytes and the bytes of context scratch of an imresize call.  Carries every shape refusal: ValueError,
    or SrNativeError (SR_ERR_UNSUPPORTED) naming the range for a scale outside [1/16, 16]."""
    h, w, cn, dh, dw = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn"), (dh, "dh"), (dw, "dw")))
    order, ty, tx, th, tw, lds, nbytes = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_size_t(0)
    check(load().sr_imresize_plan(h, w, cn, float(scale_y), float(scale_x), dh, dw, 1 if antialias else 0, C.byref(order),
                                  C.byref(ty), C.byref(tx), C.byref(th), C.byref(tw), C.byref(lds), C.byref(nbytes)))
    return {"first": "vertical" if order.value == 0 else "horizontal", "taps": (ty.value, tx.value), "tile": (th.value, tw.value),
            "lds_bytes": int(lds.value), "scratch_bytes": int(nbytes.value)}


def niqe_plan(h: int, w: int, cn: int, crop_border: int = 0) -> dict:
    """Host only (sr_niqe_plan): the kept size (multiples of 96), the block grid and the bytes of context scratch of a NIQE
    call.  ValueError for cn not 1 or 3 or a negative crop_border; SrShapeError (a ValueError) naming the minimum for a side
    below 96 after the crop."""
    h, w, cn, crop_border = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn"), (crop_border, "crop_border")))
    H, W, nby, nbx, nbytes = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    check(load().sr_niqe_plan(h, w, cn, crop_border, C.byref(H), C.byref(W), C.byref(nby), C.byref(nbx), C.byref(nbytes)))
    return {"size": (H.value, W.value), "blocks": (nby.value, nbx.value), "scratch_bytes": int(nbytes.value)}


def _f64(a, shape, name: str) -> np.ndarray:
    out = np.ascontiguousarray(a, dtype=np.float64)
    if out.shape != shape:
        raise ValueError(f"{name}: expected shape {shape}, got {out.shape}")
    return out


def niqe_features(records: np.ndarray) -> np.ndarray:
    """Host only (sr_niqe_features): records[2, nblocks] (NIQE_RECORD, scale-major) -> feat[nblocks, 36]."""
    rec = np.ascontiguousarray(records, dtype=NIQE_RECORD)
    if rec.ndim != 2 or rec.shape[0] != 2 or rec.shape[1] < 1:
        raise ValueError(f"niqe_features: records must be [2, nblocks], got shape {rec.shape}")
    feat = np.zeros((rec.shape[1], NIQE_FEATURES), dtype=np.float64)
    check(load().sr_niqe_features(rec.ctypes.data_as(C.c_void_p), rec.shape[1], feat.ctypes.data_as(C.c_void_p)))
    return feat


def niqe_sharpness(records: np.ndarray) -> np.ndarray:
    """sharp_b = sum_sigma_b(scale 1) / 96^2 of records[2, nblocks]."""
    return np.asarray(records)[0]["sum_sigma"] / float(NIQE_BLOCK * NIQE_BLOCK)


def niqe_fit(feats, sharps, threshold: float = 0.75):
    """Host only (sr_niqe_fit): per-image feature rows [n_i, 36] and sharpness [n_i] -> (mu[36], cov[36, 36], rows used).
    SrShapeError (a ValueError) giving the count when fewer than 37 rows pass."""
    feats = [np.ascontiguousarray(f, dtype=np.float64) for f in feats]
    sharps = [np.ascontiguousarray(s, dtype=np.float64).reshape(-1) for s in sharps]
    if not feats or len(feats) != len(sharps):
        raise ValueError("niqe_fit: need one sharpness array per feature array, and at least one image")
    for f, s in zip(feats, sharps):
        if f.ndim != 2 or f.shape[1] != NIQE_FEATURES or s.shape[0] != f.shape[0]:
            raise ValueError(f"niqe_fit: need [n, 36] features with [n] sharpness, got {f.shape} and {s.shape}")
    off = np.concatenate([[0], np.cumsum([f.shape[0] for f in feats])]).astype(np.int64)
    rows, sharp = np.ascontiguousarray(np.concatenate(feats)), np.ascontiguousarray(np.concatenate(sharps))
    if rows.shape[0] < 1:
        raise ValueError("niqe_fit: no blocks")
    mu, cov, used = np.zeros(NIQE_FEATURES), np.zeros((NIQE_FEATURES, NIQE_FEATURES)), C.c_int64(0)
    check(load().sr_niqe_fit(rows.ctypes.data_as(C.c_void_p), sharp.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                             len(feats), float(threshold), mu.ctypes.data_as(C.c_void_p), cov.ctypes.data_as(C.c_void_p),
                             C.byref(used)))
    return mu, cov, int(used.value)


def niqe_score(feat, mu_pris, cov_pris) -> float:
    """Host only (sr_niqe_score): the NIQE of feature rows [nblocks, 36] under (mu_pris (36,) or (1, 36), cov_pris (36, 36));
    NaN (the reason in last_error()) with fewer than two NaN-free rows.  ValueError for wrong parameter shapes."""
    feat = np.ascontiguousarray(feat, dtype=np.float64)
    if feat.ndim != 2 or feat.shape[1] != NIQE_FEATURES:
        raise ValueError(f"niqe_score: features must be [nblocks, 36], got shape {feat.shape}")
    mu = np.asarray(mu_pris, dtype=np.float64)
    if mu.shape not in ((NIQE_FEATURES,), (1, NIQE_FEATURES)):
        raise ValueError(f"niqe_score: mu_pris must have shape (36,) or (1, 36), got {mu.shape}")
    mu = _f64(mu.reshape(-1), (NIQE_FEATURES,), "niqe_score: mu_pris")
    cov = _f64(cov_pris, (NIQE_FEATURES, NIQE_FEATURES), "niqe_score: cov_pris")
    return float(load().sr_niqe_score(feat.ctypes.data_as(C.c_void_p), feat.shape[0], mu.ctypes.data_as(C.c_void_p),
                                      cov.ctypes.data_as(C.c_void_p)))


def brisque_plan(h: int, w: int, cn: int, crop_border: int = 0) -> dict:
    """Host only (sr_brisque_plan): the cropped size, the half plane's size (sides rounded up) and the bytes of context scratch
    of a BRISQUE call.  ValueError for cn not 1 or 3 or a negative crop_border; SrShapeError (a ValueError) naming the minimum
    for a side below 16 after the crop."""
    h, w, cn, crop_border = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn"), (crop_border, "crop_border")))
    H, W, H2, W2, nbytes = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    check(load().sr_brisque_plan(h, w, cn, crop_border, C.byref(H), C.byref(W), C.byref(H2), C.byref(W2), C.byref(nbytes)))
    return {"size": (H.value, W.value), "half_size": (H2.value, W2.value), "scratch_bytes": int(nbytes.value)}


def brisque_features(records: np.ndarray) -> np.ndarray:
    """Host only (sr_brisque_features): records[2] (BRISQUE_RECORD, scale 1 then scale 2) -> feat[36]."""
    rec = np.ascontiguousarray(records, dtype=BRISQUE_RECORD)
    if rec.shape != (2,):
        raise ValueError(f"brisque_features: records must be [2], got shape {rec.shape}")
    feat = np.zeros(BRISQUE_FEATURES, dtype=np.float64)
    check(load().sr_brisque_features(rec.ctypes.data_as(C.c_void_p), feat.ctypes.data_as(C.c_void_p)))
    return feat


_BRISQUE_KEYS = ("sv", "sv_coef", "gamma", "rho", "feature_min", "feature_max")


def check_brisque_model(model) -> dict:
    """-> {'sv': float64 (n_sv, 36), 'sv_coef': (n_sv,), 'gamma', 'rho': float, 'feature_min', 'feature_max': (36,), 'lower',
    'upper': float (default -1, 1)}; ValueError for missing keys, other shapes, n_sv < 1 or a gamma that is not finite and
    positive (sv_coef may come as (n_sv,) or (1, n_sv), libsvm's dual_coef_)."""
    try:
        got = {k: model[k] for k in _BRISQUE_KEYS}
        lower = model["lower"] if "lower" in model else -1.0
        upper = model["upper"] if "upper" in model else 1.0
    except (KeyError, TypeError, IndexError) as exc:
        raise ValueError("a BRISQUE model needs the keys " + ", ".join(repr(k) for k in _BRISQUE_KEYS)) from exc
    sv = np.asarray(got["sv"], dtype=np.float64)
    if sv.ndim != 2 or sv.shape[1] != BRISQUE_FEATURES or sv.shape[0] < 1:
        raise ValueError(f"BRISQUE model: sv must have shape (n_sv >= 1, 36), got {sv.shape}")
    coef = np.asarray(got["sv_coef"], dtype=np.float64)
    if coef.shape not in ((sv.shape[0],), (1, sv.shape[0])):
        raise ValueError(f"BRISQUE model: sv_coef must have shape ({sv.shape[0]},) or (1, {sv.shape[0]}), got {coef.shape}")
    out = {"sv": np.ascontiguousarray(sv), "sv_coef": np.ascontiguousarray(coef.reshape(-1))}
    for k in ("gamma", "rho", "lower", "upper"):
        v = np.asarray({"lower": lower, "upper": upper}.get(k, got.get(k)), dtype=np.float64)
        if v.size != 1 or not np.isfinite(v).all():
            raise ValueError(f"BRISQUE model: {k} must be one finite number")
        out[k] = float(v.reshape(-1)[0])
    if not out["gamma"] > 0.0:
        raise ValueError(f"BRISQUE model: gamma must be positive (got {out['gamma']})")
    for k in ("feature_min", "feature_max"):
        v = np.asarray(got[k], dtype=np.float64)
        if v.shape not in ((BRISQUE_FEATURES,), (1, BRISQUE_FEATURES)):
            raise ValueError(f"BRISQUE model: {k} must have shape (36,) or (1, 36), got {v.shape}")
        out[k] = np.ascontiguousarray(v.reshape(-1))
    return out


def brisque_score(feat, model) -> float:
    """Host only (sr_brisque_score): the score of feat[36] under a model (check_brisque_model's form); NaN for any NaN
    feature.  ValueError for wrong shapes."""
    m = check_brisque_model(model)
    f = _f64(np.asarray(feat, dtype=np.float64).reshape(-1), (BRISQUE_FEATURES,), "brisque_score: features")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return float(load().sr_brisque_score(p(f), p(m["sv"]), p(m["sv_coef"]), m["sv"].shape[0], m["gamma"], m["rho"],
                                         p(m["feature_min"]), p(m["feature_max"]), m["lower"], m["upper"]))


def save_brisque_model(path: str, model) -> None:
    """A flat .npz: sv, sv_coef, gamma, rho, feature_min, feature_max, lower, upper."""
    m = check_brisque_model(model)
    if not str(path).lower().endswith(".npz"):
        raise ValueError(f"BRISQUE model files are .npz, got {path!r}")
    with open(str(path), "wb") as f:
        np.savez(f, **{k: np.asarray(v, dtype=np.float64) for k, v in m.items()})


def load_brisque_model(path: str) -> dict:
    """Reads what save_brisque_model writes (lower / upper optional, default -1 / 1); nothing is unpickled."""
    if not str(path).lower().endswith(".npz"):
        raise ValueError(f"BRISQUE model files are .npz, got {path!r}")
    with np.load(str(path), allow_pickle=False) as z:
        missing = [k for k in _BRISQUE_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: no {' / '.join(missing)}")
        return check_brisque_model({k: z[k] for k in z.files if k in _BRISQUE_KEYS + ("lower", "upper")})


def brisque_model_from_libsvm(model_path: str, range_path: str) -> dict:
    """A model from libsvm's text model file (svm-train's output) and svm-scale's range file.  Only svm_type epsilon_svr with
    kernel_type rbf is BRISQUE's regressor: anything else is refused by name.  Support vectors are sparse index:value lists
    (1-based, absent = 0); a feature absent from the range file was constant in training (feature_min = feature_max)."""
    header, sv, coef = {}, [], []
    with open(str(model_path)) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    if "SV" not in lines:
        raise ValueError(f"{model_path}: no SV section")
    at = lines.index("SV")
    for ln in lines[:at]:
        key, _, val = ln.partition(" ")
        header[key] = val.strip()
    if header.get("svm_type") != "epsilon_svr":
        raise ValueError(f"{model_path}: svm_type {header.get('svm_type')!r} is not supported (need epsilon_svr)")
    if header.get("kernel_type") != "rbf":
        raise ValueError(f"{model_path}: kernel_type {header.get('kernel_type')!r} is not supported (need rbf)")
    for key in ("gamma", "rho"):
        if key not in header:
            raise ValueError(f"{model_path}: no {key}")
    for ln in lines[at + 1:]:
        parts = ln.split()
        row = np.zeros(BRISQUE_FEATURES)
        for item in parts[1:]:
            idx, _, val = item.partition(":")
            k = int(idx)
            if not 1 <= k <= BRISQUE_FEATURES:
                raise ValueError(f"{model_path}: feature index {k} outside 1 .. 36")
            row[k - 1] = float(val)
        coef.append(float(parts[0]))
        sv.append(row)
    if "total_sv" in header and int(header["total_sv"]) != len(sv):
        raise ValueError(f"{model_path}: total_sv {header['total_sv']} but {len(sv)} support vectors")
    with open(str(range_path)) as f:
        rl = [ln.split() for ln in f if ln.strip()]
    if len(rl) < 2 or rl[0] != ["x"] or len(rl[1]) != 2:
        raise ValueError(f"{range_path}: not an svm-scale range file of the features ('x', then 'lower upper')")
    fmin, fmax = np.zeros(BRISQUE_FEATURES), np.zeros(BRISQUE_FEATURES)
    for parts in rl[2:]:
        k = int(parts[0])
        if len(parts) != 3 or not 1 <= k <= BRISQUE_FEATURES:
            raise ValueError(f"{range_path}: bad line {' '.join(parts)!r}")
        fmin[k - 1], fmax[k - 1] = float(parts[1]), float(parts[2])
    return check_brisque_model({"sv": np.array(sv).reshape(-1, BRISQUE_FEATURES), "sv_coef": np.array(coef),
                                "gamma": float(header["gamma"]), "rho": float(header["rho"]), "feature_min": fmin,
                                "feature_max": fmax, "lower": float(rl[1][0]), "upper": float(rl[1][1])})


def psnr_from_sse(sse: int, count: int, data_range: float = 255.0) -> float:
    return float(load().sr_psnr_from_sse(C.c_uint64(sse), C.c_uint64(count), data_range))


# ------------------------------------------------------------------------------------------
# device context
# ------------------------------------------------------------------------------------------
class DeviceBuffer:
    """Owned HBM allocation."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(ctx.lib.sr_dev_alloc(ctx.handle, max(self.nbytes, 1), C.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr and self.ctx.handle:
            self.ctx.lib.sr_dev_free(self.ctx.handle, C.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001
            pass


class Context:
    """One GPU + one stream (sr_ctx).  Thread-compatible: calls are serialised inside the library."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = load()
        h = C.c_void_p()
        if stream is None:
            check(self.lib.sr_ctx_create(int(device), C.byref(h)))
        else:
            check(self.lib.sr_ctx_create_on_stream(int(device), C.c_void_p(stream), C.byref(h)))
        self.handle = h
        self.device = int(device)
        self.h2d_bytes = 0               # bytes moved by upload() / download() (transfer accounting for the tests and
        self.d2h_bytes = 0               # the device-resident pipeline's "one upload, one download" claim)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.sr_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def sync(self):
        check(self.lib.sr_ctx_sync(self.handle))

    def num_cu(self) -> int:
        """Compute units of the device (the launch-shape rules are sized by it)."""
        n = C.c_int(0)
        check(self.lib.sr_ctx_num_cu(self.handle, C.byref(n)))
        return n.value

    # memory ---------------------------------------------------------------------------
    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def upload(self, arr: np.ndarray) -> DeviceBuffer:
        arr = np.ascontiguousarray(arr)
        buf = DeviceBuffer(self, arr.nbytes)
        check(self.lib.sr_memcpy_h2d(self.handle, C.c_void_p(buf.ptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        self.h2d_bytes += arr.nbytes
        return buf

    def download(self, ptr: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        check(self.lib.sr_memcpy_d2h(self.handle, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes))
        self.d2h_bytes += out.nbytes
        return out

    def memset(self, ptr: int, value: int, nbytes: int):
        check(self.lib.sr_memset_d(self.handle, C.c_void_p(ptr), value, nbytes))

    def copy_d2d(self, dst: int, src: int, nbytes: int):
        """sr_memcpy_d2d: nbytes from one device address to another (rows of a strided view are copied one call each)."""
        check(self.lib.sr_memcpy_d2d(self.handle, C.c_void_p(dst), C.c_void_p(src), int(nbytes)))

    # profiling ------------------------------------------------------------------------
    def prof_enable(self, on: bool = True):
        check(self.lib.sr_prof_enable(self.handle, 1 if on else 0))

    def prof_select(self, name: Optional[str] = None):
        """Time only this kernel family (None: all)."""
        check(self.lib.sr_prof_select(self.handle, name.encode() if name else None))

    def prof_reset(self):
        check(self.lib.sr_prof_reset(self.handle))

    def prof_get(self):
        n = C.c_int(0)
        recs = (ProfRecord * 64)()
        check(self.lib.sr_prof_get(self.handle, recs, 64, C.byref(n)))
        return {recs[i].name.decode(): (recs[i].ms, recs[i].launches) for i in range(min(n.value, 64))}

    # device-pointer ops ------------------------------------------------------------------
    def tile_extract_pad(self, d_img: int, img_h, img_w, cn, img_stride, xywh, block, pad_mode: str, d_tiles: int):
        n = len(xywh)
        flat = (C.c_int * (4 * n))(*[int(v) for t in xywh for v in t])
        check(self.lib.sr_tile_extract_pad(self.handle, C.c_void_p(d_img), img_h, img_w, cn, img_stride, flat, n,
                                           block, PAD_MODES[pad_mode], C.c_void_p(d_tiles)))

    def tile_extract(self, d_img: int, img_h, img_w, cn, img_stride, xywh, d_tiles: Sequence[int],
                     strides: Sequence[int]):
        n = len(xywh)
        flat = (C.c_int * (4 * n))(*[int(v) for t in xywh for v in t])
        ptrs = (C.c_void_p * n)(*[C.c_void_p(p) for p in d_tiles])
        st = (C.c_int64 * n)(*[int(s) for s in strides])
        check(self.lib.sr_tile_extract(self.handle, C.c_void_p(d_img), img_h, img_w, cn, img_stride, flat, n, ptrs, st))

    def sse_u8(self, d_a: int, stride_a: int, d_b: int, stride_b: int, h: int, rowlen: int) -> int:
        out = C.c_uint64(0)
        check(self.lib.sr_sse_u8(self.handle, C.c_void_p(d_a), stride_a, C.c_void_p(d_b), stride_b, h, rowlen,
                                 C.byref(out)))
        return out.value

    def seam_scan(self, d_canvas: int, canvas_stride: int, canvas_h: int, canvas_w: int, cn: int, rects_xywh,
                  d_tiles: Sequence[int], strides: Sequence[int], window: int, stride: int, threshold: float,
                  gray_shift: int = 15):
        """-> [(tile, x, y, score)] of the windows below threshold, sorted by (tile, y, x)."""
        n = len(rects_xywh)
        rects = (TileRect * n)(*[TileRect(int(x), int(y), int(w), int(h)) for (x, y, w, h) in rects_xywh])
        ptrs = (C.c_void_p * n)(*[C.c_void_p(p) for p in d_tiles])
        st = (C.c_int64 * n)(*[int(s) for s in strides])
        cap = 1 << 18                  # records the first pass can return; a fuller scan is repeated once with room
        while True:
            recs = (SeamRecord * cap)()
            cnt = C.c_int(0)
            check(self.lib.sr_seam_scan(self.handle, C.c_void_p(d_canvas), canvas_stride, canvas_h, canvas_w, cn, rects,
                                        ptrs, st, n, window, stride, gray_shift, threshold, recs, cap, C.byref(cnt)))
            if cnt.value <= cap:
                break
            cap = cnt.value
        arr = np.frombuffer(recs, dtype=np.dtype([("tile", "<i4"), ("x", "<i4"), ("y", "<i4"), ("pad", "<i4"),
                                                  ("score", "<f8")]), count=cnt.value)
        arr = arr[np.lexsort((arr["x"], arr["y"], arr["tile"]))]
        return list(zip(arr["tile"].tolist(), arr["x"].tolist(), arr["y"].tolist(), arr["score"].tolist()))

    def sse_f32(self, d_a: int, stride_a: int, d_b: int, stride_b: int, h: int, rowlen: int) -> float:
        out = C.c_double(0.0)
        check(self.lib.sr_sse_f32(self.handle, C.c_void_p(d_a), stride_a, C.c_void_p(d_b), stride_b, h, rowlen, C.byref(out)))
        return out.value

    def sse_u8_async(self, d_a, stride_a, d_b, stride_b, h, rowlen, d_out: int):
        check(self.lib.sr_sse_u8_async(self.handle, C.c_void_p(d_a), stride_a, C.c_void_p(d_b), stride_b, h, rowlen,
                                       C.c_void_p(d_out)))

    def ssim_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, mode: str, gray_shift=15, data_range=255.0,
                row_begin=0, row_end=None) -> Tuple[float, int]:
        s, n = C.c_double(0.0), C.c_uint64(0)
        check(self.lib.sr_ssim_u8(self.handle, C.c_void_p(d_a), stride_a, C.c_void_p(d_b), stride_b, h, w, cn,
                                  SSIM_MODES[mode], gray_shift, data_range, row_begin,
                                  h if row_end is None else row_end, C.byref(s), C.byref(n)))
        return s.value, n.value

    def ssim_float(self, d_a, stride_a, d_b, stride_b, h, w, cn, dtype, mode: str, data_range=255.0, row_begin=0, row_end=None):
        """sr_ssim_float: (sum, count) of the SSIM map of two float32 (dtype SR_F32) or float64 (SR_F64) images."""
        s, n = C.c_double(0.0), C.c_uint64(0)
        check(self.lib.sr_ssim_float(self.handle, int(dtype), C.c_void_p(d_a), stride_a, C.c_void_p(d_b), stride_b, h, w, cn,
                                     SSIM_MODES[mode], float(data_range), row_begin, h if row_end is None else row_end,
                                     C.byref(s), C.byref(n)))
        return s.value, n.value

    def ssim_u8_async(self, d_a, stride_a, d_b, stride_b, h, w, cn, mode: str, d_sum: int, gray_shift=15,
                      data_range=255.0, row_begin=0, row_end=None) -> int:
        n = C.c_uint64(0)
        check(self.lib.sr_ssim_u8_async(self.handle, C.c_void_p(d_a), stride_a, C.c_void_p(d_b), stride_b, h, w, cn,
                                        SSIM_MODES[mode], gray_shift, data_range, row_begin,
                                        h if row_end is None else row_end, C.c_void_p(d_sum), C.byref(n)))
        return n.value

    def assess_u8_async(self, d_a, stride_a, d_b, stride_b, h, w, cn, d_out: int, flags=ASSESS_ALL, gray_shift=15,
                        data_range=255.0, row_begin=0, row_end=None):
        """Fused PSNR-SSE + SSIM partial sums -> 4 doubles at d_out (sse, uniform, gauss, simple); no sync."""
        check(self.lib.sr_assess_u8_async(self.handle, C.c_void_p(d_a), stride_a, C.c_void_p(d_b), stride_b, h, w, cn,
                                          gray_shift, data_range, row_begin, h if row_end is None else row_end,
                                          flags, C.c_void_p(d_out)))

    def assess_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, flags=ASSESS_ALL, gray_shift=15, data_range=255.0,
                  row_begin=0, row_end=None) -> dict:
        out = AssessSums()
        check(self.lib.sr_assess_u8(self.handle, C.c_void_p(d_a), stride_a, C.c_void_p(d_b), stride_b, h, w, cn,
                                    gray_shift, data_range, row_begin, h if row_end is None else row_end, flags,
                                    C.byref(out)))
        return {"sse": out.sse, "ssim_uniform": out.ssim_uniform, "ssim_gauss": out.ssim_gauss,
                "ssim_simple": out.ssim_simple}

    def quality_map_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, x_edges, y_edges, flags=ASSESS_ALL, gray_shift=15,
                       data_range=255.0) -> dict:
        """sr_quality_map_u8: the assess_u8 sums per cell of the separable grid x_edges x y_edges -> (gh, gw) arrays 'sse'
        (uint64, exact) and 'ssim_uniform' / 'ssim_gauss' / 'ssim_simple' (float64 sums over the cell's valid samples;
        divide by quality_map_counts).  Every argument is checked before the device is touched (ValueError)."""
        if cn not in (1, 3):
            raise ValueError("quality_map_u8: need 1 or 3 channels")
        if gray_shift not in (14, 15):
            raise ValueError("quality_map_u8: gray_shift must be 14 or 15")
        if int(flags) & ~ASSESS_ALL:
            raise ValueError(f"quality_map_u8: unknown flag bits 0x{int(flags) & ~ASSESS_ALL:x}")
        if h < 1 or w < 1:
            raise ValueError("quality_map_u8: need h, w >= 1")
        xe, gw = _edge_array(x_edges, "x_edges")
        ye, gh = _edge_array(y_edges, "y_edges")
        probe = np.zeros(gh * gw, dtype=np.uint64)                      # the library's own edge check, host only
        check(load().sr_quality_map_counts(int(h), int(w), SSIM_MODES["simple"], xe, gw, ye, gh,
                                           probe.ctypes.data_as(C.POINTER(C.c_uint64))))
        recs = (QualityCell * (gh * gw))()
        check(self.lib.sr_quality_map_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h),
                                         int(w), int(cn), int(gray_shift), float(data_range), xe, gw, ye, gh, int(flags), recs))
        arr = np.frombuffer(recs, dtype=np.dtype([("sse", "<u8"), ("ssim_uniform", "<f8"), ("ssim_gauss", "<f8"),
                                                  ("ssim_simple", "<f8")])).reshape(gh, gw)
        return {k: np.ascontiguousarray(arr[k]) for k in ("sse", "ssim_uniform", "ssim_gauss", "ssim_simple")}

    def ms_ssim_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, levels=5, gray_shift=15, data_range=255.0):
        """sr_ms_ssim_u8 -> [(sum of l cs, sum of cs, count)] per level (S_j = sum_lcs / count, CS_j = sum_cs / count; finish
        with ms_ssim_value).  Every argument is checked before the device is touched: ValueError, or its subclass
        SrShapeError for a short stride or an image too small for `levels`."""
        levels = _whole(levels, "levels")
        if not d_a or not d_b:
            raise ValueError("ms_ssim_u8: null image pointer")
        n = max(1, min(levels, MS_SSIM_MAX_LEVELS))
        out = (MsSsimLevel * n)()
        check(self.lib.sr_ms_ssim_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h), int(w),
                                     int(cn), int(gray_shift), float(data_range), levels, out))
        return [(out[j].sum_lcs, out[j].sum_cs, int(out[j].count)) for j in range(n)]

    def bench_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, crop_border=0, mode=BENCH_Y, data_range=255.0) -> dict:
        """sr_bench_u8 -> {'sse', 'ssim_sum', 'n_elems', 'n_map'} of the two images cropped by crop_border (finish with
        bench_values).  Every argument is checked before the device is touched: ValueError, or its subclass SrShapeError
        for a short stride or a crop that leaves a side below 11."""
        crop_border, mode = _whole(crop_border, "crop_border"), _whole(mode, "mode")
        if not d_a or not d_b:
            raise ValueError("bench_u8: null image pointer")
        out = BenchSums()
        check(self.lib.sr_bench_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h), int(w),
                                   int(cn), crop_border, mode, float(data_range), C.byref(out)))
        return {"sse": out.sse, "ssim_sum": out.ssim_sum, "n_elems": int(out.n_elems), "n_map": int(out.n_map)}

    def vif_u8(self, d_ref, stride_ref, d_dist, stride_dist, h, w, cn, crop_border=0, mode=BENCH_Y) -> list:
        """sr_vif_u8 -> [(num_s, den_s, count)] of the four scales, d_ref the reference and d_dist the distorted image, both
        cropped by crop_border (finish with vif_value).  Every argument is checked before the device is touched: ValueError,
        or its subclass SrShapeError for a short stride or a crop that leaves a side below 41."""
        crop_border, mode = _whole(crop_border, "crop_border"), _whole(mode, "mode")
        if not d_ref or not d_dist:
            raise ValueError("vif_u8: null image pointer")
        out = (VifScale * VIF_SCALES)()
        check(self.lib.sr_vif_u8(self.handle, C.c_void_p(d_ref), int(stride_ref), C.c_void_p(d_dist), int(stride_dist), int(h), int(w),
                                 int(cn), crop_border, mode, out))
        return [(out[s].num, out[s].den, int(out[s].count)) for s in range(VIF_SCALES)]

    def gmsd_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, crop_border=0, mode=BENCH_Y) -> dict:
        """sr_gmsd_u8 -> {'sum_d', 'sum_d2', 'count'} of the two images cropped by crop_border (finish with gmsd_value).  Every
        argument is checked before the device is touched: ValueError, or its subclass SrShapeError for a short stride or a
        crop that leaves a side below 4."""
        crop_border, mode = _whole(crop_border, "crop_border"), _whole(mode, "mode")
        if not d_a or not d_b:
            raise ValueError("gmsd_u8: null image pointer")
        out = GmsdSums()
        check(self.lib.sr_gmsd_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h), int(w),
                                  int(cn), crop_border, mode, C.byref(out)))
        return {"sum_d": out.sum_d, "sum_d2": out.sum_d2, "count": int(out.count)}

    def fsim_pool_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, F) -> np.ndarray:
        """sr_fsim_pool_u8 -> int64 [2 images, 3 (Y, I, Q times 1000), rows, cols]: the window sums of FSIM's pooling with an
        explicit F (1 .. 256), rows x cols = ceil(h / F) x ceil(w / F).  Every argument is checked before the device is touched."""
        h, w, cn, F = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn"), (F, "F")))
        if not d_a or not d_b:
            raise ValueError("fsim_pool_u8: null image pointer")
        if h < 1 or w < 1 or F < 1:
            raise ValueError("fsim_pool_u8: need h, w, F >= 1")
        out = np.zeros((2, 3, (h + F - 1) // F, (w + F - 1) // F), np.int64)
        check(self.lib.sr_fsim_pool_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), h, w, cn, F,
                                       out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def fsim_pc_f64(self, d_plane, rows, cols, d_pc) -> dict:
        """sr_fsim_pc_f64: the phase congruency of the dense float64 device plane d_plane (rows x cols) into the dense device
        plane d_pc -> {'median': [4], 'T': [4]} of the four orientations."""
        rows, cols = _whole(rows, "rows"), _whole(cols, "cols")
        if not d_plane or not d_pc:
            raise ValueError("fsim_pc_f64: null plane pointer")
        med, thr = (C.c_double * 4)(), (C.c_double * 4)()
        check(self.lib.sr_fsim_pc_f64(self.handle, C.c_void_p(d_plane), rows, cols, C.c_void_p(d_pc), med, thr))
        return {"median": np.array(med[:], np.float64), "T": np.array(thr[:], np.float64)}

    def fsim_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn) -> dict:
        """sr_fsim_u8 -> {'sum_s', 'sum_sc', 'sum_pcm', 'count', 'F', 'size'} of the pair (finish with fsim_value).  Every argument
        is checked before the device is touched: ValueError, its subclass SrShapeError for a short stride or a side below 16,
        SrNativeError for a pooled side above 2048."""
        if not d_a or not d_b:
            raise ValueError("fsim_u8: null image pointer")
        out = FsimSums()
        check(self.lib.sr_fsim_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h), int(w),
                                  int(cn), C.byref(out)))
        return {"sum_s": out.sum_s, "sum_sc": out.sum_sc, "sum_pcm": out.sum_pcm, "count": int(out.count), "F": int(out.F),
                "size": (int(out.rows), int(out.cols))}

    def vsi_pool_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, F) -> np.ndarray:
        """sr_vsi_pool_u8 -> int64 [2 images, 3 (L, M, N times 100), rows, cols]: the window sums of VSI's pooling with an
        explicit F (1 .. 256), rows x cols = ceil(h / F) x ceil(w / F).  Every argument is checked before the device is touched."""
        h, w, cn, F = (_whole(v, n) for v, n in ((h, "h"), (w, "w"), (cn, "cn"), (F, "F")))
        if not d_a or not d_b:
            raise ValueError("vsi_pool_u8: null image pointer")
        if h < 1 or w < 1 or F < 1:
            raise ValueError("vsi_pool_u8: need h, w, F >= 1")
        out = np.zeros((2, 3, (h + F - 1) // F, (w + F - 1) // F), np.int64)
        check(self.lib.sr_vsi_pool_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), h, w, cn, F,
                                      out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def vsi_saliency(self, d_img, stride, h, w, cn) -> dict:
        """sr_vsi_saliency_u8 -> {'lab': [3, 256, 256], 'vs256': [256, 256], 'range': [min a, max a, min b, max b]} of ONE image:
        the SDSP saliency on its fixed grid, for inspection.  Refusals as vsi."""
        if not d_img:
            raise ValueError("vsi_saliency: null image pointer")
        lab, vs, rng = np.zeros((3, VSI_GRID, VSI_GRID), np.float64), np.zeros((VSI_GRID, VSI_GRID), np.float64), np.zeros(4, np.float64)
        dp = C.POINTER(C.c_double)
        check(self.lib.sr_vsi_saliency_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w), int(cn), lab.ctypes.data_as(dp),
                                          vs.ctypes.data_as(dp), rng.ctypes.data_as(dp)))
        return {"lab": lab, "vs256": vs, "range": rng}

    def vsi(self, d_a, stride_a, d_b, stride_b, h, w, cn) -> dict:
        """sr_vsi_u8 -> {'sum_s', 'sum_w', 'count', 'F', 'size', 'a_range', 'b_range', 'vs_range' ([2 images, (min, max)])} of the
        pair (finish with vsi_value).  Every argument is checked before the device is touched: ValueError, its subclass
        SrShapeError for a short stride or a side below 16, SrNativeError for a gray image or F above 256."""
        if not d_a or not d_b:
            raise ValueError("vsi: null image pointer")
        out = VsiSums()
        check(self.lib.sr_vsi_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h), int(w),
                                 int(cn), C.byref(out)))
        return _vsi_dict(out)

    def delta_e_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, crop_border=0, formula=DELTA_E_2000, d_map=0,
                   map_stride=0) -> dict:
        """sr_delta_e_u8 -> {'count', 'sum', 'sum2', 'max', 'hist' (uint64[2048], bins of width 1 / 16)} of the per-pixel colour
        difference of the two images cropped by crop_border (finish with delta_e_mean_rms / delta_e_percentile /
        delta_e_fraction).  d_map: a device address that receives the float64 dE of every cropped pixel, map_stride bytes per
        row (0: dense).  Every argument is checked before the device is touched: ValueError, or its subclass SrShapeError for
        a short stride or a crop that leaves nothing."""
        crop_border, formula = _whole(crop_border, "crop_border"), delta_e_formula(formula)
        if not d_a or not d_b:
            raise ValueError("delta_e_u8: null image pointer")
        if d_map and not map_stride:
            map_stride = 8 * max(int(w) - 2 * crop_border, 0)
        out = DeltaESums()
        check(self.lib.sr_delta_e_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h), int(w),
                                     int(cn), crop_border, formula, C.c_void_p(d_map or None), int(map_stride), C.byref(out)))
        return {"count": int(out.count), "sum": out.sum, "sum2": out.sum2, "max": out.max,
                "hist": np.frombuffer(out.hist, dtype=np.uint64).copy()}

    def delta_e_cells_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, x_edges, y_edges, crop_border=0,
                         formula=DELTA_E_2000) -> dict:
        """sr_delta_e_cells_u8: the colour difference per cell of the separable grid x_edges x y_edges over the CROPPED
        rectangle -> (gh, gw) float64 arrays 'sum' and 'max' (a cell's pixel count is its area).  Every argument is checked
        before the device is touched (ValueError)."""
        crop_border, formula = _whole(crop_border, "crop_border"), delta_e_formula(formula)
        if not d_a or not d_b:
            raise ValueError("delta_e_cells_u8: null image pointer")
        xe, gw = _edge_array(x_edges, "x_edges")
        ye, gh = _edge_array(y_edges, "y_edges")
        recs = (DeltaECell * (gh * gw))()
        check(self.lib.sr_delta_e_cells_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h),
                                           int(w), int(cn), crop_border, formula, xe, gw, ye, gh, recs))
        arr = np.frombuffer(recs, dtype=np.dtype([("sum", "<f8"), ("max", "<f8")])).reshape(gh, gw)
        return {k: np.ascontiguousarray(arr[k]) for k in ("sum", "max")}

    def haarpsi(self, d_a, stride_a, d_b, stride_b, h, w, cn, crop_border=0, subsample=True, convention=HAARPSI_MATLAB) -> dict:
        """sr_haarpsi_u8 -> {'num', 'den' (float64 [channels]: V, H and, for colour, chroma), 'channels', 'count'} of the two
        images cropped by crop_border (finish with haarpsi_value).  Every argument is checked before the device is touched:
        ValueError, or its subclass SrShapeError for a short stride or a crop that leaves a side below 2."""
        crop_border, subsample, convention = _haarpsi_switches(crop_border, subsample, convention)
        if not d_a or not d_b:
            raise ValueError("haarpsi: null image pointer")
        out = HaarPsiSums()
        check(self.lib.sr_haarpsi_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h), int(w),
                                     int(cn), crop_border, subsample, convention, C.byref(out)))
        return _haarpsi_dict(out)

    def haarpsi_cells(self, d_a, stride_a, d_b, stride_b, h, w, cn, x_edges, y_edges, crop_border=0, subsample=True,
                      convention=HAARPSI_MATLAB) -> dict:
        """sr_haarpsi_cells_u8: HaarPSI's sums per cell of the separable grid x_edges x y_edges (pixels of the CROPPED
        rectangle) -> (gh, gw) float64 arrays 'num' and 'den', summed over the channels (a cell without a sample has den 0).
        Every argument is checked before the device is touched (ValueError)."""
        crop_border, subsample, convention = _haarpsi_switches(crop_border, subsample, convention)
        if not d_a or not d_b:
            raise ValueError("haarpsi_cells: null image pointer")
        xe, gw = _edge_array(x_edges, "x_edges")
        ye, gh = _edge_array(y_edges, "y_edges")
        recs = (HaarPsiCell * (gh * gw))()
        check(self.lib.sr_haarpsi_cells_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h),
                                           int(w), int(cn), crop_border, subsample, convention, xe, gw, ye, gh, recs))
        arr = np.frombuffer(recs, dtype=np.dtype([("num", "<f8"), ("den", "<f8")])).reshape(gh, gw)
        return {k: np.ascontiguousarray(arr[k]) for k in ("num", "den")}

    def niqe_u8(self, d_img, stride, h, w, cn, crop_border=0) -> np.ndarray:
        """sr_niqe_u8 -> records[2, nby * nbx] (NIQE_RECORD, scale-major) of the image cropped by crop_border (finish with
        niqe_features and niqe_score).  Every argument is checked before the device is touched: ValueError, or its subclass
        SrShapeError for a short stride or a side below 96 after the crop."""
        if not d_img:
            raise ValueError("niqe_u8: null image pointer")
        nby, nbx = niqe_plan(h, w, cn, crop_border)["blocks"]
        rec = np.zeros((2, nby * nbx), dtype=NIQE_RECORD)
        check(self.lib.sr_niqe_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w), int(cn), int(crop_border),
                                  rec.ctypes.data_as(C.c_void_p)))
        return rec

    def niqe_half_plane(self, shape) -> np.ndarray:
        """sr_niqe_half_plane: 65536 x the scale-2 plane (int32, exact) that the last niqe_u8 call of this context left in its
        scratch; shape = (H / 2, W / 2) of that call's niqe_plan size."""
        out = np.zeros(shape, dtype=np.int32)
        check(self.lib.sr_niqe_half_plane(self.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def brisque_u8(self, d_img, stride, h, w, cn, crop_border=0) -> np.ndarray:
        """sr_brisque_u8 -> records[2] (BRISQUE_RECORD, scale 1 then scale 2) of the image cropped by crop_border (finish with
        brisque_features and brisque_score).  Every argument is checked before the device is touched: ValueError, or its
        subclass SrShapeError for a short stride or a side below 16 after the crop."""
        if not d_img:
            raise ValueError("brisque_u8: null image pointer")
        brisque_plan(h, w, cn, crop_border)
        rec = np.zeros(2, dtype=BRISQUE_RECORD)
        check(self.lib.sr_brisque_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w), int(cn), int(crop_border),
                                     rec.ctypes.data_as(C.c_void_p)))
        return rec

    def brisque_half_plane(self, shape) -> np.ndarray:
        """sr_brisque_half_plane: 65536 x the scale-2 plane (int32, exact) that the last brisque_u8 call of this context left
        in its scratch; shape = that call's brisque_plan half_size."""
        out = np.zeros(shape, dtype=np.int32)
        check(self.lib.sr_brisque_half_plane(self.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def ms_ssim_planes(self, level: int, shape) -> Tuple[np.ndarray, np.ndarray]:
        """sr_ms_ssim_planes: the exact integer sums (uint16, 4^level gray values each) of level `level` that the last
        ms_ssim_u8 call of this context left in its scratch; shape = that level's (h_j, w_j) from ms_ssim_plan."""
        x, y = np.zeros(shape, dtype=np.uint16), np.zeros(shape, dtype=np.uint16)
        check(self.lib.sr_ms_ssim_planes(self.handle, int(level), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)))
        return x, y

    def assess_resized_u8(self, d_a, stride_a, d_b, stride_b, h, w, cn, dst_h, dst_w, flags=ASSESS_SSE | ASSESS_UNIFORM7,
                          gray_shift=15, data_range=255.0) -> dict:
        """The assess_u8 sums taken on the INTER_CUBIC resize of both images to dst_h x dst_w (sampled on the fly)."""
        out = AssessSums()
        check(self.lib.sr_assess_resized_u8(self.handle, C.c_void_p(d_a), stride_a, C.c_void_p(d_b), stride_b, h, w, cn,
                                            dst_h, dst_w, gray_shift, data_range, flags, C.byref(out)))
        return {"sse": out.sse, "ssim_uniform": out.ssim_uniform, "ssim_gauss": out.ssim_gauss,
                "ssim_simple": out.ssim_simple}

    def gray_moments_u8(self, d_tiles, n, tile_bytes, stride, h, w, gray_shift=15, swap_rb=True) -> np.ndarray:
        """sr_gray_moments_u8 -> (n, 2) uint64: the exact sums of gray and gray^2 of n RGB u8 tiles in HBM (tile i at
        d_tiles + i * tile_bytes, row stride in bytes)."""
        sums = np.zeros(2 * max(n, 1), dtype=np.uint64)
        check(self.lib.sr_gray_moments_u8(self.handle, C.c_void_p(d_tiles), int(n), int(tile_bytes), int(stride), int(h),
                                          int(w), int(gray_shift), 1 if swap_rb else 0,
                                          sums.ctypes.data_as(C.POINTER(C.c_uint64))))
        return sums[:2 * n].reshape(n, 2)

    def gray_std_u8(self, d_tiles, n, tile_bytes, stride, h, w, gray_shift=15, swap_rb=True) -> np.ndarray:
        """np.std of the u8 gray image of n RGB tiles in HBM (from exact integer moments, float64)."""
        sums = self.gray_moments_u8(d_tiles, n, tile_bytes, stride, h, w, gray_shift, swap_rb).reshape(-1)
        cnt = float(h) * float(w)
        s1, s2 = sums[0:2 * n:2].astype(np.float64), sums[1:2 * n:2].astype(np.float64)
        m = s1 / cnt
        return np.sqrt(np.maximum(s2 / cnt - m * m, 0.0))

    def histogram_u8(self, d_img, stride, h, w, cn) -> np.ndarray:
        """-> (cn, 256) int64 counts, np.histogram(channel, 256, [0, 256]) of u8 data."""
        out = np.zeros((cn, 256), dtype=np.uint64)
        check(self.lib.sr_histogram_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w), int(cn),
                                       out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out.astype(np.int64)

    def color_correct_u8(self, d_img, stride, h, w, cn, glut: np.ndarray, local_filter: int, radius: int, eps: float,
                         d_out, out_stride):
        g = np.ascontiguousarray(glut, dtype=np.float32).reshape(cn, 256)
        check(self.lib.sr_color_correct_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w), int(cn),
                                           g.ctypes.data_as(C.POINTER(C.c_float)), int(local_filter), int(radius),
                                           C.c_float(eps), C.c_void_p(d_out), int(out_stride)))

    def rgb2gray_u8(self, d_rgb, stride, h, w, d_gray, gray_stride, gray_shift=15):
        check(self.lib.sr_rgb2gray_u8(self.handle, C.c_void_p(d_rgb), stride, h, w, gray_shift, C.c_void_p(d_gray),
                                      gray_stride))

    def imresize(self, d_src, src_stride, h, w, cn, scale_y, scale_x, d_dst, dst_stride, dh, dw, antialias=True,
                 out_type=IMRESIZE_U8):
        """sr_imresize_u8: MATLAB's bicubic imresize of a u8 image in HBM into d_dst (uint8, float32 or float64 by out_type;
        strides in bytes).  Synchronous.  Every argument is checked before the device is touched: ValueError, its subclass
        SrShapeError for a short stride, SrNativeError (SR_ERR_UNSUPPORTED) for a scale outside [1/16, 16]."""
        if not d_src or not d_dst:
            raise ValueError("imresize: null image pointer")
        imresize_plan(h, w, cn, scale_y, scale_x, dh, dw, antialias)
        check(self.lib.sr_imresize_u8(self.handle, C.c_void_p(d_src), int(src_stride), int(h), int(w), int(cn), float(scale_y),
                                      float(scale_x), 1 if antialias else 0, _whole(out_type, "out_type"), C.c_void_p(d_dst),
                                      int(dst_stride), int(dh), int(dw)))

    def resize_cubic_u8(self, d_src, src_stride, h, w, cn, d_dst, dst_stride, dh, dw):
        check(self.lib.sr_resize_cubic_u8(self.handle, C.c_void_p(d_src), src_stride, h, w, cn, C.c_void_p(d_dst),
                                          dst_stride, dh, dw))

    def resize_cubic_window_u8(self, d_src, src_stride, h, w, cn, dh, dw, x0, y0, ww, wh, d_dst, dst_stride):
        check(self.lib.sr_resize_cubic_window_u8(self.handle, C.c_void_p(d_src), src_stride, h, w, cn, dh, dw, x0, y0,
                                                 ww, wh, C.c_void_p(d_dst), dst_stride))

    def gradient_fusion(self, dtype: int, d_tiles: Sequence[int], strides: Sequence[int], rects_xywh, cn: int, h: int, w: int,
                        d_canvas: int, canvas_stride: int, d_work: int):
        """sr_gradient_fusion: tiles in HBM (SR_U8 / SR_F32), canvas rectangles (x, y, w, h) -> u8 canvas; d_work holds
        h * w * cn floats.  Asynchronous."""
        n = len(rects_xywh)
        rects = (TileRect * n)(*[TileRect(int(x), int(y), int(tw), int(th)) for (x, y, tw, th) in rects_xywh])
        ptrs = (C.c_void_p * n)(*[C.c_void_p(p) for p in d_tiles])
        st = (C.c_int64 * n)(*[int(v) for v in strides])
        check(self.lib.sr_gradient_fusion(self.handle, int(dtype), ptrs, st, rects, n, int(cn), int(h), int(w),
                                          C.c_void_p(d_canvas), int(canvas_stride), C.c_void_p(d_work)))

    def gradient_stats_u8(self, d_img: int, stride: int, h: int, w: int, cn: int) -> Tuple[int, float]:
        """-> (exact sum of gx^2 + gy^2, fp64 sum of sqrt(gx^2 + gy^2)) of the u8 image's float32 Sobel."""
        sq, mag = C.c_uint64(0), C.c_double(0.0)
        check(self.lib.sr_gradient_stats_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w), int(cn),
                                            C.byref(sq), C.byref(mag)))
        return sq.value, mag.value

    def commercial_u8(self, d_img: int, stride: int, h: int, w: int, cn: int, flags: int, rois=(), roi_flags=(),
                      gray_shift: int = 15) -> Tuple[np.ndarray, np.ndarray]:
        """sr_commercial_u8 -> (ints (1 + n, 40) int64, flts (1 + n, 8) float64); row 0 is the whole image, row 1 + i the
        ROI rois[i] = (x, y, w, h) with the metrics of roi_flags[i] (see include/sr_hip.h for the slots)."""
        n = len(rois)
        ints = np.zeros((1 + n, 40), dtype=np.int64)
        flts = np.zeros((1 + n, 8), dtype=np.float64)
        rects = (TileRect * max(n, 1))(*[TileRect(int(x), int(y), int(rw), int(rh)) for (x, y, rw, rh) in rois])
        rf = (C.c_int * max(n, 1))(*[int(f) for f in roi_flags])
        check(self.lib.sr_commercial_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w), int(cn), int(gray_shift),
                                        int(flags), rects, rf, n, ints.ctypes.data_as(C.POINTER(C.c_int64)),
                                        flts.ctypes.data_as(C.POINTER(C.c_double))))
        return ints, flts

    def fft_c2c(self, d_in: int, d_out: int, lines: int, n: int):
        """sr_fft_c2c: forward DFT of `lines` rows of n complex64 values in HBM (synchronous)."""
        check(self.lib.sr_fft_c2c(self.handle, C.c_void_p(d_in), C.c_void_p(d_out), int(lines), int(n)))

    # content analysis (sr_content.hip) ------------------------------------------------------
    def saliency_u8(self, d_img: int, stride: int, h: int, w: int, cn: int, d_sal: int):
        """sr_saliency_u8: u8 image in HBM -> u8 spectral-residual saliency map (h * w bytes at d_sal).  Asynchronous."""
        check(self.lib.sr_saliency_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w), int(cn), C.c_void_p(d_sal)))

    def local_entropy_u8(self, d_img: int, stride: int, h: int, w: int, cn: int, window: int, d_out: int):
        """sr_local_entropy_u8: per-cell entropy of the gray image -> h * w float32 at d_out.  Asynchronous."""
        check(self.lib.sr_local_entropy_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w), int(cn), int(window),
                                           C.c_void_p(d_out)))

    def forbidden_map(self, d_sal: Optional[int], h: int, w: int, threshold: int, rects_xywh, d_map: int):
        """sr_forbidden_map: d_map = (saliency > threshold) | filled rectangles (x, y, w, h), clipped.  d_sal None: rectangles
        only.  Asynchronous."""
        n = len(rects_xywh)
        rects = (TileRect * max(n, 1))(*[TileRect(int(x), int(y), int(rw), int(rh)) for (x, y, rw, rh) in rects_xywh])
        check(self.lib.sr_forbidden_map(self.handle, C.c_void_p(d_sal), int(h), int(w), int(threshold), rects, n,
                                        C.c_void_p(d_map)))

    def rect_counts_u8(self, d_map: int, stride: int, h: int, w: int, rects_xywh) -> List[int]:
        """sr_rect_counts_u8 -> the exact count of non-zero bytes of the plane inside each rectangle (x, y, w, h)."""
        n = len(rects_xywh)
        out = (C.c_uint64 * max(n, 1))()
        rects = (TileRect * max(n, 1))(*[TileRect(int(x), int(y), int(rw), int(rh)) for (x, y, rw, rh) in rects_xywh])
        check(self.lib.sr_rect_counts_u8(self.handle, C.c_void_p(d_map), int(stride), int(h), int(w), rects, n, out))
        return [int(out[i]) for i in range(n)]

    # MSER text regions (sr_mser.hip) ----------------------------------------------------------
    def mser(self, d_img: int, stride: int, h: int, w: int, cn: int, params: Optional["MserParams"] = None,
             polarity_mask: int = MSER_BOTH) -> np.ndarray:
        """sr_mser_u8: the MSER regions of the u8 image in HBM as a structured array (MSER_REGION_DTYPE) in output order
        (polarity, level, seed).  Every refusal is raised before the device is touched (mser_plan).  The detection runs ONCE
        whatever the count: records beyond the first MSER_FIRST_CAP are fetched from the copy the context keeps
        (sr_mser_last_regions), without device work.  Synchronous."""
        params = params if params is not None else mser_params()
        mask = _mser_polarity_mask(polarity_mask)
        if not d_img:
            raise ValueError("mser: null image pointer")
        mser_plan(h, w, params)
        return _mser_fetch(lambda buf, cap, n: self.lib.sr_mser_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w),
                                                                   int(cn), C.byref(params), mask, buf, cap, n),
                           MSER_REGION_DTYPE, MSER_FIRST_CAP,
                           again=lambda buf, cap, n: self.lib.sr_mser_last_regions(self.handle, buf, cap, n))

    def mser_workspace(self) -> Tuple[int, int]:
        """sr_mser_workspace -> (device address, bytes) of the context's MSER workspace; (0, 0) before the first call."""
        p, n = _vp(None), _sz(0)
        check(self.lib.sr_mser_workspace(self.handle, C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)

    def mser_tree(self, d_img: int, stride: int, h: int, w: int, cn: int, polarity: int = 0) -> np.ndarray:
        """sr_mser_tree_u8: the whole node table of one polarity (0 dark, 1 bright) in (level, seed) order (MSER_NODE_DTYPE).
        Synchronous."""
        if polarity not in (0, 1):
            raise ValueError(f"mser_tree: polarity must be 0 or 1, got {polarity!r}")
        if not d_img:
            raise ValueError("mser_tree: null image pointer")
        plan = mser_plan(h, w)
        # a node per pixel up to 2^20 nodes in one run; a larger table takes a second run with the reported count
        return _mser_fetch(lambda buf, cap, n: self.lib.sr_mser_tree_u8(self.handle, C.c_void_p(d_img), int(stride), int(h), int(w),
                                                                        int(cn), int(polarity), buf, cap, n),
                           MSER_NODE_DTYPE, min(plan["node_cap"], 1 << 20))

    # Cascade detection (sr_cascade.hip) ---------------------------------------------------------
    def cascade(self, model: "CascadeModel", d_img: int, stride: int, h: int, w: int, cn: int,
                params: Optional["CascadeParams"] = None) -> np.ndarray:
        """sr_cascade_u8: the raw candidates of the u8 image in HBM, int32 [n, 4] (x, y, w, h) in canonical order (scale, y,
        x).  Every refusal is raised before the device is touched (CascadeModel.plan).  The detection runs ONCE whatever the
        count: candidates beyond the first CASCADE_FIRST_CAP come from the copy the context keeps
        (sr_cascade_last_candidates).  Synchronous."""
        params = params if params is not None else cascade_params()
        if not d_img:
            raise ValueError("cascade: null image pointer")
        model.plan(h, w, params)
        return _cascade_rects(_mser_fetch(
            lambda buf, cap, n: self.lib.sr_cascade_u8(self.handle, model.handle, C.c_void_p(d_img), int(stride), int(h), int(w),
                                                       int(cn), C.byref(params), buf, cap, n),
            CASCADE_RECT_DTYPE, CASCADE_FIRST_CAP,
            again=lambda buf, cap, n: self.lib.sr_cascade_last_candidates(self.handle, buf, cap, n)))

    def cascade_plane(self, model: "CascadeModel", d_img: int, stride: int, h: int, w: int, cn: int, k: int,
                      params: Optional["CascadeParams"] = None) -> np.ndarray:
        """sr_cascade_plane_u8: the scaled plane of scale k of the plan as the kernels made it (inspection)."""
        params = params if params is not None else cascade_params()
        scales = model.plan(h, w, params)["scales"]
        if not d_img or not 0 <= int(k) < len(scales):
            raise ValueError(f"cascade_plane: null image pointer or scale {k} of {len(scales)}")
        out = np.zeros((scales[k]["sh"], scales[k]["sw"]), np.uint8)
        _check_unsupported(self.lib.sr_cascade_plane_u8(self.handle, model.handle, C.c_void_p(d_img), int(stride), int(h), int(w),
                                                        int(cn), C.byref(params), int(k), C.c_void_p(out.ctypes.data)))
        return out

    def cascade_stage_map(self, model: "CascadeModel", d_img: int, stride: int, h: int, w: int, cn: int,
                          step: int = 1) -> np.ndarray:
        """sr_cascade_stage_map_u8: int32 [ny, nx], the number of stages each window of the gray plane itself passes
        (inspection; every stage on every window, no compaction)."""
        ny, nx = model.map_shape(h, w, step)
        if not d_img:
            raise ValueError("cascade_stage_map: null image pointer")
        out = np.zeros(max(ny * nx, 1), np.int32)
        n = _i64(0)
        _check_unsupported(self.lib.sr_cascade_stage_map_u8(self.handle, model.handle, C.c_void_p(d_img), int(stride), int(h),
                                                            int(w), int(cn), int(step), C.c_void_p(out.ctypes.data), ny * nx,
                                                            C.byref(n)))
        assert n.value == ny * nx
        return out[:ny * nx].reshape(ny, nx)

    def cascade_workspace(self) -> Tuple[int, int]:
        """sr_cascade_workspace -> (device address, bytes) of the context's cascade workspace; (0, 0) before the first call."""
        p, n = C.c_void_p(), _sz(0)
        check(self.lib.sr_cascade_workspace(self.handle, C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)

    # Poisson fusion and seam repair (sr_poisson.hip) ------------------------------------------
    def poisson_clone_u8(self, d_dest: int, dest_stride: int, d_patch: int, patch_stride: int, d_mask: int, mask_stride: int,
                         h: int, w: int, mode: int, d_out: int, out_stride: int):
        """sr_poisson_clone_u8: the seamlessClone solve on one h x w x 3 rectangle (mode 1 normal, 2 mixed, 3 monochrome).
        A side above POISSON_MAX_SIDE is refused before the device is touched.  Asynchronous."""
        if max(int(h), int(w)) > POISSON_MAX_SIDE:
            raise NotImplementedError(f"poisson clone: a side of {max(h, w)} pixels is above the FFT engine's {POISSON_MAX_SIDE}")
        rc = self.lib.sr_poisson_clone_u8(self.handle, C.c_void_p(d_dest), int(dest_stride), C.c_void_p(d_patch),
                                          int(patch_stride), C.c_void_p(d_mask), int(mask_stride), int(h), int(w), int(mode),
                                          C.c_void_p(d_out), int(out_stride))
        if rc == SR_ERR_UNSUPPORTED:
            raise NotImplementedError(last_error())
        check(rc)

    def gaussian_blur15_u8(self, d_src: int, src_stride: int, h: int, w: int, cn: int, d_dst: int, dst_stride: int):
        """sr_gaussian_blur15_u8: cv2.GaussianBlur(roi, (15, 15), 0) on u8; d_dst may be d_src.  Asynchronous."""
        check(self.lib.sr_gaussian_blur15_u8(self.handle, C.c_void_p(d_src), int(src_stride), int(h), int(w), int(cn),
                                             C.c_void_p(d_dst), int(dst_stride)))

    def region_ssim_u8(self, d_a: int, stride_a: int, d_b: int, stride_b: int, h: int, w: int, cn: int,
                       gray_shift: int = 15) -> float:
        """sr_region_ssim_u8: _compute_ssim of two u8 rectangles in HBM (synchronous)."""
        out = C.c_double(0.0)
        check(self.lib.sr_region_ssim_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h),
                                         int(w), int(cn), int(gray_shift), C.byref(out)))
        return out.value

    def resize_linear_u8(self, d_src: int, src_stride: int, h: int, w: int, cn: int, d_dst: int, dst_stride: int, dh: int,
                         dw: int):
        """sr_resize_linear_u8: cv2.resize(INTER_LINEAR) on u8.  Asynchronous."""
        check(self.lib.sr_resize_linear_u8(self.handle, C.c_void_p(d_src), int(src_stride), int(h), int(w), int(cn),
                                           C.c_void_p(d_dst), int(dst_stride), int(dh), int(dw)))

    def tile_ssim_sums_u8(self, d_canvas: int, canvas_stride: int, h: int, w: int, cn: int, rects_xywh,
                          d_tiles: Sequence[int], strides: Sequence[int], gray_shift: int = 15) -> np.ndarray:
        """-> (n, 5) exact sums of a, b, a^2, b^2, a b (a: gray canvas ROI, b: gray tile, resized to a clipped ROI)."""
        n = len(rects_xywh)
        out = np.zeros((max(n, 1), 5), dtype=np.uint64)
        rects = (TileRect * max(n, 1))(*[TileRect(int(x), int(y), int(tw), int(th)) for (x, y, tw, th) in rects_xywh])
        ptrs = (C.c_void_p * max(n, 1))(*[C.c_void_p(p) for p in d_tiles])
        st = (C.c_int64 * max(n, 1))(*[int(v) for v in strides])
        check(self.lib.sr_tile_ssim_sums_u8(self.handle, C.c_void_p(d_canvas), int(canvas_stride), int(h), int(w), int(cn),
                                            rects, ptrs, st, n, int(gray_shift),
                                            out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out[:n]

    # numpy-in / numpy-out conveniences (stage through HBM) ----------------------------------
    def pyr_down_np(self, img: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(img, dtype=np.float32)
        h, w = a.shape[:2]
        cn = a.shape[2] if a.ndim == 3 else 1
        out_shape = ((h + 1) // 2, (w + 1) // 2) + a.shape[2:]
        src = self.upload(a)
        dst = self.alloc(int(np.prod(out_shape)) * 4)
        check(self.lib.sr_pyr_down(self.handle, C.c_void_p(src.ptr), h, w, cn, C.c_void_p(dst.ptr)))
        res = self.download(dst.ptr, out_shape, np.float32)
        src.free(); dst.free()
        return res

    def pyr_up_np(self, img: np.ndarray, dst_hw, a: Optional[np.ndarray] = None, mode: str = "up") -> np.ndarray:
        """mode 'up': pyrUp(img); 'sub': a - pyrUp(img); 'add': pyrUp(img) + a."""
        s = np.ascontiguousarray(img, dtype=np.float32)
        hs, ws = s.shape[:2]
        cn = s.shape[2] if s.ndim == 3 else 1
        hd, wd = int(dst_hw[0]), int(dst_hw[1])
        out_shape = (hd, wd) + s.shape[2:]
        src = self.upload(s)
        dst = self.alloc(int(np.prod(out_shape)) * 4)
        if mode == "up":
            check(self.lib.sr_pyr_up(self.handle, C.c_void_p(src.ptr), hs, ws, cn, C.c_void_p(dst.ptr), hd, wd))
        else:
            if (hs, ws) != ((hd + 1) // 2, (wd + 1) // 2):
                raise SrShapeError(f"pyrUp: source {hs}x{ws} does not match destination {hd}x{wd}")
            aa = self.upload(np.ascontiguousarray(a, dtype=np.float32))
            fn = self.lib.sr_pyr_up_sub if mode == "sub" else self.lib.sr_pyr_up_add
            check(fn(self.handle, C.c_void_p(aa.ptr), hd, wd, cn, C.c_void_p(src.ptr), C.c_void_p(dst.ptr)))
            aa.free()
        res = self.download(dst.ptr, out_shape, np.float32)
        src.free(); dst.free()
        return res

    def fusion_np(self, tiles: Sequence[np.ndarray], positions_yx, output_shape, levels: int, weight_type: str,
                  laplacian: bool = True, return_float: bool = False):
        """tiles: list of HWC (or HW) arrays, all u8 or all float; positions (y, x)."""
        n = len(tiles)
        is_u8 = all(t.dtype == np.uint8 for t in tiles)
        arrs = [np.ascontiguousarray(t if is_u8 else t.astype(np.float32)) for t in tiles]
        cn = arrs[0].shape[2] if arrs[0].ndim == 3 else 1
        if any(a.ndim != arrs[0].ndim or a.shape[2:] != arrs[0].shape[2:] for a in arrs):
            raise ValueError("fusion: every tile must have the same number of channels")   # the C side copies h*w*cn per tile
        H, W = int(output_shape[0]), int(output_shape[1])
        rects = (TileRect * n)(*[TileRect(int(p[1]), int(p[0]), a.shape[1], a.shape[0])
                                 for a, p in zip(arrs, positions_yx)])
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        out = np.empty((H, W) if cn == 1 else (H, W, cn), dtype=np.uint8)
        outf = np.empty(out.shape, dtype=np.float32) if return_float else None
        fptr = outf.ctypes.data_as(C.c_void_p) if outf is not None else None
        dt = SR_U8 if is_u8 else SR_F32
        self.h2d_bytes += sum(a.nbytes for a in arrs)        # the *_host entry points stage tiles and canvas themselves
        self.d2h_bytes += out.nbytes + (outf.nbytes if outf is not None else 0)
        if laplacian:
            check(self.lib.sr_laplacian_fusion_host(self.handle, dt, ptrs, rects, n, cn, H, W, int(levels),
                                                    WEIGHT_TYPES[weight_type], out.ctypes.data_as(C.c_void_p), fptr))
        else:
            check(self.lib.sr_weighted_fusion_host(self.handle, dt, ptrs, rects, n, cn, H, W,
                                                   WEIGHT_TYPES[weight_type], out.ctypes.data_as(C.c_void_p), fptr))
        return (out, outf) if return_float else out


def _feather_merge_np(self, arrays, descs, output_width: int, output_height: int, blending: bool = True) -> np.ndarray:
    """TilingModule.merge_tiles on the GPU: arrays are HxWx3 tiles, ALL uint8 or ALL float32; descs dicts with the
    sr_merge_tile fields."""
    n = len(arrays)
    is_f32 = n > 0 and arrays[0].dtype == np.float32
    if any(a.dtype != (np.float32 if is_f32 else np.uint8) for a in arrays):
        raise ValueError("feather_merge_np: tiles must be all uint8 or all float32")
    es = 4 if is_f32 else 1
    bufs = [self.upload(a) for a in arrays]
    canvas = self.alloc(output_width * output_height * 3)
    try:
        self.feather_merge(SR_F32 if is_f32 else SR_U8, descs, [b.ptr for b in bufs], [a.shape[1] * 3 * es for a in arrays],
                           blending, canvas.ptr, output_width * 3, output_height, output_width)
        return self.download(canvas.ptr, (output_height, output_width, 3), np.uint8)
    finally:
        self.sync()
        for b in bufs:
            b.free()
        canvas.free()


def _feather_merge(self, dtype: int, descs, d_tiles: Sequence[int], strides: Sequence[int], blending: bool, d_canvas: int,
                   canvas_stride: int, canvas_h: int, canvas_w: int):
    """sr_feather_merge_dt on device pointers: tiles (SR_U8 / SR_F32, row strides in bytes) -> u8 canvas view.  descs are
    dicts with the sr_merge_tile fields.  Asynchronous."""
    n = len(descs)
    mt = (MergeTile * max(n, 1))(*[MergeTile(*[int(d[k]) for k in ("x", "y", "src_w", "src_h", "out_w", "out_h",
                                                                     "ov_t", "ov_b", "ov_l", "ov_r")]) for d in descs])
    ptrs = (C.c_void_p * max(n, 1))(*[C.c_void_p(p) for p in d_tiles])
    st = (C.c_int64 * max(n, 1))(*[int(s) for s in strides])
    check(self.lib.sr_feather_merge_dt(self.handle, int(dtype), mt, n, ptrs, st, 1 if blending else 0, C.c_void_p(d_canvas),
                                       int(canvas_stride), int(canvas_h), int(canvas_w)))


Context.feather_merge = _feather_merge
Context.feather_merge_np = _feather_merge_np


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """sr_comm_unique_id: the 128-byte rendezvous token rank 0 creates and ships to every rank."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _preload_rccl()
    check(load().sr_comm_unique_id(buf))
    return buf.raw


def _xfer_args(rects_xywh, world, need, owners, owned_ptrs, owned_strides, recv_ptrs):
    n, rects = _rects(rects_xywh)
    flat = (C.c_int * (2 * world * n))(*[v for r in range(world) for t in range(n) for v in need[r][t]])
    own = (C.c_int * n)(*[int(o) for o in owners])
    dp = (_vp * n)(*[int(p) if p else None for p in owned_ptrs])
    st = (_i64 * n)(*[int(v) for v in owned_strides])
    rp = (_vp * n)(*[int(p) if p else None for p in recv_ptrs])
    return n, rects, flat, own, dp, st, rp


def exchange_xfers(rects_xywh, cn: int, world: int, rank: int, need, owners, owned_ptrs, owned_strides, recv_ptrs):
    """Host-only (sr_exchange_xfers): ([(peer, pointer, bytes)] sends, receives) of one rank's grouped exchange."""
    n, rects, flat, own, dp, st, rp = _xfer_args(rects_xywh, world, need, owners, owned_ptrs, owned_strides, recv_ptrs)
    sends, recvs = (Xfer * (n * world))(), (Xfer * n)()
    ns, nr = C.c_int(0), C.c_int(0)
    check(load().sr_exchange_xfers(rects, n, int(cn), int(world), int(rank), flat, own, dp, st, rp, sends, n * world, C.byref(ns),
                                   recvs, n, C.byref(nr)))
    return ([(sends[i].peer, sends[i].d_ptr or 0, sends[i].bytes) for i in range(ns.value)],
            [(recvs[i].peer, recvs[i].d_ptr or 0, recvs[i].bytes) for i in range(nr.value)])


def sharded_tile_bases(rects_xywh, cn: int, world: int, rank: int, need, owners, owned_ptrs, strides, recv_ptrs) -> List[int]:
    """Host-only (sr_sharded_tile_bases): the per-tile base pointers rank `rank` hands to its strip blend (0 for tiles its
    strip does not read); validates owners, rows, dense strides of received tiles and receive buffers."""
    n, rects, flat, own, dp, st, rp = _xfer_args(rects_xywh, world, need, owners, owned_ptrs, strides, recv_ptrs)
    base = (_vp * n)()
    check(load().sr_sharded_tile_bases(rects, n, int(cn), int(world), int(rank), flat, own, dp, st, rp, base))
    return [int(b or 0) for b in base]


class Comm:
    """RCCL communicator of the C ABI (sr_comm_*): one process per GPU, transfers on the context's stream."""

    def __init__(self, ctx: "Context", unique_id: bytes, world: int, rank: int):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        self.ctx, self.world, self.rank = ctx, int(world), int(rank)
        h = _vp()
        _preload_rccl()
        check(load().sr_comm_init(ctx.handle, C.create_string_buffer(unique_id, COMM_ID_BYTES), self.world, self.rank, C.byref(h)))
        self.h = h

    def exchange(self, sends, recvs):
        """sends / recvs: [(peer, device pointer, bytes)] -- one grouped batch, asynchronous on the context's stream."""
        s = (Xfer * max(len(sends), 1))(*[Xfer(int(p), int(d), int(b)) for (p, d, b) in sends])
        r = (Xfer * max(len(recvs), 1))(*[Xfer(int(p), int(d), int(b)) for (p, d, b) in recvs])
        check(load().sr_comm_exchange(self.ctx.handle, self.h, s, len(sends), r, len(recvs)))

    def exchange_tile_rows(self, rects_xywh, cn: int, need, owners, owned_ptrs, owned_strides, recv_ptrs):
        """sr_comm_exchange_tile_rows: need[r][t] = (r0, r1) and owners from exchange_plan(); owned_ptrs[t] / recv_ptrs[t]
        are device pointers or 0."""
        n, rects, flat, own, dp, st, rp = _xfer_args(rects_xywh, self.world, need, owners, owned_ptrs, owned_strides, recv_ptrs)
        check(load().sr_comm_exchange_tile_rows(self.ctx.handle, self.h, rects, n, int(cn), flat, own, dp, st, rp))

    def blend_sharded(self, plan: "BlendPlan", rects_xywh, cn: int, need, owners, owned_ptrs, strides, recv_ptrs, d_canvas: int,
                      canvas_stride: int, ctx: Optional["Context"] = None):
        """sr_laplacian_blend_sharded: the row exchange and this rank's strip blend on one stream (plan made on the same
        context, for the same tiles)."""
        n, rects, flat, own, dp, st, rp = _xfer_args(rects_xywh, self.world, need, owners, owned_ptrs, strides, recv_ptrs)
        check(load().sr_laplacian_blend_sharded((ctx or self.ctx).handle, self.h, plan.handle, rects, n, int(cn), flat, own, dp, st, rp,
                                                _vp(int(d_canvas)), int(canvas_stride)))

    def allreduce_f64(self, d_ptr: int, count: int):
        check(load().sr_comm_allreduce_f64(self.ctx.handle, self.h, _vp(int(d_ptr)), int(count)))

    def close(self):
        if getattr(self, "h", None):
            h, self.h = self.h, None
            check(load().sr_comm_destroy(h))


class BlendPlan:
    """sr_blend_plan: device workspace for one tile arrangement (optionally one canvas strip)."""

    def __init__(self, ctx: Context, rects_xywh: Sequence[Tuple[int, int, int, int]], cn: int, canvas_h: int,
                 canvas_w: int, levels: int = 6, weight_type: str = "cosine", row_begin: int = 0,
                 row_end: Optional[int] = None):
        self.ctx = ctx
        self.n = len(rects_xywh)
        self.cn = cn
        self.canvas_h, self.canvas_w = int(canvas_h), int(canvas_w)
        self.row_begin = int(row_begin)
        self.row_end = int(canvas_h if row_end is None else row_end)
        rects = (TileRect * self.n)(*[TileRect(int(x), int(y), int(w), int(h)) for (x, y, w, h) in rects_xywh])
        h = C.c_void_p()
        check(ctx.lib.sr_blend_plan_create(ctx.handle, rects, self.n, cn, self.canvas_h, self.canvas_w, int(levels),
                                           WEIGHT_TYPES[weight_type], self.row_begin, self.row_end, C.byref(h)))
        self.handle = h

    def tile_rows(self, t: int) -> Tuple[int, int]:
        a, b = C.c_int(0), C.c_int(0)
        check(self.ctx.lib.sr_blend_plan_tile_rows(self.handle, t, C.byref(a), C.byref(b)))
        return a.value, b.value

    def workspace_bytes(self) -> int:
        b = C.c_size_t(0)
        check(self.ctx.lib.sr_blend_plan_workspace_bytes(self.handle, C.byref(b)))
        return b.value

    def g1_format(self, dtype: int = SR_U8) -> int:
        """0: a blend of tiles of `dtype` keeps G_1 as fp32 planes, 1: as the exact 16-bit integers 256 * G_1."""
        f = C.c_int(-1)
        check(self.ctx.lib.sr_blend_plan_g1_format(self.handle, int(dtype), C.byref(f)))
        return f.value

    def march_items(self, nt: int) -> np.ndarray:
        """The plan's work lists of the marched gather (sr_blend_plan_march_items): nt = 1 .. 4 -> int32 [items, 8] of
        (x0, y0, ncell, nstep, tile[4]) in launch order; nt = 0 -> int32 [rectangles, 4] of (x, y, w, h)."""
        per = 4 if nt == 0 else 8
        cnt = _i64(0)
        check(self.ctx.lib.sr_blend_plan_march_items(self.handle, int(nt), None, 0, C.byref(cnt)))
        out = np.zeros((cnt.value, per), dtype=np.int32)
        if cnt.value:
            check(self.ctx.lib.sr_blend_plan_march_items(self.handle, int(nt), out.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         cnt.value, C.byref(cnt)))
        return out

    def blend(self, d_tiles: Sequence[int], strides: Sequence[int], d_canvas: int, canvas_stride: int,
              dtype: int = SR_U8, d_canvas_f32: Optional[int] = None, laplacian: bool = True):
        ptrs = (C.c_void_p * self.n)(*[C.c_void_p(p) for p in d_tiles])
        st = (C.c_int64 * self.n)(*[int(s) for s in strides])
        fn = self.ctx.lib.sr_laplacian_blend if laplacian else self.ctx.lib.sr_weighted_blend
        check(fn(self.handle, dtype, ptrs, st, C.c_void_p(d_canvas), int(canvas_stride),
                 C.c_void_p(d_canvas_f32) if d_canvas_f32 else None))

    def blend_custom_weights(self, d_tiles, strides, d_weights, weight_strides, d_canvas: int, canvas_stride: int,
                             dtype: int = SR_U8, d_canvas_f32: Optional[int] = None):
        ptrs, st = self._tile_args(d_tiles, strides)
        wp = (C.c_void_p * self.n)(*[C.c_void_p(p) for p in d_weights])
        ws = (C.c_int64 * self.n)(*[int(s) for s in weight_strides])
        check(self.ctx.lib.sr_weighted_blend_custom(self.handle, dtype, ptrs, st, wp, ws, C.c_void_p(d_canvas),
                                                    int(canvas_stride), C.c_void_p(d_canvas_f32) if d_canvas_f32 else None))

    def _tile_args(self, d_tiles, strides):
        return ((C.c_void_p * self.n)(*[C.c_void_p(p) for p in d_tiles]), (C.c_int64 * self.n)(*[int(s) for s in strides]))

    def pyramids(self, d_tiles: Sequence[int], strides: Sequence[int], tile_idx: Sequence[int], first: bool,
                 dtype: int = SR_U8):
        """Stage A for the listed tiles (first=True also builds the weight pyramids)."""
        ptrs, st = self._tile_args(d_tiles, strides)
        idx = (C.c_int * max(len(tile_idx), 1))(*[int(t) for t in tile_idx])
        check(self.ctx.lib.sr_blend_pyramids(self.handle, dtype, ptrs, st, idx, len(tile_idx), 1 if first else 0))

    def gather(self, d_tiles: Sequence[int], strides: Sequence[int], d_canvas: int, canvas_stride: int,
               dtype: int = SR_U8, d_canvas_f32: Optional[int] = None):
        """Stage B: canvas gather over all tiles."""
        ptrs, st = self._tile_args(d_tiles, strides)
        check(self.ctx.lib.sr_blend_gather(self.handle, dtype, ptrs, st, C.c_void_p(d_canvas), int(canvas_stride),
                                           C.c_void_p(d_canvas_f32) if d_canvas_f32 else None))

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.sr_blend_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


# ------------------------------------------------------------------------------------------
# LPIPS (sr_lpips_*): caller-supplied weights, state-dict names of lpips.LPIPS(net) (lpips >= 0.1.4)
# ------------------------------------------------------------------------------------------
LPIPS_NETS = {"alex": 0, "vgg": 1}
# convolutions of the backbones in forward order: "net.slice<S>.<index in torchvision's features>"
LPIPS_CONV_KEYS = {
    "alex": ["net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10"],
    "vgg": ["net.slice1.0", "net.slice1.2", "net.slice2.5", "net.slice2.7", "net.slice3.10", "net.slice3.12",
            "net.slice3.14", "net.slice4.17", "net.slice4.19", "net.slice4.21", "net.slice5.24", "net.slice5.26",
            "net.slice5.28"],
}
LPIPS_CONV_SHAPES = {
    "alex": [(64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3)],
    "vgg": [(64, 3, 3), (64, 64, 3), (128, 64, 3), (128, 128, 3), (256, 128, 3), (256, 256, 3), (256, 256, 3),
            (512, 256, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3)],
}
LPIPS_TAP_CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}


def load_lpips_weights(path: str) -> dict:
    """Reads a flat .npz of ``lpips.LPIPS(net).state_dict()`` arrays (numpy.load with allow_pickle=False: nothing in the
    file is executed).  Returns {name: ndarray}."""
    with np.load(path, allow_pickle=False) as z:
        return {k: np.asarray(z[k]) for k in z.files}


def lpips_pack_weights(net: str, weights: dict):
    """Validates a state-dict of arrays against the backbone's shapes -> (conv weights, conv biases, lin weights, shift,
    scale) as contiguous fp32 arrays in forward order.  Host only."""
    if net not in LPIPS_NETS:
        raise ValueError(f"LPIPS net must be 'alex' or 'vgg', got {net!r}")
    convs_w, convs_b = [], []
    for key, (co, ci, k) in zip(LPIPS_CONV_KEYS[net], LPIPS_CONV_SHAPES[net]):
        if key + ".weight" not in weights or key + ".bias" not in weights:
            raise ValueError(f"LPIPS weights for {net!r} lack {key}.weight / .bias")
        w = np.ascontiguousarray(weights[key + ".weight"], dtype=np.float32)
        b = np.ascontiguousarray(weights[key + ".bias"], dtype=np.float32)
        if w.shape != (co, ci, k, k) or b.shape != (co,):
            raise ValueError(f"LPIPS weight {key}: expected {(co, ci, k, k)} / {(co,)}, got {w.shape} / {b.shape}")
        convs_w.append(w)
        convs_b.append(b)
    lins = []
    for i, c in enumerate(LPIPS_TAP_CHANNELS[net]):
        name = next((n for n in (f"lin{i}.model.1.weight", f"lins.{i}.model.1.weight", f"lin{i}.model.0.weight")
                     if n in weights), None)
        if name is None:
            raise ValueError(f"LPIPS weights for {net!r} lack lin{i}.model.1.weight")
        lw = np.ascontiguousarray(np.asarray(weights[name], dtype=np.float32).reshape(-1))
        if lw.shape != (c,):
            raise ValueError(f"LPIPS weight {name}: expected {c} values, got {lw.shape}")
        lins.append(lw)
    shift = np.ascontiguousarray(weights.get("scaling_layer.shift", np.array([-.030, -.088, -.188])), dtype=np.float32).reshape(-1)
    scale = np.ascontiguousarray(weights.get("scaling_layer.scale", np.array([.458, .448, .450])), dtype=np.float32).reshape(-1)
    if shift.shape != (3,) or scale.shape != (3,):
        raise ValueError("LPIPS scaling_layer.shift / .scale must hold 3 values")
    return convs_w, convs_b, lins, shift, scale


def lpips_synthetic_weights(net: str, seed: int = 20260313) -> dict:
    """Seeded random weights of the real shapes (He-scaled convolutions, non-negative 1x1 `lin` layers) for timing and
    structural tests: the pretrained LPIPS weights cannot be fetched offline.  NOT a substitute for them."""
    rng = np.random.default_rng(seed)
    w = {}
    for key, (co, ci, k) in zip(LPIPS_CONV_KEYS[net], LPIPS_CONV_SHAPES[net]):
        w[key + ".weight"] = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32)
        w[key + ".bias"] = rng.uniform(0, 0.1, co).astype(np.float32)
    for i, c in enumerate(LPIPS_TAP_CHANNELS[net]):
        w[f"lin{i}.model.1.weight"] = rng.uniform(0, 2.0 / c, (1, c, 1, 1)).astype(np.float32)
    return w


LPIPS_PLAN_MAX_ACT, LPIPS_PLAN_FIELDS = 18, 12


def lpips_tile_plan(net: str, h: int, w: int, tile: int, tile_index: int) -> dict:
    """sr_lpips_tile_plan (host only, no GPU): what the forward works on for one tile.  Returns {"buffer_floats": int,
    "acts": [per activation {"need_y", "own_y", "need_x", "own_x": (a, b), "pitch", "C", "H", "W"}]}; activation 0 is the image.  net
    "dists": sr_dists_tile_plan, the same records for the DISTS stack (stage 0 is activation 0)."""
    n, floats = C.c_int(0), C.c_int64(0)
    rec = (C.c_int * (LPIPS_PLAN_MAX_ACT * LPIPS_PLAN_FIELDS))()
    if net == "dists":
        check(load().sr_dists_tile_plan(int(h), int(w), int(tile), int(tile_index), C.byref(n), rec, C.byref(floats)))
    else:
        check(load().sr_lpips_tile_plan(LPIPS_NETS[net], int(h), int(w), int(tile), int(tile_index), C.byref(n), rec, C.byref(floats)))
    acts = []
    for j in range(n.value):
        r = rec[j * LPIPS_PLAN_FIELDS:(j + 1) * LPIPS_PLAN_FIELDS]
        acts.append({"need_y": (r[0], r[1]), "own_y": (r[2], r[3]), "need_x": (r[4], r[5]), "own_x": (r[6], r[7]),
                     "pitch": r[8], "C": r[9], "H": r[10], "W": r[11]})
    return {"buffer_floats": floats.value, "acts": acts}


class LpipsModel:
    """sr_lpips_model: one backbone + lin layers resident on the GPU."""

    def __init__(self, ctx: Context, net: str, weights: dict):
        convs_w, convs_b, lins, shift, scale = lpips_pack_weights(net, weights)
        self.ctx, self.net = ctx, net
        n = len(convs_w)
        pw = (C.c_void_p * n)(*[a.ctypes.data for a in convs_w])
        pb = (C.c_void_p * n)(*[a.ctypes.data for a in convs_b])
        pl = (C.c_void_p * 5)(*[a.ctypes.data for a in lins])
        h = C.c_void_p()
        check(ctx.lib.sr_lpips_create(ctx.handle, LPIPS_NETS[net], pw, pb, n, pl, 5, shift.ctypes.data_as(C.c_void_p),
                                      scale.ctypes.data_as(C.c_void_p), C.byref(h)))
        self.handle = h

    def layer_sizes(self, h: int, w: int):
        out = (C.c_int * 10)()
        check(self.ctx.lib.sr_lpips_layer_sizes(LPIPS_NETS[self.net], int(h), int(w), out))
        return [(out[2 * i], out[2 * i + 1]) for i in range(5)]

    def tile_count(self, h: int, w: int, tile: int) -> int:
        n = C.c_int(0)
        check(self.ctx.lib.sr_lpips_tile_count(int(h), int(w), int(tile), C.byref(n)))
        return n.value

    def layer_sums(self, d_a: int, stride_a: int, d_b: int, stride_b: int, h: int, w: int, cn: int, tile: int = 4096,
                   tile_begin: int = 0, tile_end: int = -1):
        """Per-tap sums of the lin maps over tiles [tile_begin, tile_end) (additive across disjoint tile ranges)."""
        out = (C.c_double * 5)()
        check(self.ctx.lib.sr_lpips_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h),
                                       int(w), int(cn), int(tile), int(tile_begin), int(tile_end), out))
        return [out[i] for i in range(5)]

    def value(self, d_a: int, stride_a: int, d_b: int, stride_b: int, h: int, w: int, cn: int, tile: int = 4096,
              per_layer: bool = False):
        sums = self.layer_sums(d_a, stride_a, d_b, stride_b, h, w, cn, tile)
        vals = [s / (lh * lw) for s, (lh, lw) in zip(sums, self.layer_sizes(h, w))]
        return (float(sum(vals)), vals) if per_layer else float(sum(vals))

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.sr_lpips_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


# ------------------------------------------------------------------------------------------
# DISTS (sr_dists_*): caller-supplied weights, state-dict names of DISTS_pytorch.DISTS()
# ------------------------------------------------------------------------------------------
# the 13 convolutions in forward order: "stage<S>.<index in torchvision's VGG16 features>"; the published weights.pt holds
# only alpha and beta, so torchvision's own "features.<index>" is accepted for each
DISTS_CONV_KEYS = ["stage1.0", "stage1.2", "stage2.5", "stage2.7", "stage3.10", "stage3.12", "stage3.14", "stage4.17",
                   "stage4.19", "stage4.21", "stage5.24", "stage5.26", "stage5.28"]
DISTS_CONV_SHAPES = LPIPS_CONV_SHAPES["vgg"]
DISTS_CHANNELS = (3, 64, 128, 256, 512, 512)
DISTS_TOTAL = sum(DISTS_CHANNELS)        # 1475
_DISTS_HANN = np.outer([0.25, 0.5, 0.25], [0.25, 0.5, 0.25])


def load_dists_weights(path: str) -> dict:
    """Reads a flat .npz holding the VGG16 convolutions (``stageN.K.weight`` / ``.bias`` or ``features.K.*``) and ``alpha`` /
    ``beta`` (numpy.load with allow_pickle=False: nothing in the file is executed).  Returns {name: ndarray}."""
    with np.load(path, allow_pickle=False) as z:
        return {k: np.asarray(z[k]) for k in z.files}


def dists_pack_weights(weights: dict):
    """Validates a dict of arrays -> (conv weights, conv biases, alpha, beta, mean or None, std or None) as contiguous fp32
    arrays.  Every refusal is a ValueError that names the key.  Host only."""
    convs_w, convs_b = [], []
    for key, (co, ci, k) in zip(DISTS_CONV_KEYS, DISTS_CONV_SHAPES):
        alt = "features." + key.split(".")[1]
        arrs = []
        for suffix, shape in ((".weight", (co, ci, k, k)), (".bias", (co,))):
            name = next((n for n in (key + suffix, alt + suffix) if n in weights), None)
            if name is None:
                raise ValueError(f"DISTS weights lack {key}{suffix} (or {alt}{suffix})")
            a = np.ascontiguousarray(weights[name], dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"DISTS weight {name}: expected {shape}, got {a.shape}")
            arrs.append(a)
        convs_w.append(arrs[0])
        convs_b.append(arrs[1])
    ab = []
    for name in ("alpha", "beta"):
        if name not in weights:
            raise ValueError(f"DISTS weights lack {name}")
        v = np.ascontiguousarray(np.asarray(weights[name], dtype=np.float32).reshape(-1))
        if v.shape != (DISTS_TOTAL,):
            raise ValueError(f"DISTS weight {name}: expected {DISTS_TOTAL} values, got {np.asarray(weights[name]).shape}")
        if not np.all(np.isfinite(v)):
            raise ValueError(f"DISTS weight {name}: not finite")
        ab.append(v)
    if not float(ab[0].astype(np.float64).sum() + ab[1].astype(np.float64).sum()) > 0.0:
        raise ValueError("DISTS weights alpha / beta: the total must be positive")
    ms = []
    for name in ("mean", "std"):
        if name not in weights:
            ms.append(None)
            continue
        v = np.ascontiguousarray(np.asarray(weights[name], dtype=np.float32).reshape(-1))
        if v.shape != (3,) or not np.all(np.isfinite(v)) or (name == "std" and np.any(v == 0)):
            raise ValueError(f"DISTS weight {name}: expected 3 finite values (std non-zero), got {np.asarray(weights[name]).shape}")
        ms.append(v)
    for name, v in weights.items():
        if name.startswith("stage") and name.endswith(".filter"):     # L2pooling's buffer: fixed here, so it must be the Hann one
            f = np.asarray(v, dtype=np.float64)
            if f.ndim != 4 or f.shape[1:] != (1, 3, 3) or not np.allclose(f, _DISTS_HANN[None, None], rtol=0, atol=1e-7):
                raise ValueError(f"DISTS weight {name}: not the 3 x 3 Hann filter outer((1/4, 1/2, 1/4)) the L2 pooling here is fixed to")
    return convs_w, convs_b, ab[0], ab[1], ms[0], ms[1]


def dists_synthetic_weights(seed: int = 20260519) -> dict:
    """Seeded random weights of the real shapes (He-scaled convolutions, alpha, beta ~ U(0, 1)) for timing and structural
    tests.  NOT the published weights: those cannot be fetched offline."""
    rng = np.random.default_rng(seed)
    w = {}
    for key, (co, ci, k) in zip(DISTS_CONV_KEYS, DISTS_CONV_SHAPES):
        w[key + ".weight"] = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32)
        w[key + ".bias"] = rng.uniform(0, 0.1, co).astype(np.float32)
    w["alpha"] = rng.uniform(0, 1, (1, DISTS_TOTAL, 1, 1)).astype(np.float32)
    w["beta"] = rng.uniform(0, 1, (1, DISTS_TOTAL, 1, 1)).astype(np.float32)
    return w


def dists_layer_sizes(h: int, w: int):
    """Host only: the six (H, W) of DISTS's feature maps (stage 0 = the image, then ceil halving from stage 2 on)."""
    out = (C.c_int * 12)()
    check(load().sr_dists_layer_sizes(int(h), int(w), out))
    return [(out[2 * i], out[2 * i + 1]) for i in range(6)]


def dists_score(sums, hw, alpha, beta, per_channel: bool = False):
    """Host only: the DISTS value from 1475 x 5 float64 sums, the six sizes and alpha / beta (sr_dists_score)."""
    sums = _f64(sums, (DISTS_TOTAL, 5), "sums")
    hw_a = np.ascontiguousarray(np.asarray(hw, dtype=np.int32).reshape(-1))
    if hw_a.shape != (12,):
        raise ValueError("dists_score: hw must hold six (H, W)")
    al = np.ascontiguousarray(np.asarray(alpha, dtype=np.float32).reshape(-1))
    be = np.ascontiguousarray(np.asarray(beta, dtype=np.float32).reshape(-1))
    if al.shape != (DISTS_TOTAL,) or be.shape != (DISTS_TOTAL,):
        raise ValueError(f"dists_score: alpha and beta must hold {DISTS_TOTAL} values")
    score = C.c_double(0.0)
    s1, s2 = np.empty(DISTS_TOTAL, np.float64), np.empty(DISTS_TOTAL, np.float64)
    check(load().sr_dists_score(sums.ctypes.data, hw_a.ctypes.data, al.ctypes.data, be.ctypes.data, C.byref(score),
                                s1.ctypes.data if per_channel else None, s2.ctypes.data if per_channel else None))
    return (score.value, s1, s2) if per_channel else score.value


class DistsModel:
    """sr_dists_model: the VGG16 convolutions resident on the GPU, alpha / beta on the host."""

    def __init__(self, ctx: Context, weights: dict):
        convs_w, convs_b, self.alpha, self.beta, mean, std = dists_pack_weights(weights)
        self.ctx = ctx
        pw = (C.c_void_p * 13)(*[a.ctypes.data for a in convs_w])
        pb = (C.c_void_p * 13)(*[a.ctypes.data for a in convs_b])
        h = C.c_void_p()
        check(ctx.lib.sr_dists_create(ctx.handle, pw, pb, mean.ctypes.data if mean is not None else None,
                                      std.ctypes.data if std is not None else None, C.byref(h)))
        self.handle = h

    def layer_sizes(self, h: int, w: int):
        return dists_layer_sizes(h, w)

    def tile_count(self, h: int, w: int, tile: int) -> int:
        n = C.c_int(0)
        check(self.ctx.lib.sr_dists_tile_count(int(h), int(w), int(tile), C.byref(n)))
        return n.value

    def sums(self, d_a: int, stride_a: int, d_b: int, stride_b: int, h: int, w: int, cn: int, tile: int = 4096,
             tile_begin: int = 0, tile_end: int = -1) -> np.ndarray:
        """The 1475 x 5 float64 sums (a, b, a^2, b^2, a b per channel, stage 0 first) over tiles [tile_begin, tile_end):
        additive across disjoint tile ranges."""
        out = np.zeros((DISTS_TOTAL, 5), np.float64)
        check(self.ctx.lib.sr_dists_u8(self.handle, C.c_void_p(d_a), int(stride_a), C.c_void_p(d_b), int(stride_b), int(h),
                                       int(w), int(cn), int(tile), int(tile_begin), int(tile_end), out.ctypes.data))
        return out

    def value(self, d_a: int, stride_a: int, d_b: int, stride_b: int, h: int, w: int, cn: int, tile: int = 4096,
              per_channel: bool = False):
        """DISTS of the pair; with per_channel also S1 and S2 (1475 each)."""
        sums = self.sums(d_a, stride_a, d_b, stride_b, h, w, cn, tile)
        return dists_score(sums, self.layer_sizes(h, w), self.alpha, self.beta, per_channel)

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.sr_dists_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def dists_l2pool(ctx, x: np.ndarray) -> np.ndarray:
    """The L2 pooling kernel on a dense [C][H][W] fp32 array (inspection: sr_dists_l2pool_f32)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 3:
        raise ValueError("dists_l2pool: a [C][H][W] array")
    c, h, w = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    d_in, d_out = ctx.upload(x), ctx.alloc(c * ho * wo * 4)
    try:
        check(ctx.lib.sr_dists_l2pool_f32(ctx.handle, C.c_void_p(d_in.ptr), c, h, w, C.c_void_p(d_out.ptr)))
        return ctx.download(d_out.ptr, (c, ho, wo), np.float32)
    finally:
        d_in.free(); d_out.free()


# ------------------------------------------------------------------------------------------
# local SR network (sr_srnet_*): caller-supplied weights; sr_network.CompactSRNet parses state dicts into these arrays
# ------------------------------------------------------------------------------------------
def _check_unsupported(rc: int) -> None:
    """SR_ERR_UNSUPPORTED -> NotImplementedError, everything else as check()."""
    if rc == SR_ERR_UNSUPPORTED:
        raise NotImplementedError(last_error())
    check(rc)


def srnet_plan(h: int, w: int, n_feat: int, n_body: int, scale: int, tile: int = 0) -> Tuple[int, int, int]:
    """sr_srnet_plan (host only) -> (halo, sub-tiles, workspace bytes)."""
    halo, n, ws = C.c_int(0), C.c_int(0), C.c_size_t(0)
    _check_unsupported(load().sr_srnet_plan(int(h), int(w), int(n_feat), int(n_body), int(scale), int(tile), C.byref(halo),
                                            C.byref(n), C.byref(ws)))
    return halo.value, n.value, int(ws.value)


def ens_plan(h: int, w: int, scale: int, mask: int) -> Tuple[int, int]:
    """sr_ens_plan (host only) -> (members, workspace bytes) of a self-ensemble of an h x w input at ``scale`` over ``mask``."""
    n, ws = C.c_int(0), C.c_size_t(0)
    check(load().sr_ens_plan(_whole(h, "h"), _whole(w, "w"), _whole(scale, "scale"), _whole(mask, "mask"), C.byref(n), C.byref(ws)))
    return n.value, int(ws.value)


def _ctx_handle(ctx):
    return ctx.handle if ctx is not None else None


def d4_u8(ctx, d_src: int, src_stride: int, h: int, w: int, k: int, d_dst: int, dst_stride: int) -> None:
    """sr_d4_u8: d_dst = T_k(d_src), h x w x 3 u8 (w x h x 3 out for k & 4).  Arguments are refused before the context is
    looked at, so ``ctx`` may be None where only the refusal matters.  Asynchronous."""
    check(load().sr_d4_u8(_ctx_handle(ctx), C.c_void_p(d_src), int(src_stride), int(h), int(w), _whole(k, "k"), C.c_void_p(d_dst),
                          int(dst_stride)))


def d4_acc_f32(ctx, d_y: int, y_stride: int, H: int, W: int, k: int, first: bool, d_acc: int, acc_stride: int) -> None:
    """sr_d4_acc_f32: d_acc (H x W x 3 fp32) = T_k^-1(d_y) if ``first`` else d_acc + T_k^-1(d_y).  Asynchronous."""
    check(load().sr_d4_acc_f32(_ctx_handle(ctx), C.c_void_p(d_y), int(y_stride), int(H), int(W), _whole(k, "k"), int(bool(first)),
                               C.c_void_p(d_acc), int(acc_stride)))


def ens_finish(ctx, d_acc: int, acc_stride: int, H: int, W: int, n: int, d_dst: int, dst_stride: int, u8: bool) -> None:
    """sr_ens_finish_u8 / sr_ens_finish_f32: d_dst = d_acc / n, as u8 by the forwards' rule or as fp32.  Asynchronous."""
    fn = load().sr_ens_finish_u8 if u8 else load().sr_ens_finish_f32
    check(fn(_ctx_handle(ctx), C.c_void_p(d_acc), int(acc_stride), int(H), int(W), _whole(n, "n"), C.c_void_p(d_dst), int(dst_stride)))


class _SrModel:
    """What SrNetModel, ResNetModel, RrdbModel, RcanModel, SwinirModel and HatModel share: the caller's tables as checked fp32 arrays, the create call, the two
    forwards, close.  ``_kind`` names the sr_<kind>_* entry points, ``_run_args`` what their forwards take after the
    destination stride."""
    _kind = ""
    _run_args = ("tile",)

    @staticmethod
    def _conv_arrays(weights, biases, shapes, what: str):
        """-> (weights, biases) as contiguous fp32, checked against ``shapes`` = (cout, cin) per convolution."""
        ws = [np.ascontiguousarray(a, dtype=np.float32) for a in weights]
        bs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in biases]
        for k, (w, b, (co, ci)) in enumerate(zip(ws, bs, shapes)):
            if w.shape != (co, ci, 3, 3) or b.shape != (co,):
                raise ValueError(f"{what} {k}: expected {(co, ci, 3, 3)} / {(co,)}, got {w.shape} / {b.shape}")
        return ws, bs

    def _create(self, ctx: Context, args, *tables, count: bool = False):
        """sr_<kind>_create(ctx, *args, one pointer table per entry of ``tables``[, their length], &handle)."""
        ptrs = [(C.c_void_p * len(t))(*[a.ctypes.data for a in t]) for t in tables]
        h = C.c_void_p()
        create = getattr(ctx.lib, f"sr_{self._kind}_create")
        _check_unsupported(create(ctx.handle, *args, *ptrs, *([len(tables[0])] if count else []), C.byref(h)))
        self.ctx, self.handle = ctx, h

    def _run(self, entry: str, d_src: int, src_stride: int, h: int, w: int, d_dst: int, dst_stride: int, args, named, last=()):
        names = self._run_args
        if len(args) > len(names) or not set(named) <= set(names[len(args):]):
            raise TypeError(f"sr_{self._kind}_{entry} takes {', '.join(names)} after the strides, got {args} {named}")
        ints = [int(v) for v in args] + [int(named.get(n, 0)) for n in names[len(args):]] + [int(v) for v in last]
        check(getattr(self.ctx.lib, f"sr_{self._kind}_{entry}")(self.handle, C.c_void_p(d_src), int(src_stride), int(h), int(w),
                                                                C.c_void_p(d_dst), int(dst_stride), *ints))

    def upscale_u8(self, d_src: int, src_stride: int, h: int, w: int, d_dst: int, dst_stride: int, *args, **named):
        """sr_<kind>_u8: h x w x 3 u8 -> (h s) x (w s) x 3 u8, HBM -> HBM; then ``tile = 0`` (RrdbModel: and ``tail = 0``; RcanModel:
        and SwinirModel: ``tail = 0`` alone), by position or by name.  Asynchronous."""
        self._run("u8", d_src, src_stride, h, w, d_dst, dst_stride, args, named)

    def forward_f32(self, d_src: int, src_stride: int, h: int, w: int, d_dst: int, dst_stride: int, *args, **named):
        """sr_<kind>_f32: the unclamped fp32 output (HWC, stride in bytes); arguments as upscale_u8.  Asynchronous."""
        self._run("f32", d_src, src_stride, h, w, d_dst, dst_stride, args, named)

    def ensemble_u8(self, d_src: int, src_stride: int, h: int, w: int, d_dst: int, dst_stride: int, *args, mask: int, **named):
        """sr_<kind>_ens_u8: the geometric self-ensemble over the members of ``mask`` (bit k: the transform T_k of
        include/sr_hip.h; 1 .. 255), u8 out; the other arguments as upscale_u8.  Asynchronous."""
        self._run("ens_u8", d_src, src_stride, h, w, d_dst, dst_stride, args, named, last=(_whole(mask, "mask"),))

    def ensemble_f32(self, d_src: int, src_stride: int, h: int, w: int, d_dst: int, dst_stride: int, *args, mask: int, **named):
        """sr_<kind>_ens_f32: the ensemble's unclamped fp32 output; arguments as ensemble_u8.  Asynchronous."""
        self._run("ens_f32", d_src, src_stride, h, w, d_dst, dst_stride, args, named, last=(_whole(mask, "mask"),))

    def close(self):
        if getattr(self, "handle", None):
            getattr(self.ctx.lib, f"sr_{self._kind}_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class SrNetModel(_SrModel):
    """sr_srnet_model: the compact SR network resident on the GPU.  weights / biases: D + 2 arrays in layer order (OIHW fp32),
    slopes: D + 1 arrays of F values."""
    _kind = "srnet"

    def __init__(self, ctx: Context, n_feat: int, n_body: int, scale: int, weights, biases, slopes):
        n_feat, n_body, scale = int(n_feat), int(n_body), int(scale)
        srnet_plan(1, 1, n_feat, n_body, scale)                  # the supported range, refused before any array is touched
        if len(weights) != n_body + 2 or len(biases) != n_body + 2 or len(slopes) != n_body + 1:
            raise ValueError(f"SR network with {n_body} body convolutions needs {n_body + 2} weight / bias arrays and {n_body + 1} slope vectors")
        ss = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in slopes]
        shapes = [(n_feat, 3)] + [(n_feat, n_feat)] * n_body + [(3 * scale * scale, n_feat)]
        ws, bs = self._conv_arrays(weights, biases, shapes, "SR network layer")
        if any(s.shape != (n_feat,) for s in ss):
            raise ValueError(f"SR network slopes must hold {n_feat} values each")
        self.n_feat, self.n_body, self.scale = n_feat, n_body, scale
        self._create(ctx, (n_feat, n_body, scale), ws, bs, ss)

    def plan(self, h: int, w: int, tile: int = 0) -> Tuple[int, int, int]:
        return srnet_plan(h, w, self.n_feat, self.n_body, self.scale, tile)


# ------------------------------------------------------------------------------------------
# local SR network, residual family (sr_resnet_*): sr_network.ResidualSRNet parses BasicSR state dicts into these arrays
# ------------------------------------------------------------------------------------------
def resnet_desc(n_feat: int, n_blocks: int, scale: int, long_skip: bool = False, conv_hr: bool = False, bilinear_base: bool = False,
                a_head: float = 1.0, a_up: float = 1.0, a_hr: float = 1.0, res_scale: float = 1.0, mean=(0.0, 0.0, 0.0),
                range: float = 1.0) -> ResNetDesc:  # noqa: A002 (the header's name)
    mean = [float(v) for v in np.asarray(mean, dtype=np.float64).reshape(-1)]
    if len(mean) != 3:
        raise ValueError(f"mean holds 3 values, got {len(mean)}")
    return ResNetDesc(int(n_feat), int(n_blocks), int(scale), int(bool(long_skip)), int(bool(conv_hr)), int(bool(bilinear_base)),
                      float(a_head), float(a_up), float(a_hr), float(res_scale), (C.c_float * 3)(*mean), float(range))


def resnet_conv_shapes(desc: ResNetDesc) -> List[Tuple[int, int]]:
    """(cout, cin) of every convolution in sr_resnet_create's order."""
    F, s = desc.n_feat, desc.scale
    ups = {1: [], 2: [2], 3: [3], 4: [2, 2]}.get(s, [])
    return ([(F, 3)] + [(F, F)] * (2 * desc.n_blocks + (1 if desc.long_skip else 0)) + [(F * r * r, F) for r in ups]
            + ([(F, F)] if desc.conv_hr else []) + [(3, F)])


def resnet_plan(desc: ResNetDesc, h: int, w: int, tile: int = 0) -> Tuple[int, int, int]:
    """sr_resnet_plan (host only) -> (halo, sub-tiles, workspace bytes)."""
    halo, n, ws = C.c_int(0), C.c_int(0), C.c_size_t(0)
    _check_unsupported(load().sr_resnet_plan(C.byref(desc), int(h), int(w), int(tile), C.byref(halo), C.byref(n), C.byref(ws)))
    return halo.value, n.value, int(ws.value)


class ResNetModel(_SrModel):
    """sr_resnet_model: a residual SR network (MSRResNet / EDSR) resident on the GPU.  weights / biases: one OIHW fp32 array
    and one bias vector per convolution in forward order (resnet_conv_shapes)."""
    _kind = "resnet"

    def __init__(self, ctx: Context, desc: ResNetDesc, weights, biases):
        resnet_plan(desc, 1, 1)                                  # the supported range, refused before any array is touched
        shapes = resnet_conv_shapes(desc)
        if len(weights) != len(shapes) or len(biases) != len(shapes):
            raise ValueError(f"this residual SR network has {len(shapes)} convolutions, got {len(weights)} weight / {len(biases)} bias arrays")
        ws, bs = self._conv_arrays(weights, biases, shapes, "residual SR network convolution")
        self.desc, self.scale = desc, desc.scale
        self._create(ctx, (C.byref(desc),), ws, bs, count=True)

    def plan(self, h: int, w: int, tile: int = 0) -> Tuple[int, int, int]:
        return resnet_plan(self.desc, h, w, tile)


# ------------------------------------------------------------------------------------------
# local SR network, RRDBNet (sr_rrdb_*): sr_network.RRDBSRNet parses BasicSR state dicts into these arrays
# ------------------------------------------------------------------------------------------
def rrdb_desc(n_feat: int, n_grow: int, n_blocks: int, scale: int = 4, slope: float = 0.2, res_scale: float = 0.2) -> RrdbDesc:
    return RrdbDesc(int(n_feat), int(n_grow), int(n_blocks), int(scale), float(slope), float(res_scale))


def rrdb_conv_shapes(desc: RrdbDesc) -> List[Tuple[int, int]]:
    """(cout, cin) of every convolution in sr_rrdb_create's order."""
    F, G = desc.n_feat, desc.n_grow
    dense = [(G, F + k * G) for k in range(4)] + [(F, F + 4 * G)]
    return [(F, 3)] + dense * (3 * desc.n_blocks) + [(F, F)] * 4 + [(3, F)]


def rrdb_plan(desc: RrdbDesc, h: int, w: int, tile: int = 0, tail: int = 0) -> Tuple[int, int, int, int]:
    """sr_rrdb_plan (host only) -> (halo, trunk pieces, tail sub-pieces, workspace bytes)."""
    halo, n, nt, ws = C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    _check_unsupported(load().sr_rrdb_plan(C.byref(desc), int(h), int(w), int(tile), int(tail), C.byref(halo), C.byref(n), C.byref(nt),
                                           C.byref(ws)))
    return halo.value, n.value, nt.value, int(ws.value)


class RrdbModel(_SrModel):
    """sr_rrdb_model: an RRDBNet (ESRGAN / Real-ESRGAN x4) resident on the GPU.  weights / biases: one OIHW fp32 array and one
    bias vector per convolution in forward order (rrdb_conv_shapes)."""
    _kind = "rrdb"
    _run_args = ("tile", "tail")

    def __init__(self, ctx: Context, desc: RrdbDesc, weights, biases):
        rrdb_plan(desc, 1, 1)                                    # the supported range, refused before any array is touched
        shapes = rrdb_conv_shapes(desc)
        if len(weights) != len(shapes) or len(biases) != len(shapes):
            raise ValueError(f"this RRDB network has {len(shapes)} convolutions, got {len(weights)} weight / {len(biases)} bias arrays")
        ws, bs = self._conv_arrays(weights, biases, shapes, "RRDB network convolution")
        self.desc, self.scale = desc, desc.scale
        self._create(ctx, (C.byref(desc),), ws, bs, count=True)

    def plan(self, h: int, w: int, tile: int = 0, tail: int = 0) -> Tuple[int, int, int, int]:
        return rrdb_plan(self.desc, h, w, tile, tail)


# ------------------------------------------------------------------------------------------
# local SR network, RCAN (sr_rcan_*): sr_network.RCANSRNet parses BasicSR state dicts into these arrays
# ------------------------------------------------------------------------------------------
def rcan_desc(n_feat: int, n_squeeze: int, n_groups: int, n_blocks: int, scale: int, res_scale: float = 1.0, mean=(0.0, 0.0, 0.0),
              range: float = 1.0) -> RcanDesc:  # noqa: A002 (the header's name)
    mean = [float(v) for v in np.asarray(mean, dtype=np.float64).reshape(-1)]
    if len(mean) != 3:
        raise ValueError(f"mean holds 3 values, got {len(mean)}")
    return RcanDesc(int(n_feat), int(n_squeeze), int(n_groups), int(n_blocks), int(scale), float(res_scale), (C.c_float * 3)(*mean),
                    float(range))


def rcan_conv_shapes(desc: RcanDesc) -> List[Tuple[int, int, int]]:
    """(cout, cin, kernel side) of every table in sr_rcan_create's order: 3 for a 3 x 3 convolution, 1 for one of the two 1 x 1
    layers of an RCAB's attention."""
    F, R, s = desc.n_feat, desc.n_squeeze, desc.scale
    ups = {1: [], 2: [2], 3: [3], 4: [2, 2]}.get(s, [])
    group = [(F, F, 3), (F, F, 3), (R, F, 1), (F, R, 1)] * desc.n_blocks + [(F, F, 3)]
    return [(F, 3, 3)] + group * desc.n_groups + [(F, F, 3)] + [(F * r * r, F, 3) for r in ups] + [(3, F, 3)]


def rcan_plan(desc: RcanDesc, h: int, w: int, tail: int = 0) -> Tuple[int, int, int]:
    """sr_rcan_plan (host only) -> (the tail's halo, tail sub-pieces, workspace bytes)."""
    halo, nt, ws = C.c_int(0), C.c_int(0), C.c_size_t(0)
    _check_unsupported(load().sr_rcan_plan(C.byref(desc), int(h), int(w), int(tail), C.byref(halo), C.byref(nt), C.byref(ws)))
    return halo.value, nt.value, int(ws.value)


class RcanModel(_SrModel):
    """sr_rcan_model: an RCAN resident on the GPU.  weights / biases: one fp32 array and one bias vector per table in forward
    order (rcan_conv_shapes): OIHW for the 3 x 3 convolutions, (out, in) or (out, in, 1, 1) for the 1 x 1 layers.  The trunk is
    one piece (the channel mean is global), so the forwards take ``tail`` alone."""
    _kind = "rcan"
    _run_args = ("tail",)

    def __init__(self, ctx: Context, desc: RcanDesc, weights, biases):
        rcan_plan(desc, 1, 1)                                    # the supported range, refused before any array is touched
        shapes = rcan_conv_shapes(desc)
        if len(weights) != len(shapes) or len(biases) != len(shapes):
            raise ValueError(f"this RCAN has {len(shapes)} tables, got {len(weights)} weight / {len(biases)} bias arrays")
        ws = [np.ascontiguousarray(a, dtype=np.float32) for a in weights]
        bs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in biases]
        for k, (w, b, (co, ci, ks)) in enumerate(zip(ws, bs, shapes)):
            ok = w.shape == (co, ci, ks, ks) or (ks == 1 and w.shape == (co, ci))
            if not ok or b.shape != (co,):
                raise ValueError(f"RCAN table {k}: expected {(co, ci, ks, ks)} / {(co,)}, got {w.shape} / {b.shape}")
        self.desc, self.scale = desc, desc.scale
        self._create(ctx, (C.byref(desc),), ws, bs, count=True)

    def plan(self, h: int, w: int, tail: int = 0) -> Tuple[int, int, int]:
        return rcan_plan(self.desc, h, w, tail)


def rcan_attention(ctx, d_x: int, plane_stride: int, row_stride: int, n_feat: int, n_squeeze: int, h: int, w: int, w1, b1, w2, b2):
    """sr_rcan_attention_f32: the channel mean and the attention of one RCAB on a planar fp32 tensor on the device (element
    (c, y, x) at d_x + c plane_stride + y row_stride + 4 x bytes) -> (mean[F], s[F]) as fp32 arrays.  Arguments are refused
    before the context is looked at, so ``ctx`` may be None where only the refusal matters.  Synchronous."""
    F, R = int(n_feat), int(n_squeeze)
    tabs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (w1, b1, w2, b2)]
    for a, n, name in zip(tabs, (R * F, R, F * R, F), ("w1", "b1", "w2", "b2")):
        if 1 <= R <= F <= 256 and a.size != n:                   # outside that range the library refuses by name
            raise ValueError(f"{name} holds {a.size} values, expected {n}")
    mean, s = np.empty(max(F, 1), np.float32), np.empty(max(F, 1), np.float32)
    _check_unsupported(load().sr_rcan_attention_f32(_ctx_handle(ctx), C.c_void_p(d_x), int(plane_stride), int(row_stride), F, R, int(h), int(w),
                                                    *[a.ctypes.data_as(C.c_void_p) for a in tabs], mean.ctypes.data_as(C.c_void_p),
                                                    s.ctypes.data_as(C.c_void_p)))
    return mean, s


# ------------------------------------------------------------------------------------------
# What the two window-attention families (SwinIR, HAT) share on this side: the names and shapes of an attention block, an
# MLP and the pixelshuffle reconstruction, the plan and index calls, the model base and the inspection call.
# ------------------------------------------------------------------------------------------
def _sw_conv(co, ci):
    return ((co, ci, 3, 3), (co,))


def _sw_block_names(b: str, attn: str = "attn."):
    """-> (the names of block b's attention tables, of its MLP's); attn: '' where the attention is the block itself (HAT's OCAB)."""
    return ([f"{b}.norm1", f"{b}.{attn}qkv", f"{b}.{attn}relative_position_bias_table", f"{b}.{attn}proj"],
            [f"{b}.norm2", f"{b}.mlp.fc1", f"{b}.mlp.fc2"])


def _sw_block_shapes(Cn: int, nh: int, hid: int, rows: int):
    """-> (the shapes of an attention's tables, its bias table of ``rows`` rows, and of an MLP's)."""
    ln = ((Cn,), (Cn,))
    return [ln, ((3 * Cn, Cn), (3 * Cn,)), ((rows, nh), None), ((Cn, Cn), (Cn,))], [ln, ((hid, Cn), (hid,)), ((Cn, hid), (Cn,))]


def _sw_shuffle_tail(Cn: int, s: int):
    """-> (names, shapes) of the pixelshuffle reconstruction at scale s."""
    rs = [2, 2] if s == 4 else [s]
    return (["conv_before_upsample.0"] + [f"upsample.{2 * k}" for k in range(len(rs))] + ["conv_last"],
            [_sw_conv(64, Cn)] + [_sw_conv(64 * r * r, 64) for r in rs] + [_sw_conv(3, 64)])


def _sw_plan(entry: str, desc, h: int, w: int, tail: int) -> Tuple[int, int, int, int, int]:
    hp, wp, halo, nt, ws = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    _check_unsupported(getattr(load(), entry)(C.byref(desc), int(h), int(w), int(tail), C.byref(hp), C.byref(wp), C.byref(halo), C.byref(nt),
                                              C.byref(ws)))
    return hp.value, wp.value, halo.value, nt.value, int(ws.value)


def _sw_index(entry: str, shape) -> np.ndarray:
    idx = np.empty(shape, np.int32)
    check(getattr(load(), entry)(idx.ctypes.data_as(C.c_void_p), idx.size))
    return idx


class _SwModel(_SrModel):
    """What SwinirModel and HatModel share: the checked tables, plan, fill_workspace.  ``_name``: what a ValueError calls the
    family; ``_shapes`` / ``_plan``: its *_table_shapes / *_plan; ``_conv1x1``: whether an (out, in) table may come as
    (out, in, 1, 1).  The trunk is one piece, so the forwards take ``tail`` alone."""
    _run_args = ("tail",)
    _name = ""
    _conv1x1 = False
    _shapes = _plan = None

    def _tables(self, desc, weights, biases):
        """-> (weights, biases) as contiguous fp32, checked against the family's shapes."""
        self._plan(desc, 1, 1)                                   # the supported range, refused before any array is touched
        shapes = self._shapes(desc)
        if len(weights) != len(shapes) or len(biases) != len(shapes):
            raise ValueError(f"this {self._name} has {len(shapes)} tables, got {len(weights)} weight / {len(biases)} bias arrays")
        ws = [np.ascontiguousarray(a, dtype=np.float32) for a in weights]
        bs = [np.zeros(1, np.float32) if sb is None else np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a, (_, sb) in zip(biases, shapes)]
        for k, (w, b, (sw, sb)) in enumerate(zip(ws, bs, shapes)):
            ok = w.shape == sw or (self._conv1x1 and len(sw) == 2 and w.shape == sw + (1, 1))
            if not ok or (sb is not None and b.shape != sb):
                raise ValueError(f"{self._name} table {k}: expected {sw} / {sb}, got {w.shape} / {b.shape}")
        self.desc, self.scale = desc, desc.scale
        return ws, bs

    def plan(self, h: int, w: int, tail: int = 0):
        return self._plan(self.desc, h, w, tail)

    def fill_workspace(self, h: int, w: int, byte: int, tail: int = 0):
        """sr_<kind>_fill_workspace: the buffers of an h x w forward, grown and filled with ``byte`` (for tests)."""
        check(getattr(self.ctx.lib, f"sr_{self._kind}_fill_workspace")(self.handle, int(h), int(w), int(tail), int(byte)))


def _sw_bias_table(table, rows: int, n_heads: int) -> np.ndarray:
    t = np.ascontiguousarray(table, dtype=np.float32)
    if 1 <= int(n_heads) <= 256 and t.shape != (rows, int(n_heads)):
        raise ValueError(f"the bias table is {(rows, int(n_heads))}, got {t.shape}")
    return t


def _sw_attention(entry: str, ctx, d_qkv: int, plane_stride: int, row_stride: int, n_feat: int, n_heads: int, hp: int, wp: int, args,
                  d_out: int, out_plane_stride: int, out_row_stride: int):
    """sr_<entry>(ctx, the qkv view, C, heads, hp, wp, *args, the output view); ``args``: what the entry takes between them."""
    _check_unsupported(getattr(load(), entry)(_ctx_handle(ctx), C.c_void_p(d_qkv), int(plane_stride), int(row_stride), int(n_feat),
                                              int(n_heads), int(hp), int(wp), *args, C.c_void_p(d_out), int(out_plane_stride),
                                              int(out_row_stride)))


# ------------------------------------------------------------------------------------------
# local SR network, SwinIR (sr_swinir_*): sr_network.SwinIRSRNet parses BasicSR state dicts into these arrays
# ------------------------------------------------------------------------------------------
SWINIR_UPSAMPLERS = {"pixelshuffle": 0, "pixelshuffledirect": 1, "nearest+conv": 2}
SWINIR_WINDOW = 8


def swinir_desc(n_feat: int, n_heads: int, n_hidden: int, n_groups: int, depth: int, scale: int, upsampler="pixelshuffle",
                mean=(0.0, 0.0, 0.0), range: float = 1.0) -> SwinirDesc:  # noqa: A002 (the header's name)
    mean = [float(v) for v in np.asarray(mean, dtype=np.float64).reshape(-1)]
    if len(mean) != 3:
        raise ValueError(f"mean holds 3 values, got {len(mean)}")
    kind = SWINIR_UPSAMPLERS.get(upsampler, upsampler)
    return SwinirDesc(int(n_feat), int(n_heads), int(n_hidden), int(n_groups), int(depth), int(scale), int(kind), (C.c_float * 3)(*mean),
                      float(range))


def swinir_table_names(desc: SwinirDesc) -> List[str]:
    """BasicSR's name of every table in sr_swinir_create's order (weight key = name + '.weight', bias key = name + '.bias';
    the bias table's key is the name itself and it has no bias)."""
    names = ["conv_first", "patch_embed.norm"]
    for i in range(desc.n_groups):
        for j in range(desc.depth):
            b = f"layers.{i}.residual_group.blocks.{j}"
            names += sum(_sw_block_names(b), [])
        names.append(f"layers.{i}.conv")
    names += ["norm", "conv_after_body"]
    if desc.upsampler == 0:
        names += _sw_shuffle_tail(desc.n_feat, desc.scale)[0]
    elif desc.upsampler == 1:
        names += ["upsample.0"]
    else:
        names += ["conv_before_upsample.0", "conv_up1", "conv_up2", "conv_hr", "conv_last"]
    return names


def swinir_table_shapes(desc: SwinirDesc) -> List[Tuple[tuple, Optional[tuple]]]:
    """(weight shape, bias shape) of every table in sr_swinir_create's order; the bias table has no bias (None)."""
    Cn, s, conv, ln = desc.n_feat, desc.scale, _sw_conv, ((desc.n_feat,), (desc.n_feat,))
    layer = sum(_sw_block_shapes(Cn, desc.n_heads, desc.n_hidden, (2 * SWINIR_WINDOW - 1) ** 2), [])
    shapes = [conv(Cn, 3), ln] + (layer * desc.depth + [conv(Cn, Cn)]) * desc.n_groups + [ln, conv(Cn, Cn)]
    if desc.upsampler == 0:
        shapes += _sw_shuffle_tail(Cn, s)[1]
    elif desc.upsampler == 1:
        shapes += [conv(3 * s * s, Cn)]
    else:
        shapes += [conv(64, Cn), conv(64, 64), conv(64, 64), conv(64, 64), conv(3, 64)]
    return shapes


def swinir_plan(desc: SwinirDesc, h: int, w: int, tail: int = 0) -> Tuple[int, int, int, int, int]:
    """sr_swinir_plan (host only) -> (padded rows, padded columns, the tail's halo, tail sub-pieces, workspace bytes)."""
    return _sw_plan("sr_swinir_plan", desc, h, w, tail)


def swinir_rel_index() -> np.ndarray:
    """sr_swinir_rel_index (host only) -> (64, 64) int32: the bias-table row of (query token, key token)."""
    return _sw_index("sr_swinir_rel_index", (64, 64))


class SwinirModel(_SwModel):
    """sr_swinir_model: a SwinIR resident on the GPU.  weights / biases: one fp32 array each per table in forward order
    (swinir_table_shapes / swinir_table_names); the bias entry of a relative-position table is ignored (None is fine).  The
    trunk is one piece, so the forwards take ``tail`` alone."""
    _kind, _name = "swinir", "SwinIR"
    _shapes, _plan = staticmethod(swinir_table_shapes), staticmethod(swinir_plan)

    def __init__(self, ctx: Context, desc: SwinirDesc, weights, biases):
        ws, bs = self._tables(desc, weights, biases)
        self._create(ctx, (C.byref(desc),), ws, bs, count=True)


def swinir_layernorm(ctx, d_x: int, plane_stride: int, row_stride: int, n_feat: int, h: int, w: int, gamma, beta, d_out: int,
                     out_plane_stride: int, out_row_stride: int):
    """sr_swinir_layernorm_f32: the backend's LayerNorm over the channels of a planar fp32 tensor on the device (element
    (c, y, x) at d_x + c plane_stride + y row_stride + 4 x bytes) into d_out, laid out likewise.  Synchronous."""
    g, b = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (gamma, beta))
    if 1 <= int(n_feat) <= 256 and (g.size != n_feat or b.size != n_feat):
        raise ValueError(f"gamma / beta hold {g.size} / {b.size} values, expected {n_feat}")
    _check_unsupported(load().sr_swinir_layernorm_f32(_ctx_handle(ctx), C.c_void_p(d_x), int(plane_stride), int(row_stride), int(n_feat), int(h),
                                                      int(w), g.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.c_void_p(d_out),
                                                      int(out_plane_stride), int(out_row_stride)))


def swinir_attention(ctx, d_qkv: int, plane_stride: int, row_stride: int, n_feat: int, n_heads: int, hp: int, wp: int, shift: int, table,
                     d_out: int, out_plane_stride: int, out_row_stride: int):
    """sr_swinir_attention_f32: the window attention (before proj) on a planar qkv tensor of 3 C planes whose q planes are
    already scaled; ``table``: the (225, heads) relative-position bias table; into the C planes of d_out.  Synchronous."""
    t = _sw_bias_table(table, (2 * SWINIR_WINDOW - 1) ** 2, n_heads)
    _sw_attention("sr_swinir_attention_f32", ctx, d_qkv, plane_stride, row_stride, n_feat, n_heads, hp, wp,
                  (int(shift), t.ctypes.data_as(C.c_void_p)), d_out, out_plane_stride, out_row_stride)


# ------------------------------------------------------------------------------------------
# local SR network, HAT (sr_hat_*): sr_network.HATSRNet parses HAT state dicts into these arrays
# ------------------------------------------------------------------------------------------
HAT_WINDOW, HAT_OVERLAP_WINDOW = 16, 24
HAT_REL_ROWS = (2 * HAT_WINDOW - 1) ** 2                          # 961
HAT_OCA_ROWS = (HAT_WINDOW + HAT_OVERLAP_WINDOW - 1) ** 2         # 1521


def hat_desc(n_feat: int, n_heads: int, n_hidden: int, n_mid: int, n_squeeze: int, n_groups: int, depth: int, scale: int,
             conv_scale: float = 0.01, mean=(0.0, 0.0, 0.0), range: float = 1.0) -> HatDesc:  # noqa: A002 (the header's name)
    mean = [float(v) for v in np.asarray(mean, dtype=np.float64).reshape(-1)]
    if len(mean) != 3:
        raise ValueError(f"mean holds 3 values, got {len(mean)}")
    return HatDesc(int(n_feat), int(n_heads), int(n_hidden), int(n_mid), int(n_squeeze), int(n_groups), int(depth), int(scale),
                   float(conv_scale), (C.c_float * 3)(*mean), float(range))


def hat_table_names(desc: HatDesc) -> List[str]:
    """HAT's name of every table in sr_hat_create's order (weight key = name + '.weight', bias key = name + '.bias'; a bias
    table's key is the name itself and it has no bias)."""
    names = ["conv_first", "patch_embed.norm"]
    for i in range(desc.n_groups):
        for j in range(desc.depth):
            b = f"layers.{i}.residual_group.blocks.{j}"
            attn, mlp = _sw_block_names(b)
            names += attn + [f"{b}.conv_block.cab.0", f"{b}.conv_block.cab.2", f"{b}.conv_block.cab.3.attention.1",
                             f"{b}.conv_block.cab.3.attention.3"] + mlp
        names += sum(_sw_block_names(f"layers.{i}.residual_group.overlap_attn", ""), []) + [f"layers.{i}.conv"]
    return names + ["norm", "conv_after_body"] + _sw_shuffle_tail(desc.n_feat, desc.scale)[0]


def hat_table_shapes(desc: HatDesc) -> List[Tuple[tuple, Optional[tuple]]]:
    """(weight shape, bias shape) of every table in sr_hat_create's order; a bias table has no bias (None).  The two 1 x 1
    layers of a CAB's attention are (out, in); (out, in, 1, 1) arrays are accepted for them."""
    Cn, nh, mid, sq, conv, ln = desc.n_feat, desc.n_heads, desc.n_mid, desc.n_squeeze, _sw_conv, ((desc.n_feat,), (desc.n_feat,))
    attn, mlp = _sw_block_shapes(Cn, nh, desc.n_hidden, HAT_REL_ROWS)
    hab = attn + [conv(mid, Cn), conv(Cn, mid), ((sq, Cn), (sq,)), ((Cn, sq), (Cn,))] + mlp
    ocab = sum(_sw_block_shapes(Cn, nh, desc.n_hidden, HAT_OCA_ROWS), [])
    shapes = [conv(Cn, 3), ln] + (hab * desc.depth + ocab + [conv(Cn, Cn)]) * desc.n_groups + [ln, conv(Cn, Cn)]
    return shapes + _sw_shuffle_tail(Cn, desc.scale)[1]


def hat_plan(desc: HatDesc, h: int, w: int, tail: int = 0) -> Tuple[int, int, int, int, int]:
    """sr_hat_plan (host only) -> (padded rows, padded columns, the tail's halo, tail sub-pieces, workspace bytes)."""
    return _sw_plan("sr_hat_plan", desc, h, w, tail)


def hat_rel_index() -> np.ndarray:
    """sr_hat_rel_index (host only) -> (256, 256) int32: the bias-table row of (query token, key token) of a 16 x 16 window."""
    return _sw_index("sr_hat_rel_index", (256, 256))


def hat_oca_index() -> np.ndarray:
    """sr_hat_oca_index (host only) -> (256, 576) int32: the default index of the overlapping cross-attention, wrapped."""
    return _sw_index("sr_hat_oca_index", (256, 576))


def _hat_index(index, name: str = "relative_position_index_OCA") -> Optional[np.ndarray]:
    """A caller's relative_position_index_OCA as contiguous int32 (256, 576), every value in [-1521, 1520]; None stays None.
    ``name``: what a ValueError calls it (a state dict's key)."""
    if index is None:
        return None
    a = np.asarray(index)
    if a.shape != (256, 576) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: expected an integer array of shape (256, 576), got {a.dtype} {a.shape}")
    if a.min() < -HAT_OCA_ROWS or a.max() >= HAT_OCA_ROWS:
        raise ValueError(f"{name}: values must lie in [-{HAT_OCA_ROWS}, {HAT_OCA_ROWS - 1}], got [{int(a.min())}, {int(a.max())}]")
    return np.ascontiguousarray(a, dtype=np.int32)


class HatModel(_SwModel):
    """sr_hat_model: a HAT resident on the GPU.  weights / biases: one fp32 array each per table in forward order
    (hat_table_shapes / hat_table_names); the bias entry of a relative-position table is ignored (None is fine).  ``rpi_oca``:
    the state's relative_position_index_OCA (256, 576), or None for the default formula.  The trunk is one piece, so the
    forwards take ``tail`` alone."""
    _kind, _name, _conv1x1 = "hat", "HAT", True
    _shapes, _plan = staticmethod(hat_table_shapes), staticmethod(hat_plan)

    def __init__(self, ctx: Context, desc: HatDesc, weights, biases, rpi_oca=None):
        ws, bs = self._tables(desc, weights, biases)
        self._rpi = _hat_index(rpi_oca)
        self._create(ctx, (C.byref(desc),), ws, bs)

    def _create(self, ctx: Context, args, ws, bs):
        ptrs = [(C.c_void_p * len(t))(*[a.ctypes.data for a in t]) for t in (ws, bs)]
        h = C.c_void_p()
        rpi = None if self._rpi is None else self._rpi.ctypes.data_as(C.c_void_p)
        _check_unsupported(ctx.lib.sr_hat_create(ctx.handle, *args, *ptrs, len(ws), rpi, C.byref(h)))
        self.ctx, self.handle = ctx, h


def hat_attention(ctx, d_qkv: int, plane_stride: int, row_stride: int, n_feat: int, n_heads: int, hp: int, wp: int, shift: int, table,
                  d_out: int, out_plane_stride: int, out_row_stride: int):
    """sr_hat_attention_f32: the 16 x 16 window attention (before proj) on a planar qkv tensor of 3 C planes whose q planes are
    already scaled; ``table``: the (961, heads) relative-position bias table; into the C planes of d_out.  Synchronous."""
    t = _sw_bias_table(table, HAT_REL_ROWS, n_heads)
    _sw_attention("sr_hat_attention_f32", ctx, d_qkv, plane_stride, row_stride, n_feat, n_heads, hp, wp,
                  (int(shift), t.ctypes.data_as(C.c_void_p)), d_out, out_plane_stride, out_row_stride)


def hat_oca(ctx, d_qkv: int, plane_stride: int, row_stride: int, n_feat: int, n_heads: int, hp: int, wp: int, table, index, d_out: int,
            out_plane_stride: int, out_row_stride: int):
    """sr_hat_oca_f32: the overlapping cross-attention (before proj) on a planar qkv tensor of 3 C planes whose q planes are
    already scaled; ``table``: the (1521, heads) bias table; ``index``: (256, 576) integers in [-1521, 1520] or None for the
    default formula; into the C planes of d_out.  Synchronous."""
    t = _sw_bias_table(table, HAT_OCA_ROWS, n_heads)
    idx = _hat_index(index)
    _sw_attention("sr_hat_oca_f32", ctx, d_qkv, plane_stride, row_stride, n_feat, n_heads, hp, wp,
                  (t.ctypes.data_as(C.c_void_p), None if idx is None else idx.ctypes.data_as(C.c_void_p)), d_out, out_plane_stride,
                  out_row_stride)


# ------------------------------------------------------------------------------------------
# local SR network, Swin2SR (sr_swin2sr_*): sr_network.Swin2SRNet parses `transformers` / official state dicts into these arrays
# ------------------------------------------------------------------------------------------
SWIN2SR_CPB_HIDDEN = 512
SWIN2SR_MASK_PACKAGE, SWIN2SR_MASK_OFFICIAL = -200.0, -100.0     # the package adds the shifted-window mask twice


def swin2sr_desc(n_feat: int, n_heads: int, n_hidden: int, n_groups: int, depth: int, scale: int, upsampler="pixelshuffle",
                 mean=(0.0, 0.0, 0.0), range: float = 1.0, mask_value: float = SWIN2SR_MASK_PACKAGE) -> Swin2srDesc:  # noqa: A002
    mean = [float(v) for v in np.asarray(mean, dtype=np.float64).reshape(-1)]
    if len(mean) != 3:
        raise ValueError(f"mean holds 3 values, got {len(mean)}")
    kind = SWINIR_UPSAMPLERS.get(upsampler, upsampler)
    return Swin2srDesc(int(n_feat), int(n_heads), int(n_hidden), int(n_groups), int(depth), int(scale), int(kind), (C.c_float * 3)(*mean),
                       float(range), float(mask_value))


def _s2_tail_names(desc) -> List[str]:
    if desc.upsampler == 0:
        ups = ["upsample.upsample.convolution"] if desc.scale == 3 else [f"upsample.upsample.convolution_{k}" for k in (0, 1)[:desc.scale // 2]]
        return ["upsample.conv_before_upsample"] + ups + ["upsample.final_convolution"]
    if desc.upsampler == 1:
        return ["upsample.conv"]
    return ["upsample.conv_before_upsample", "upsample.conv_up1", "upsample.conv_up2", "upsample.conv_hr", "upsample.final_convolution"]


def swin2sr_table_names(desc: Swin2srDesc) -> List[str]:
    """The `transformers` package's name of every table in sr_swin2sr_create's order (weight key = name + '.weight', bias key =
    name + '.bias'), except: the qkv table is the package's query / key / value stacked (named '<...>.attention.self.qkv'), and
    the logit_scale table's key is the name itself."""
    names = ["swin2sr.first_convolution", "swin2sr.embeddings.patch_embeddings.projection", "swin2sr.embeddings.patch_embeddings.layernorm"]
    for i in range(desc.n_groups):
        for j in range(desc.depth):
            b = f"swin2sr.encoder.stages.{i}.layers.{j}"
            a = f"{b}.attention.self"
            names += [f"{a}.qkv", f"{a}.logit_scale", f"{a}.continuous_position_bias_mlp.0", f"{a}.continuous_position_bias_mlp.2",
                      f"{b}.attention.output.dense", f"{b}.layernorm_before", f"{b}.intermediate.dense", f"{b}.output.dense",
                      f"{b}.layernorm_after"]
        names += [f"swin2sr.encoder.stages.{i}.conv", f"swin2sr.encoder.stages.{i}.patch_embed.projection"]
    return names + ["swin2sr.layernorm", "swin2sr.conv_after_body"] + _s2_tail_names(desc)


def swin2sr_table_shapes(desc: Swin2srDesc) -> List[Tuple[tuple, Optional[tuple]]]:
    """(weight shape, bias shape) of every table in sr_swin2sr_create's order; logit_scale and cpb_mlp.2 have no bias (None).  The
    1 x 1 projections are (out, in); (out, in, 1, 1) arrays are accepted for them."""
    Cn, nh, hid, s, conv, ln = desc.n_feat, desc.n_heads, desc.n_hidden, desc.scale, _sw_conv, ((desc.n_feat,), (desc.n_feat,))
    lin = ((Cn, Cn), (Cn,))
    layer = [((3 * Cn, Cn), (3 * Cn,)), ((nh,), None), ((SWIN2SR_CPB_HIDDEN, 2), (SWIN2SR_CPB_HIDDEN,)), ((nh, SWIN2SR_CPB_HIDDEN), None), lin, ln,
             ((hid, Cn), (hid,)), ((Cn, hid), (Cn,)), ln]
    shapes = [conv(Cn, 3), lin, ln] + (layer * desc.depth + [conv(Cn, Cn), lin]) * desc.n_groups + [ln, conv(Cn, Cn)]
    if desc.upsampler == 0:
        shapes += _sw_shuffle_tail(Cn, s)[1]
    elif desc.upsampler == 1:
        shapes += [conv(3 * s * s, Cn)]
    else:
        shapes += [conv(64, Cn), conv(64, 64), conv(64, 64), conv(64, 64), conv(3, 64)]
    return shapes


def swin2sr_plan(desc: Swin2srDesc, h: int, w: int, tail: int = 0) -> Tuple[int, int, int, int, int]:
    """sr_swin2sr_plan (host only) -> (padded rows, padded columns, the tail's halo, tail sub-pieces, workspace bytes)."""
    return _sw_plan("sr_swin2sr_plan", desc, h, w, tail)


def swin2sr_cpb_bias(w1, b1, w2, logit_scale=None):
    """sr_swin2sr_cpb_bias (host only): the continuous position bias 16 sigmoid(cpb_mlp(coords)) as a (225, heads) fp32 table
    (float64 from the fp32 weights, rounded once); with ``logit_scale`` (heads values) -> (table, scale), scale[h] =
    (float)exp(min(logit_scale[h], ln 100))."""
    w1, b1, w2 = (np.ascontiguousarray(a, dtype=np.float32) for a in (w1, b1, w2))
    if w2.ndim != 2 or w2.shape[1] != SWIN2SR_CPB_HIDDEN or w1.shape != (SWIN2SR_CPB_HIDDEN, 2) or b1.reshape(-1).shape != (SWIN2SR_CPB_HIDDEN,):
        raise ValueError(f"the cpb MLP is (512, 2), (512,), (heads, 512), got {w1.shape}, {b1.shape}, {w2.shape}")
    heads = int(w2.shape[0])
    table = np.empty(((2 * SWINIR_WINDOW - 1) ** 2, heads), np.float32)
    ls = sc = None
    if logit_scale is not None:
        ls = np.ascontiguousarray(logit_scale, dtype=np.float32).reshape(-1)
        if ls.size != heads:
            raise ValueError(f"logit_scale holds {ls.size} values, expected {heads}")
        sc = np.empty(heads, np.float32)
    _check_unsupported(load().sr_swin2sr_cpb_bias(w1.ctypes.data_as(C.c_void_p), b1.ctypes.data_as(C.c_void_p), w2.ctypes.data_as(C.c_void_p),
                                                  None if ls is None else ls.ctypes.data_as(C.c_void_p), heads,
                                                  table.ctypes.data_as(C.c_void_p), None if sc is None else sc.ctypes.data_as(C.c_void_p)))
    return table if sc is None else (table, sc)


class Swin2srModel(_SwModel):
    """sr_swin2sr_model: a Swin2SR resident on the GPU.  weights / biases: one fp32 array each per table in forward order
    (swin2sr_table_shapes / swin2sr_table_names); the bias entries of logit_scale and cpb_mlp.2 are ignored (None is fine).  The
    trunk is one piece, so the forwards take ``tail`` alone."""
    _kind, _name, _conv1x1 = "swin2sr", "Swin2SR", True
    _shapes, _plan = staticmethod(swin2sr_table_shapes), staticmethod(swin2sr_plan)

    def __init__(self, ctx: Context, desc: Swin2srDesc, weights, biases):
        ws, bs = self._tables(desc, weights, biases)
        self._create(ctx, (C.byref(desc),), ws, bs, count=True)


def swin2sr_attention(ctx, d_qkv: int, plane_stride: int, row_stride: int, n_feat: int, n_heads: int, hp: int, wp: int, shift: int, table,
                      scale, mask_value: float, d_out: int, out_plane_stride: int, out_row_stride: int):
    """sr_swin2sr_attention_f32: the cosine window attention (before proj) on a planar qkv tensor of 3 C planes; ``table``: the
    (225, heads) position bias (swin2sr_cpb_bias); ``scale``: heads values (the clamped exp of logit_scale); into the C planes of
    d_out.  Synchronous."""
    t = _sw_bias_table(table, (2 * SWINIR_WINDOW - 1) ** 2, n_heads)
    sc = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
    if 1 <= int(n_heads) <= 256 and sc.size != int(n_heads):
        raise ValueError(f"scale holds {sc.size} values, expected {int(n_heads)}")
    _sw_attention("sr_swin2sr_attention_f32", ctx, d_qkv, plane_stride, row_stride, n_feat, n_heads, hp, wp,
                  (int(shift), t.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.c_float(float(mask_value))), d_out,
                  out_plane_stride, out_row_stride)


def swin2sr_layernorm_add(ctx, d_x: int, plane_stride: int, row_stride: int, n_feat: int, h: int, w: int, gamma, beta, d_skip: int,
                          skip_plane_stride: int, skip_row_stride: int, d_out: int, out_plane_stride: int, out_row_stride: int):
    """sr_swin2sr_layernorm_add_f32: d_out = d_skip + (float)LayerNorm(d_x) over the channels of planar fp32 tensors on the device;
    d_out may be d_skip itself.  Synchronous."""
    g, b = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (gamma, beta))
    if 1 <= int(n_feat) <= 256 and (g.size != n_feat or b.size != n_feat):
        raise ValueError(f"gamma / beta hold {g.size} / {b.size} values, expected {n_feat}")
    _check_unsupported(load().sr_swin2sr_layernorm_add_f32(_ctx_handle(ctx), C.c_void_p(d_x), int(plane_stride), int(row_stride), int(n_feat),
                                                           int(h), int(w), g.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                                           C.c_void_p(d_skip), int(skip_plane_stride), int(skip_row_stride), C.c_void_p(d_out),
                                                           int(out_plane_stride), int(out_row_stride)))


_default_ctx = {}
_default_lock = threading.Lock()


def default_context(device: int = 0) -> Context:
    """Process-wide context per device.  Raises SrNativeError when no MI355X / HIP device exists."""
    with _default_lock:
        ctx = _default_ctx.get(device)
        if ctx is None:
            ctx = Context(device)
            _default_ctx[device] = ctx
        return ctx

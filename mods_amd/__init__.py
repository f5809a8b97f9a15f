"""mods_amd -- Python harness over the C ABI of libmodsx.so (include/modsx.h).

The product is the shared library (HIP kernels + C++ host engine); this module only
binds it with ctypes so the tests and bench.py can drive it.  There is no Python or
CPU implementation of the path in here: without the built library, or without a GPU,
every device entry point raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MODSX_LIB", os.path.join(_HERE, "libmodsx.so"))   # MODSX_LIB: kernel experiments (tools/)

KEYPOINT = np.dtype([("x", "f8"), ("y", "f8"), ("a11", "f8"), ("a12", "f8"), ("a21", "f8"), ("a22", "f8"),
                     ("s", "f8"), ("response", "f8"), ("octave_number", "i4"), ("pyramid_scale", "f8"),
                     ("sub_type", "i4")], align=True)
REGION = np.dtype([("img_id", "i4"), ("img_reproj_id", "i4"), ("id", "i4"), ("parent_id", "i4"), ("type", "i4"),
                   ("det_kp", KEYPOINT), ("reproj_kp", KEYPOINT)], align=True)
SSKP = np.dtype([("octave", "i4"), ("level", "i4"), ("r0", "i4"), ("c0", "i4"), ("r", "i4"), ("c", "i4"),
                 ("type", "i4"), ("pad", "i4"), ("b0", "f4"), ("b1", "f4"), ("b2", "f4"), ("val", "f4"),
                 ("x", "f4"), ("y", "f4"), ("s", "f4"), ("pixelDistance", "f4")], align=True)
TENT = np.dtype([("q", "i4"), ("t0", "i4"), ("tj", "i4"), ("t1", "i4"), ("d1", "f8"), ("d2", "f8"),
                 ("d2by2ndcl", "f8"), ("ratio", "f8")], align=True)
CANDIDATE = np.dtype([("img", "i4"), ("octave", "i4"), ("level", "i4"), ("type", "i4"), ("r0", "i4"), ("c0", "i4"), ("r", "i4"),
                      ("c", "i4"), ("b0", "f4"), ("b1", "f4"), ("b2", "f4"), ("val", "f4")], align=True)


class HessAffParams(C.Structure):
    _fields_ = [("threshold", C.c_float), ("mode", C.c_int), ("reg_number", C.c_int),
                ("rel_threshold", C.c_float), ("rel_reg_number", C.c_float), ("numberOfScales", C.c_int),
                ("initialSigma", C.c_float), ("edgeEigenValueRatio", C.c_double), ("border", C.c_int),
                ("maxIterations", C.c_int), ("convergenceThreshold", C.c_float), ("smmWindowSize", C.c_int),
                ("affInitialSigma", C.c_float), ("doBaumberg", C.c_int), ("detectorType", C.c_int)]


class SurfDetParams(C.Structure):
    """modsx_surfdet_params: the [SURF] section of the config files"""
    _fields_ = [("octaves", C.c_int), ("intervals", C.c_int), ("init_sample", C.c_int), ("thresh", C.c_float)]


def surfdet_params(octaves=4, intervals=4, init_sample=2, thresh=0.0004):
    return SurfDetParams(int(octaves), int(intervals), int(init_sample), float(thresh))


class KazeParams(C.Structure):
    """modsx_kaze_params: AKAZEOptions as the reference's KAZE branch leaves them"""
    _fields_ = [("omax", C.c_int), ("nsublevels", C.c_int), ("soffset", C.c_float), ("derivative_factor", C.c_float),
                ("dthreshold", C.c_float), ("min_dthreshold", C.c_float), ("kcontrast_percentile", C.c_float),
                ("kcontrast_nbins", C.c_int), ("descriptor", C.c_int), ("diffusivity", C.c_int)]


def kaze_params(**kw):
    """modsx_default_kaze_params with the given fields replaced"""
    p = KazeParams()
    lib().modsx_default_kaze_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(KazeParams._fields_):
            raise TypeError("kaze_params: no field %r" % k)
        setattr(p, k, v)
    return p


# include/modsx.h: modsx_kaze_point
KAZE_POINT = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("response", np.float32),
                       ("octave", np.int32), ("class_id", np.int32)])


class AffShapeParams(C.Structure):
    """modsx_affshape_params: the fields of AffineShapeParams that DetectAffineShape reads"""
    _fields_ = [("maxIterations", C.c_int), ("smmWindowSize", C.c_int), ("convergenceThreshold", C.c_float),
                ("affBmbrgMethod", C.c_int)]


class ClaheParams(C.Structure):
    """modsx_clahe_params: cv::CLAHE's clip limit and tile grid, and which OpenCV's rule (0 = 2.4.9, 1 = 3.x / 4.x)"""
    _fields_ = [("clip_limit", C.c_double), ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("variant", C.c_int)]


class CaffeParams(C.Structure):
    """modsx_caffe_params: mrSize and patchSize of the reference's "CAFFE" branch and its per-channel mean (B, G, R)"""
    _fields_ = [("mrSize", C.c_double), ("patchSize", C.c_int), ("mean", C.c_double * 3)]


class MserParams(C.Structure):
    _fields_ = [("min_size", C.c_int), ("max_area", C.c_double), ("min_margin", C.c_double), ("relative", C.c_int),
                ("mode", C.c_int), ("reg_number", C.c_int), ("rel_threshold", C.c_float), ("rel_reg_number", C.c_float)]


class PairParams(C.Structure):
    _fields_ = [("det", HessAffParams),
                ("ori_mrSize", C.c_double), ("ori_patchSize", C.c_int), ("ori_maxAngles", C.c_int),
                ("ori_threshold", C.c_double),
                ("desc_mrSize", C.c_double), ("desc_patchSize", C.c_int), ("desc_photoNorm", C.c_int),
                ("desc_type", C.c_int), ("desc_maxBinValue", C.c_double),
                ("match_ratio", C.c_double), ("contradDist", C.c_double), ("nn", C.c_int),
                ("duplicateDist", C.c_double),
                ("err_threshold", C.c_double), ("confidence", C.c_double), ("max_samples", C.c_int),
                ("localOptimization", C.c_int), ("HLAFCoef", C.c_double), ("doSymmCheck", C.c_int),
                ("ransac_seed", C.c_uint), ("useF", C.c_int), ("LAFCoef", C.c_double), ("errorType", C.c_int),
                ("detector", C.c_int), ("mser", MserParams),
                ("n_desc", C.c_int), ("desc_types", C.c_int * 4), ("desc_ratios", C.c_double * 4)]


class View(C.Structure):
    _fields_ = [("zoom", C.c_double), ("tilt", C.c_double), ("phi", C.c_double), ("InitSigma", C.c_double),
                ("doBlur", C.c_int)]


def make_view(tilt=1.0, phi=0.0, zoom=1.0, init_sigma=0.5, do_blur=1):
    v = View()
    v.zoom, v.tilt, v.phi, v.InitSigma, v.doBlur = zoom, tilt, phi, init_sigma, do_blur
    return v


def _view_array(views):
    arr = (View * len(views))()
    for i, v in enumerate(views):
        arr[i].zoom, arr[i].tilt, arr[i].phi, arr[i].InitSigma, arr[i].doBlur = v.zoom, v.tilt, v.phi, v.InitSigma, v.doBlur
    return arr


class LadderStep(C.Structure):
    _fields_ = [("views", C.c_void_p), ("nviews", C.c_int), ("match_ratio", C.c_double), ("detector", C.c_int),
                ("n_desc", C.c_int), ("desc_types", C.c_int * 4), ("desc_ratios", C.c_double * 4)]


class PairResult(C.Structure):
    _fields_ = [("n_regions1", C.c_int), ("n_regions2", C.c_int), ("n_tentatives", C.c_int), ("n_unique", C.c_int),
                ("n_ransac_inliers", C.c_int), ("n_verified", C.c_int), ("ransac_samples", C.c_int),
                ("ransac_lo", C.c_int), ("H", C.c_double * 9), ("tentatives", C.c_void_p),
                ("ransac_inlier", C.c_void_p), ("verified", C.c_void_p)]


class RepClassSel(C.Structure):
    _fields_ = [("detector", C.c_int), ("desc_type", C.c_int), ("ratio", C.c_double)]


EXPORTS = ["modsx_version", "modsx_last_error", "modsx_free", "modsx_create", "modsx_destroy", "modsx_synchronize",
           "modsx_default_hessaff_params", "modsx_default_pair_params", "modsx_image_upload", "modsx_image_update",
           "modsx_image_wrap_device", "modsx_image_free", "modsx_image_download", "modsx_detect_affine_keypoints",
           "modsx_detect_scalespace", "modsx_octave_levels", "modsx_gaussian_blur", "modsx_resize_half", "modsx_response",
           "modsx_detect_affine_regions", "modsx_detect_orientation", "modsx_reproject_regions", "modsx_reproject_regions_touch_boundary",
           "modsx_describe_regions", "modsx_match_fginn", "modsx_duplicate_filtering", "modsx_ransac_h",
           "modsx_loransac_h", "modsx_ransac_h_errtype", "modsx_loransac_h_errtype", "modsx_ransac_f", "modsx_loransac_f", "modsx_match_pair", "modsx_match_pairs", "modsx_match_pairs_views", "modsx_pair_result_release",
           "modsx_set_vs_pars", "modsx_synth_view", "modsx_detect_describe_views", "modsx_match_fginn_device",
           "modsx_match_pair_views", "modsx_match_ladder", "modsx_save_regions", "modsx_load_regions", "modsx_default_mser_params", "modsx_detect_msers", "modsx_detect_msers_u8", "modsx_last_timings", "modsx_profile",
           "modsx_kernel_stats", "modsx_last_batch_verify", "modsx_last_match_geometry", "modsx_describe_counters", "modsx_comm_unique_id", "modsx_comm_create", "modsx_comm_destroy", "modsx_comm_info",
           "modsx_view_block_order", "modsx_detect_describe_views_sharded", "modsx_match_fginn_sharded",
           "modsx_match_pair_views_sharded", "modsx_match_pairs_views_sharded", "modsx_match_ladder_sharded", "modsx_comm_loopback_id", "modsx_comm_set_lanes",
           "modsx_comm_attach", "modsx_comm_lane_done", "modsx_comm_reset_lanes", "modsx_comm_set_timeout", "modsx_comm_stats",
           "modsx_shard_block_bytes", "modsx_shard_block_pack", "modsx_shard_blocks_unpack", "modsx_shard_device_pack",
           "modsx_shard_device_unpack", "modsx_verify_device_stats", "modsx_verify_device_timing", "modsx_comm_set_exchange",
           "modsx_shard_owner_plan", "modsx_db_create", "modsx_db_free", "modsx_db_rows", "modsx_db_nearest",
           "modsx_match_fginn_db", "modsx_match_fginn_db_device", "modsx_set_fginn_db",
           "modsx_debug_orientation_counts", "modsx_debug_orientation_launches", "modsx_orientation_tables",
           "modsx_debug_reproject_certain_drop", "modsx_debug_describe_plan", "modsx_debug_describe_plan_slim", "modsx_describe_slim_counters",
           "modsx_debug_views_counters", "modsx_debug_view_plan", "modsx_debug_views_groups", "modsx_debug_synth_views",
           "modsx_debug_baumberg_geometry", "modsx_debug_baumberg_geometry_ctx", "modsx_debug_baumberg_variant",
           "modsx_debug_baumberg", "modsx_debug_check_borders", "modsx_debug_describe_lanes", "modsx_debug_describe_lane_map",
           "modsx_rep_create", "modsx_rep_free", "modsx_rep_add_views", "modsx_rep_append", "modsx_rep_class",
           "modsx_rep_match_fginn", "modsx_match_reps", "modsx_match_one_to_many",
           "modsx_rep_append_f32", "modsx_rep_describe_append", "modsx_rep_class_f32", "modsx_rep_match_fginn_f32",
           "modsx_rep_match_group_f32", "modsx_rep_class_rank", "modsx_debug_fginn32_group_geometry",
           "modsx_fginn32_group_counters",
           "modsx_rep_append_bin", "modsx_rep_append_bin_device", "modsx_rep_class_bin", "modsx_rep_match_hamming",
           "modsx_rep_match_group_hamming", "modsx_rep_class_order", "modsx_debug_hamming_group_geometry",
           "modsx_hamming_group_counters",
           "modsx_match_hamming", "modsx_match_hamming_device", "modsx_hamming_tentatives", "modsx_debug_match_hamming",
           "modsx_match_regions_hamming", "modsx_debug_hamming_geometry",
           "modsx_blur_geometry", "modsx_detect_counters", "modsx_debug_pyramids", "modsx_debug_scan_levels",
           "modsx_debug_detect_scalespace_batch", "modsx_debug_mser_front",
           "modsx_match_fginn_f32", "modsx_match_fginn_f32_device", "modsx_match_regions_f32", "modsx_debug_match_fginn_f32",
           "modsx_debug_fginn32_geometry", "modsx_debug_fginn32_dpass",
           "modsx_match_fginn_f32_dist", "modsx_match_fginn_f32_dist_device", "modsx_match_regions_f32_dist",
           "modsx_debug_match_fginn_f32_dist", "modsx_match_fginn_l1", "modsx_match_fginn_l1_device", "modsx_match_regions_l1",
           "modsx_debug_match_fginn_l1", "modsx_debug_fginn_l1_geometry",
           "modsx_extract_patches", "modsx_extract_patches_device", "modsx_liop_patches", "modsx_liop_patches_device",
           "modsx_describe_regions_liop", "modsx_describe_regions_liop_device", "modsx_liop_tables", "modsx_debug_liop",
           "modsx_liop_counters",
           "modsx_describe_regions_raw", "modsx_describe_regions_raw_device", "modsx_sift_norm_rows", "modsx_sift_norm_rows_device",
           "modsx_describe_regions_dspsift", "modsx_describe_regions_dspsift_device", "modsx_dsp_counters",
           "modsx_surf_patches", "modsx_surf_patches_device", "modsx_describe_regions_surf", "modsx_describe_regions_surf_device",
           "modsx_surf_tables", "modsx_surf_counters",
           "modsx_detect_surf", "modsx_detect_surf_batch", "modsx_surf_regions", "modsx_surfdet_geometry", "modsx_surfdet_normalise",
           "modsx_debug_surfdet", "modsx_surfdet_counters",
           "modsx_default_kaze_params", "modsx_detect_kaze", "modsx_detect_kaze_batch", "modsx_kaze_regions", "modsx_kaze_geometry",
           "modsx_debug_kaze", "modsx_debug_kaze_scan", "modsx_kaze_counters",
           "modsx_default_affshape_params", "modsx_detect_affine_shape", "modsx_detect_affine_shape_batch",
           "modsx_debug_affine_shape", "modsx_affshape_jobs", "modsx_affshape_counters",
           "modsx_default_clahe_params", "modsx_image_clahe", "modsx_image_clahe_new", "modsx_image_clahe_batch",
           "modsx_clahe_geometry", "modsx_debug_clahe", "modsx_clahe_counters",
           "modsx_default_caffe_params", "modsx_caffe_patches", "modsx_caffe_patches_device", "modsx_caffe_jobs",
           "modsx_debug_caffe_geometry", "modsx_caffe_norm_rows", "modsx_caffe_norm_rows_device", "modsx_caffe_counters",
           "modsx_rep_append_f32_device",
           "modsx_daisy_dim", "modsx_daisy_patches", "modsx_daisy_patches_device", "modsx_describe_regions_daisy",
           "modsx_describe_regions_daisy_device", "modsx_daisy_tables", "modsx_daisy_counters"]
# include/modsx_degensac.h: the reference's own verification symbols (link-time drop-in for libdegensac)
EXPORTS_DEGENSAC = ["exp_ransacHcustom", "exp_ransacFcustom", "HDs", "HDsi", "HDsidx", "HDsSym", "HDsiSym", "HDsSymidx",
                    "HDsSymMax", "HDsiSymMax", "HDsSymidxMax", "FDs", "FDsSym", "exFDs", "exFDsSym",
                    "modsx_ransac_set_seed"]

SHARD_ROW_REGION, SHARD_ROW_KP = 0, 1     # include/modsx.h: what of a region travels in a row (all 200 B / the 56 B verification slice)
EXCHANGE_ALL_GATHER, EXCHANGE_OWNER = 0, 1   # include/modsx.h: modsx_comm_set_exchange
# include/modsx.h: modsx_describe_counters, in its order
DESCRIBE_COUNTERS = ("calls", "chunks", "max_chunks", "chunks_mid_image", "chunks_later_image", "jobs", "direct_jobs", "fused_windows",
                     "lds_row_tiles", "lds_col_tiles", "sample_tiles", "global_row_tiles", "global_col_tiles", "clamped_windows")
# ... and behind those, which the planner books (describe_plan gives them too), what only the device counts: k_describe
# workgroups that took the ordered gather.  Context.describe_counters() has both
DESCRIBE_DEVICE_COUNTERS = ("ordered_workgroups",)
# include/modsx.h: modsx_describe_slim_counters, in its order
DESCRIBE_SLIM_COUNTERS = ("slim_launches", "full_launches", "redo_workgroups")
# include/modsx.h: modsx_detect_counters, in its order
DETECT_COUNTERS = ("blur_th16", "blur_th32") + tuple("blur_r%d" % r for r in range(1, 9)) + (
    "hessian", "resize", "scan_per_octave", "scan_per_level", "nms_flushes", "last_jobs", "last_tiles", "last_accepted",
    "second_copies")
# include/modsx.h: modsx_liop_counters, in its order
LIOP_COUNTERS = ("calls", "regions", "exact_path", "sub_batches")
LIOP_DIM, LIOP_PIXELS = 144, 673      # include/modsx.h: MODSX_LIOP_DIM, MODSX_LIOP_PIXELS
# include/modsx.h: modsx_dsp_counters, in its order
DSP_COUNTERS = ("calls", "regions", "scale_passes")
# include/modsx.h: modsx_surf_counters, in its order
SURF_COUNTERS = ("calls", "patches", "sub_batches")
SURF_DIM = 64                         # include/modsx.h: MODSX_SURF_DIM
# include/modsx.h: modsx_surfdet_counters, in its order
SURFDET_COUNTERS = ("calls", "images", "extrema", "accepted", "regrows")
# include/modsx.h: modsx_kaze_counters, in its order
KAZE_COUNTERS = ("calls", "images", "launches", "fed_steps", "host_waits", "raw_maxima", "survivors", "keypoints", "filter_us")
KAZE_MAX_LEVELS, KAZE_MAX_TAU, DET_KAZE = 32, 64, 9     # include/modsx.h: MODSX_KAZE_MAX_LEVELS, MODSX_KAZE_MAX_TAU, MODSX_DET_KAZE
# include/modsx.h: modsx_affshape_counters, in its order
AFFSHAPE_COUNTERS = ("calls", "regions", "border_refused", "launched", "converged", "launches")
# include/modsx.h: modsx_clahe_counters and modsx_clahe_geometry, in their order
CLAHE_COUNTERS = ("calls", "images", "tiles", "strips", "pixels", "launches")
CLAHE_GEOMETRY = ("tile_w", "tile_h", "pad_cols", "pad_rows", "clip_limit", "lut_scale_bits", "strips", "strip_rows", "apply_blocks")
CLAHE_MAX_TILES = 256                     # include/modsx.h: MODSX_CLAHE_MAX_TILES
# include/modsx.h: modsx_caffe_counters, modsx_debug_caffe_geometry and modsx_caffe_jobs, in their order
CAFFE_COUNTERS = ("calls", "regions", "border_regions", "launches")
CAFFE_GEOMETRY = ("workgroups", "waves", "chunks", "chunk_cols", "lds_stride", "lds_bytes_gray", "lds_bytes_colour")
CAFFE_JOB_FIELDS = ("curr_sc", "x", "y", "a11", "a12", "a21", "a22")
CAFFE_MAX_PATCH, CAFFE_MAX_DIM = 255, 4096      # include/modsx.h: MODSX_CAFFE_MAX_PATCH, MODSX_CAFFE_MAX_DIM
CAFFE_NORM_L2, CAFFE_NORM_L1, CAFFE_NORM_ROOTL2, CAFFE_NORM_NONE = 0, 1, 2, 3
CAFFE_NORMS = {"L2": CAFFE_NORM_L2, "L1": CAFFE_NORM_L1, "RootL2": CAFFE_NORM_ROOTL2, "none": CAFFE_NORM_NONE}   # `Normalization=`
DET_SURF, SURFDET_MAX_LAYERS = 6, 12      # include/modsx.h: MODSX_DET_SURF, MODSX_SURFDET_MAX_LAYERS
DET_HESSIAN, DET_MSER = 0, 3              # include/modsx.h: MODSX_DET_HESSIAN, MODSX_DET_MSER
# include/modsx.h: the float descriptor classes of a stored representation, and the first capacity of such a class in rows
DESC_CAFFE, DESC_DAISY, DESC_LIOP, DESC_MROGH, DESC_SURF = 8, 9, 10, 11, 12
REP_F32_FIRST_ROWS = 4096
DIST_L2, DIST_L1 = 0, 1               # include/modsx.h: MODSX_DIST_L2, MODSX_DIST_L1 (vector_dist of the [Matching] section)
# include/modsx.h: the binary descriptor classes of a stored representation, their own detector, the first capacity in rows
DET_ORB = 4
DESC_BRISK, DESC_FREAK, DESC_ORB = 16, 17, 18
REP_BIN_FIRST_ROWS = 4096
# include/modsx.h: modsx_hamming_group_counters, in its order
HAMMING_GROUP_COUNTERS = ("launch_sets", "problems", "rows_packed", "match_pack_launches")
# include/modsx.h: modsx_daisy_counters, in its order
DAISY_COUNTERS = ("calls", "patches", "sub_batches")
DAISY_MAX_DIM, DAISY_MAX_TAPS = 200, 51      # include/modsx.h: MODSX_DAISY_MAX_DIM, MODSX_DAISY_MAX_TAPS
DAISY_NRM_PARTIAL, DAISY_NRM_FULL, DAISY_NRM_SIFT = 0, 1, 2
DAISY_SKIPPED, DAISY_ZEROED, DAISY_SAMPLED = 0, 1, 2     # modsx_daisy_tables: the state of a grid point
MAXB = 32                             # csrc/engine.hpp: MODSX_MAXB, the views / images of one launch set
KP_FIELDS = ("x", "y", "a11", "a12", "a21", "a22", "s")
KERNEL_CLASSES = ["blur_hess", "hessian", "resize", "nms_localize", "baumberg", "orientation", "patch_sample",
                  "blur_rows", "describe", "match_fginn", "gray", "warp_affine", "view_blur", "blur_cols", "match_sweep1", "match_db"]


def build(force=False):
    """Compile libmodsx.so for gfx950 with hipcc (in-tree)."""
    src = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".hip", ".cpp", ".hpp"))]
    srcs.append(os.path.join(_HERE, "..", "include", "modsx.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", src, "-j8"], stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libmodsx.so is not built; run __graft_entry__.build() (needs hipcc)")
        L = C.CDLL(LIB_PATH)
        L.modsx_last_error.restype = C.c_char_p
        L.modsx_create.restype = C.c_void_p
        L.modsx_create.argtypes = [C.c_int]
        L.modsx_comm_create.restype = C.c_void_p
        L.modsx_comm_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.modsx_comm_destroy.argtypes = [C.c_void_p]
        L.modsx_comm_info.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        L.modsx_comm_loopback_id.argtypes = [C.c_void_p, C.c_int]
        L.modsx_comm_set_lanes.argtypes = [C.c_void_p, C.c_int]
        L.modsx_comm_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_comm_lane_done.argtypes = [C.c_void_p, C.c_int]
        L.modsx_comm_reset_lanes.argtypes = [C.c_void_p]
        L.modsx_comm_set_timeout.argtypes = [C.c_void_p, C.c_int]
        L.modsx_comm_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_destroy.argtypes = [C.c_void_p]
        L.modsx_free.argtypes = [C.c_void_p]
        L.modsx_image_upload.restype = C.c_void_p
        L.modsx_image_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.modsx_image_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.modsx_debug_last_batch_verify_each.argtypes = [C.c_void_p, C.c_int]
        L.modsx_image_wrap_device.restype = C.c_void_p
        L.modsx_image_wrap_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.modsx_image_free.argtypes = [C.c_void_p, C.c_void_p]
        L.modsx_db_create.restype = C.c_void_p
        L.modsx_db_create.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int]
        L.modsx_db_free.restype = None
        L.modsx_db_free.argtypes = [C.c_void_p, C.c_void_p]
        L.modsx_db_rows.restype = C.c_long
        L.modsx_db_rows.argtypes = [C.c_void_p]
        L.modsx_db_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.modsx_set_fginn_db.argtypes = [C.c_void_p, C.c_void_p]
        L.modsx_debug_reproject_certain_drop.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
        L.modsx_describe_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_describe_slim_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_debug_describe_plan_slim.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_ulonglong, C.c_void_p, C.c_int,
                                                     C.c_void_p]
        L.modsx_debug_orientation_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_debug_orientation_launches.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_orientation_tables.argtypes = [C.c_void_p] * 6
        L.modsx_debug_views_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_debug_view_plan.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_debug_views_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_debug_synth_views.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.modsx_blur_geometry.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.modsx_detect_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_debug_pyramids.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_ulonglong,
                                           C.c_void_p]
        L.modsx_debug_scan_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_debug_detect_scalespace_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_debug_mser_front.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_debug_describe_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_ulonglong, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_int, C.c_void_p]
        L.modsx_debug_baumberg_geometry.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.modsx_debug_baumberg.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_debug_baumberg_variant.argtypes = [C.c_int]
        L.modsx_debug_baumberg_geometry_ctx.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.modsx_debug_check_borders.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.modsx_debug_describe_lanes.argtypes = [C.c_int, C.c_void_p]
        L.modsx_debug_describe_lane_map.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_rep_create.restype = C.c_void_p
        L.modsx_rep_create.argtypes = [C.c_void_p]
        L.modsx_rep_free.restype = None
        L.modsx_rep_free.argtypes = [C.c_void_p, C.c_void_p]
        L.modsx_rep_add_views.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_rep_append.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.modsx_rep_class.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.modsx_rep_match_fginn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                            C.c_void_p]
        L.modsx_rep_append_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.modsx_rep_describe_append.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                                C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.modsx_rep_class_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_rep_match_fginn_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                                C.c_void_p]
        L.modsx_rep_match_group_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                C.c_int, C.c_void_p, C.c_void_p]
        L.modsx_rep_class_rank.argtypes = [C.c_int, C.c_int]
        L.modsx_debug_fginn32_group_geometry.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_int]
        L.modsx_fginn32_group_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_rep_append_bin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.modsx_rep_append_bin_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.modsx_rep_class_bin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_rep_match_hamming.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
        L.modsx_rep_match_group_hamming.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                                    C.c_void_p]
        L.modsx_rep_class_order.argtypes = [C.c_int, C.c_int]
        L.modsx_debug_hamming_group_geometry.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_int]
        L.modsx_hamming_group_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_match_reps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p]
        L.modsx_match_one_to_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_match_hamming.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]
        L.modsx_match_hamming_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
        L.modsx_hamming_tentatives.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p]
        L.modsx_debug_match_hamming.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_void_p]
        L.modsx_debug_hamming_last_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.modsx_match_regions_hamming.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        L.modsx_match_fginn_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                            C.c_double, C.c_int, C.c_void_p]
        L.modsx_match_fginn_f32_device.argtypes = L.modsx_match_fginn_f32.argtypes
        L.modsx_match_regions_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p]
        L.modsx_debug_match_fginn_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                                  C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
        f32a, rega, dbga = (list(f.argtypes) for f in (L.modsx_match_fginn_f32, L.modsx_match_regions_f32, L.modsx_debug_match_fginn_f32))
        L.modsx_match_fginn_f32_dist.argtypes = f32a[:10] + [C.c_int] + f32a[10:]            # dist behind nn
        L.modsx_match_fginn_f32_dist_device.argtypes = L.modsx_match_fginn_f32_dist.argtypes
        L.modsx_match_regions_f32_dist.argtypes = rega[:9] + [C.c_int] + rega[9:]            # dist behind par
        L.modsx_debug_match_fginn_f32_dist.argtypes = dbga[:10] + [C.c_int] + dbga[10:]
        L.modsx_match_fginn_l1.argtypes = f32a[:5] + f32a[6:]                                # no dim
        L.modsx_match_fginn_l1_device.argtypes = L.modsx_match_fginn_l1.argtypes
        L.modsx_match_regions_l1.argtypes = rega[:7] + rega[8:]
        L.modsx_debug_match_fginn_l1.argtypes = dbga[:5] + dbga[6:]
        L.modsx_debug_fginn_l1_geometry.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.modsx_debug_fginn32_geometry.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.modsx_debug_fginn32_dpass.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.modsx_debug_fginn32_last_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.modsx_extract_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.modsx_extract_patches_device.argtypes = L.modsx_extract_patches.argtypes
        L.modsx_describe_regions_liop.argtypes = L.modsx_extract_patches.argtypes
        L.modsx_describe_regions_liop_device.argtypes = L.modsx_extract_patches.argtypes
        L.modsx_liop_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.modsx_liop_patches_device.argtypes = L.modsx_liop_patches.argtypes
        L.modsx_liop_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_debug_liop.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_liop_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_describe_regions_raw.argtypes = L.modsx_extract_patches.argtypes
        L.modsx_describe_regions_raw_device.argtypes = L.modsx_extract_patches.argtypes
        L.modsx_sift_norm_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
        L.modsx_sift_norm_rows_device.argtypes = L.modsx_sift_norm_rows.argtypes
        L.modsx_describe_regions_dspsift.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                                     C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
        L.modsx_describe_regions_dspsift_device.argtypes = L.modsx_describe_regions_dspsift.argtypes
        L.modsx_dsp_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_surf_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
        L.modsx_surf_patches_device.argtypes = L.modsx_surf_patches.argtypes
        L.modsx_describe_regions_surf.argtypes = L.modsx_extract_patches.argtypes
        L.modsx_describe_regions_surf_device.argtypes = L.modsx_extract_patches.argtypes
        L.modsx_surf_tables.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_surf_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_daisy_dim.argtypes = [C.c_int, C.c_int, C.c_int]
        L.modsx_daisy_patches.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]
        L.modsx_daisy_patches_device.argtypes = L.modsx_daisy_patches.argtypes
        L.modsx_describe_regions_daisy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double] + [C.c_int] * 8 + [C.c_void_p]
        L.modsx_describe_regions_daisy_device.argtypes = L.modsx_describe_regions_daisy.argtypes
        L.modsx_detect_surf.argtypes = [C.c_void_p] * 4
        L.modsx_detect_surf_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_surf_regions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.modsx_surfdet_geometry.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.modsx_surfdet_normalise.argtypes = [C.c_void_p, C.c_void_p]
        L.modsx_debug_surfdet.argtypes = [C.c_void_p] * 13 + [C.c_int, C.c_void_p]
        L.modsx_surfdet_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_default_kaze_params.argtypes = [C.c_void_p]
        L.modsx_default_kaze_params.restype = None
        L.modsx_detect_kaze.argtypes = [C.c_void_p] * 4
        L.modsx_detect_kaze_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_kaze_regions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.modsx_kaze_geometry.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6
        L.modsx_debug_kaze.argtypes = [C.c_void_p] * 14 + [C.c_int, C.c_void_p]
        L.modsx_debug_kaze_scan.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
        L.modsx_kaze_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_daisy_tables.argtypes = [C.c_int] * 4 + [C.c_void_p] * 9
        L.modsx_default_affshape_params.restype = None
        L.modsx_default_affshape_params.argtypes = [C.c_void_p]
        L.modsx_detect_affine_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.modsx_detect_affine_shape_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.modsx_debug_affine_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.modsx_affshape_jobs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_affshape_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_daisy_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_default_clahe_params.restype = None
        L.modsx_default_clahe_params.argtypes = [C.c_void_p]
        L.modsx_image_clahe.argtypes = [C.c_void_p] * 4
        L.modsx_image_clahe_new.restype = C.c_void_p
        L.modsx_image_clahe_new.argtypes = [C.c_void_p] * 3
        L.modsx_image_clahe_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.modsx_clahe_geometry.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.modsx_debug_clahe.argtypes = [C.c_void_p] * 5
        L.modsx_clahe_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_debug_clahe_last_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.modsx_default_caffe_params.restype = None
        L.modsx_default_caffe_params.argtypes = [C.c_void_p]
        L.modsx_caffe_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.modsx_caffe_patches_device.argtypes = L.modsx_caffe_patches.argtypes
        L.modsx_caffe_jobs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.modsx_debug_caffe_geometry.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.modsx_caffe_norm_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.modsx_caffe_norm_rows_device.argtypes = L.modsx_caffe_norm_rows.argtypes
        L.modsx_caffe_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.modsx_rep_append_f32_device.argtypes = L.modsx_rep_append_f32.argtypes
        L.modsx_synth_view.restype = C.c_void_p
        L.modsx_synth_view.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _err():
    return lib().modsx_last_error().decode()


def _patch_rows(patches):
    patches = np.ascontiguousarray(patches, np.float32)
    if patches.ndim == 2 and patches.shape == (41, 41):
        patches = patches[None]
    if patches.shape[1:] not in ((41, 41), (1681,)):
        raise ValueError("LIOP patches are [n][41][41] float32")
    return patches


def liop_tables(patch_size=41):
    """(pixels [673] int32, sx [673][4] float64, sy [673][4] float64): the measurement pixels (x + 41 y, raster order) and
    neighbour sample coordinates of vl_liopdesc_new_basic(41), as the library builds them on the host (no device needed)."""
    n = lib().modsx_liop_tables(int(patch_size), None, None, None, 0)
    if n < 0:
        raise RuntimeError("liop_tables failed: " + _err())
    pixels, sx, sy = np.zeros(n, np.int32), np.zeros((n, 4), np.float64), np.zeros((n, 4), np.float64)
    got = lib().modsx_liop_tables(int(patch_size), _p(pixels), _p(sx), _p(sy), n)
    assert got == n, (got, n)
    return pixels, sx, sy


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def surf_tables(mr_size=5.1962, patch_size=41):
    """dict(sample_x [24] int32, sample_y [24] int32, w1 [16][81] float32, w2 [16] float32, haar_size int): the sample
    coordinates (index k + 12, l + 12), the gaussian weights and the Haar size of the SURF functor at (patch_size, mr_size), as
    the library builds them on the host (no device needed)."""
    sx, sy = np.zeros(24, np.int32), np.zeros(24, np.int32)
    w1, w2, hs = np.zeros((16, 81), np.float32), np.zeros(16, np.float32), np.zeros(1, np.int32)
    if lib().modsx_surf_tables(int(patch_size), C.c_double(mr_size), _p(sx), _p(sy), _p(w1), _p(w2), _p(hs)) != 0:
        raise RuntimeError("surf_tables failed: " + _err())
    return dict(sample_x=sx, sample_y=sy, w1=w1, w2=w2, haar_size=int(hs[0]))


def daisy_dim(radq=3, thq=8, histq=8):
    """(radq * thq + 1) * histq, the width of a DAISY row; raises for values the library refuses (no device needed)."""
    d = lib().modsx_daisy_dim(int(radq), int(thq), int(histq))
    if d < 0:
        raise RuntimeError("daisy_dim failed: " + _err())
    return d


def daisy_tables(rad=15, radq=3, thq=8, histq=8):
    """dict(k5 [5], kos [8], zin [8] float32, fsz [1 + radq] int32, taps [1 + radq][51] float32 (zero beyond fsz), selected [radq],
    state / base [npts] int32, w [npts][4] float32): the filters, layer directions and grid points of the DAISY functor at (rad,
    radq, thq, histq) on a 41 x 41 patch, as the library builds them on the host (no device needed); include/modsx.h:
    modsx_daisy_tables."""
    npts = daisy_dim(radq, thq, histq) // int(histq)
    k5, kos, zin = np.zeros(5, np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32)
    fsz, taps = np.zeros(1 + radq, np.int32), np.zeros((1 + radq, DAISY_MAX_TAPS), np.float32)
    sel, state, base, w = np.zeros(radq, np.int32), np.zeros(npts, np.int32), np.zeros(npts, np.int32), np.zeros((npts, 4), np.float32)
    if lib().modsx_daisy_tables(int(rad), int(radq), int(thq), int(histq), _p(k5), _p(kos), _p(zin), _p(fsz), _p(taps), _p(sel), _p(state),
                                _p(base), _p(w)) != 0:
        raise RuntimeError("daisy_tables failed: " + _err())
    return dict(k5=k5, kos=kos, zin=zin, fsz=fsz, taps=taps, selected=sel, state=state, base=base, w=w)


def _check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, _err()))
    return rc


def default_hessaff_params(**kw):
    p = HessAffParams()
    lib().modsx_default_hessaff_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_mser_params(**kw):
    p = MserParams()
    lib().modsx_default_mser_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def detect_msers_u8(gray, params=None, tilt=1.0, zoom=1.0):
    """DetectMSERs on a host u8 image (no device needed)."""
    params = params or default_mser_params()
    g = np.ascontiguousarray(gray, np.uint8)
    out = C.c_void_p()
    n = _check(lib().modsx_detect_msers_u8(_p(g), g.shape[0], g.shape[1], C.byref(params), C.c_double(tilt),
                                           C.c_double(zoom), C.byref(out)), "detect_msers_u8")
    return _take(out, n, KEYPOINT)


def default_pair_params(**kw):
    p = PairParams()
    lib().modsx_default_pair_params(C.byref(p))
    descs = kw.pop("descs", None)     # [(MODSX_DESC_* type, FGINN ratio), ...]: the step's Descriptors / FGINNThreshold lists
    if descs is not None:
        _set_descs(p, descs)
    for k, v in kw.items():
        if hasattr(p.det, k) and not hasattr(p, k):
            setattr(p.det, k, v)
        else:
            setattr(p, k, v)
    return p


def _set_descs(obj, descs):
    obj.n_desc = len(descs)
    for i, (t, r) in enumerate(descs):
        obj.desc_types[i] = int(t)
        obj.desc_ratios[i] = float(r)


def _take(ptr, n, dtype):
    """Copy a malloc'd array returned through `**out` into numpy and free it."""
    if n <= 0:
        if ptr:
            lib().modsx_free(ptr)
        return np.zeros(0, dtype)
    buf = (C.c_char * (n * dtype.itemsize)).from_address(ptr.value if hasattr(ptr, "value") else ptr)
    arr = np.frombuffer(buf, dtype=dtype, count=n).copy()
    lib().modsx_free(ptr)
    return arr


# ---- host-only entry points (no device needed) ---------------------------------------------------
def detect_affine_regions(kps, img_id=0, det_type=0):
    kps = np.ascontiguousarray(kps, KEYPOINT)
    out = np.zeros(len(kps), REGION)
    _check(lib().modsx_detect_affine_regions(_p(kps), len(kps), img_id, det_type, _p(out)), "detect_affine_regions")
    return out


def surf_regions(kps, img_id=0):
    """Regions of SURF keypoints as the reference's SURF branch leaves them: type DET_SURF, det_kp as given (no device needed)."""
    kps = np.ascontiguousarray(kps, KEYPOINT)
    out = np.zeros(len(kps), REGION)
    _check(lib().modsx_surf_regions(_p(kps), len(kps), int(img_id), _p(out)), "surf_regions")
    return out


def default_affshape_params(**kw):
    """AffineShapeParams() as DetectAffineShape reads it: maxIterations 16, smmWindowSize 19, convergenceThreshold 0.05, SMM."""
    p = AffShapeParams()
    lib().modsx_default_affshape_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def affshape_jobs(regs, cols, rows):
    """dict(ratio [n] f32, res [n] i32, border [n] bool): what DetectAffineShape forms on the host for every region of a cols x rows
    image -- (float)(s / (double)1.6f), the truncated window argument (int)(10.0 * ratio) and the up-front border test with the
    region's own matrix (no device needed); raises for regions or images the library refuses."""
    regs = np.ascontiguousarray(regs, REGION)
    n = len(regs)
    ratio, res, border = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
    _check(lib().modsx_affshape_jobs(_p(regs), n, int(cols), int(rows), _p(ratio), _p(res), _p(border)), "affshape_jobs")
    return dict(ratio=ratio[:n], res=res[:n], border=border[:n].astype(bool))


def clahe_params(clip_limit=4.0, tiles=(8, 8), variant=0):
    """modsx_clahe_params; tiles = (tiles_x, tiles_y) as cv::Size(width, height).  The defaults are what the drivers set."""
    p = ClaheParams()
    lib().modsx_default_clahe_params(C.byref(p))
    p.clip_limit, p.tiles_x, p.tiles_y, p.variant = float(clip_limit), int(tiles[0]), int(tiles[1]), int(variant)
    return p


def clahe_geometry(rows, cols, clip_limit=4.0, tiles=(8, 8), variant=0):
    """dict of CLAHE_GEOMETRY (and lut_scale as np.float32): the tile and padded size, clipLimit, lutScale, the histogram
    launch's strips per tile / rows per strip and the pixel pass's workgroups for a rows x cols image, from the function the
    launcher itself calls (no device needed); raises for what the library refuses."""
    out = np.zeros(len(CLAHE_GEOMETRY), np.int32)
    n = _check(lib().modsx_clahe_geometry(int(rows), int(cols), C.byref(clahe_params(clip_limit, tiles, variant)), _p(out)),
               "clahe_geometry")
    assert n == len(CLAHE_GEOMETRY), n
    g = dict(zip(CLAHE_GEOMETRY, (int(x) for x in out)))
    g["lut_scale"] = out[5:6].view(np.float32)[0]
    return g


def caffe_params(mr_size=None, patch_size=None, mean=None):
    """modsx_caffe_params; the defaults are the library's: mrSize 3 sqrt(3), patchSize 41, mean (104, 117, 123) in B, G, R order."""
    p = CaffeParams()
    lib().modsx_default_caffe_params(C.byref(p))
    if mr_size is not None:
        p.mrSize = float(mr_size)
    if patch_size is not None:
        p.patchSize = int(patch_size)
    if mean is not None:
        p.mean[0], p.mean[1], p.mean[2] = (float(m) for m in mean)
    return p


def caffe_jobs(regs, par, rows, cols):
    """dict(curr_sc, x, y, a11, a12, a21, a22 [n] f32, border [n] bool): what the "CAFFE" branch calls interpolate with for every
    region on planes of rows x cols, and interpolateCheckBorders for it -- from the function that fills the launcher's job table
    (no device needed); raises for what the library refuses."""
    regs = np.ascontiguousarray(regs, REGION)
    n = len(regs)
    out = np.zeros((max(n, 1), 8), np.float32)
    _check(lib().modsx_caffe_jobs(_p(regs), n, C.byref(par), int(rows), int(cols), _p(out)), "caffe_jobs")
    d = {k: out[:n, i].copy() for i, k in enumerate(CAFFE_JOB_FIELDS)}
    d["border"] = out[:n, 7] != 0
    return d


def caffe_geometry(n, patch_size):
    """dict of CAFFE_GEOMETRY: the work split the patch launcher uses for n regions at patch_size (no device needed)."""
    out = np.zeros(len(CAFFE_GEOMETRY), np.int32)
    got = _check(lib().modsx_debug_caffe_geometry(int(n), int(patch_size), _p(out)), "caffe_geometry")
    assert got == len(CAFFE_GEOMETRY), got
    return dict(zip(CAFFE_GEOMETRY, (int(x) for x in out)))


def surfdet_normalise(params):
    """The parameters as FastHessian::saveParameters stores them (no device needed)."""
    out = SurfDetParams()
    _check(lib().modsx_surfdet_normalise(C.byref(params), C.byref(out)), "surfdet_normalise")
    return out


def surfdet_geometry(rows, cols, params=None):
    """[n][4] int32 (width, height, step, filter): the response layers the SURF detector builds for a rows x cols image; raises
    where the library refuses the image (no device needed)."""
    params = params or surfdet_params()
    layers = np.zeros((SURFDET_MAX_LAYERS, 4), np.int32)
    n = _check(lib().modsx_surfdet_geometry(int(rows), int(cols), C.byref(params), _p(layers)), "surfdet_geometry")
    return layers[:n].copy()


def kaze_regions(kps, img_id=0):
    """Regions of KAZE keypoints as the reference's KAZE branch leaves them: type DET_KAZE, det_kp as given (no device needed)."""
    kps = np.ascontiguousarray(kps, KEYPOINT)
    out = np.zeros(len(kps), REGION)
    _check(lib().modsx_kaze_regions(_p(kps), len(kps), int(img_id), _p(out)), "kaze_regions")
    return out


def kaze_geometry(rows, cols, params=None):
    """dict(levels [n][8] int32 (octave, sublevel, rows, cols, sigma_size, derivative kernel size, derivative distance, FED steps),
    sigmas [n][2] f32 (esigma, etime), tau: a list of f32 arrays, tiles: dict(width, height, scan, max_distance), omax): the level
    table the KAZE detector builds for a rows x cols image; raises where the library refuses (no device needed)."""
    params = params or kaze_params()
    levels, sig = np.zeros((KAZE_MAX_LEVELS, 8), np.int32), np.zeros((KAZE_MAX_LEVELS, 2), np.float32)
    tau, tiles, omax = np.zeros((KAZE_MAX_LEVELS, KAZE_MAX_TAU), np.float32), np.zeros(4, np.int32), C.c_int(0)
    n = _check(lib().modsx_kaze_geometry(int(rows), int(cols), C.byref(params), _p(levels), _p(sig), _p(tau), _p(tiles), C.byref(omax)),
               "kaze_geometry")
    return dict(levels=levels[:n].copy(), sigmas=sig[:n].copy(), tau=[tau[i, :levels[i, 7]].copy() for i in range(n)],
                tiles=dict(zip(("width", "height", "scan", "max_distance"), (int(v) for v in tiles))), omax=omax.value)


def reproject_regions(regs, H, w, h):
    regs = np.ascontiguousarray(regs, REGION).copy()
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    n = _check(lib().modsx_reproject_regions(_p(regs), len(regs), _p(H), int(w), int(h)), "reproject_regions")
    return regs[:n].copy()


def reproject_regions_touch_boundary(regs, H, w, h, mr_size=3.0 * 3.0 ** 0.5):
    regs = np.ascontiguousarray(regs, REGION).copy()
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    n = _check(lib().modsx_reproject_regions_touch_boundary(_p(regs), len(regs), _p(H), int(w), int(h), C.c_double(mr_size)),
               "reproject_regions_touch_boundary")
    return regs[:n].copy()


def duplicate_filtering(pts, key, r=2.0, do_sort=True):
    pts = np.ascontiguousarray(pts, np.float64)
    key = np.ascontiguousarray(key, np.float64)
    T = len(pts)
    order = np.zeros(max(T, 1), np.int32)
    keep = np.zeros(max(T, 1), np.uint8)
    _check(lib().modsx_duplicate_filtering(_p(pts), _p(key), T, C.c_double(r), int(do_sort), _p(order), _p(keep)),
           "duplicate_filtering")
    return order[:T], keep[:T].astype(bool)


def ransac_h(u, th, conf=0.99, max_sam=100000, oriented=1, sym_check=1, seed=1):
    u = np.ascontiguousarray(u, np.float64)
    n = len(u)
    H = np.zeros(9)
    inl = np.zeros(n, np.uint8)
    dout = np.zeros(3, np.int32)
    J = C.c_double(0)
    rc = _check(lib().modsx_ransac_h(_p(u), n, C.c_double(th), C.c_double(conf), int(max_sam), _p(H), _p(inl), _p(dout),
                                     int(oriented), int(sym_check), C.c_uint(seed), C.byref(J)), "ransac_h")
    return dict(n=rc, H=H, inl=inl.astype(bool), samples=int(dout[0]), lo_count=int(dout[1]),
                ori_rejects=int(dout[2]), J=J.value)


def loransac_h(pts, laf1, laf2, err_threshold=3.0, confidence=0.99, max_samples=100000, lo=1, hlaf_coef=12.0,
               sym_check=1, seed=1, error_type=0):
    pts = np.ascontiguousarray(pts, np.float64)
    laf1 = np.ascontiguousarray(laf1, np.float64)
    laf2 = np.ascontiguousarray(laf2, np.float64)
    T = len(pts)
    H, Hraw = np.zeros(9), np.zeros(9)
    inl = np.zeros(max(T, 1), np.uint8)
    keep = np.zeros(max(T, 1), np.uint8)
    dout = np.zeros(3, np.int32)
    n = _check(lib().modsx_loransac_h_errtype(_p(pts), _p(laf1), _p(laf2), T, C.c_double(err_threshold),
                                              C.c_double(confidence), int(max_samples), int(lo), C.c_double(hlaf_coef),
                                              int(sym_check), int(error_type), C.c_uint(seed), _p(H), _p(Hraw), _p(inl),
                                              _p(keep), _p(dout)), "loransac_h")
    return dict(n=n, H=H.reshape(3, 3), Hraw=Hraw, inl=inl[:T].astype(bool), keep=keep[:T].astype(bool),
                samples=int(dout[0]), lo_count=int(dout[1]), ori_rejects=int(dout[2]))


def loransac_f(pts, laf1, laf2, err_threshold=4.0, confidence=0.99, max_samples=100000, lo=1, laf_coef=3.0,
               sym_check=1, error_type=0, seed=1):
    """LORANSACFiltering with useF = 1 (exp_ransacFcustom + F_LAF_check), host C++."""
    pts = np.ascontiguousarray(pts, np.float64)
    laf1 = np.ascontiguousarray(laf1, np.float64)
    laf2 = np.ascontiguousarray(laf2, np.float64)
    T = len(pts)
    F = np.zeros(9)
    inl = np.zeros(max(T, 1), np.uint8)
    keep = np.zeros(max(T, 1), np.uint8)
    dout = np.zeros(3, np.int32)
    n = _check(lib().modsx_loransac_f(_p(pts), _p(laf1), _p(laf2), T, C.c_double(err_threshold),
                                      C.c_double(confidence), int(max_samples), int(lo), C.c_double(laf_coef),
                                      int(sym_check), int(error_type), C.c_uint(seed), _p(F), _p(inl), _p(keep),
                                      _p(dout)), "loransac_f")
    return dict(n=n, F=F.reshape(3, 3), inl=inl[:T].astype(bool), keep=keep[:T].astype(bool),
                samples=int(dout[0]), lo_count=int(dout[1]), degen_count=int(dout[2]))


def verify_device_stats(reset=False):
    """modsx_verify_device_stats: how much of DEGENSAC's rFtH hypothesis loop ran on the device (process-wide counters)."""
    out = (C.c_long * 6)()
    lib().modsx_verify_device_stats(out, int(bool(reset)))
    d = dict(zip(("batches", "hypotheses", "events", "disagreements", "loops", "loop_us"), list(out)))
    t = (C.c_long * 4)()
    lib().modsx_verify_device_timing(t, int(bool(reset)))
    d.update(zip(("draw_us", "device_wait_us", "host_phase_us", "event_body_us"), list(t)))
    return d


class RegionClass(C.Structure):
    _fields_ = [("det_name", C.c_char_p), ("desc_name", C.c_char_p), ("regs", C.c_void_p), ("desc", C.c_void_p),
                ("n", C.c_int), ("dim", C.c_int), ("stride", C.c_int)]


def save_regions(path, classes):
    """ImageRepresentation::SaveRegions: classes = [(det_name, desc_name, regs (REGION), desc [n, stride] f32, dim)]."""
    arr = (RegionClass * len(classes))()
    keep = []
    for i, (det, dn, regs, desc, dim) in enumerate(classes):
        regs = np.ascontiguousarray(regs, REGION)
        desc = np.ascontiguousarray(desc, np.float32).reshape(len(regs), -1) if len(regs) else np.zeros((0, max(dim, 1)), np.float32)
        keep += [regs, desc]
        arr[i].det_name, arr[i].desc_name = det.encode(), dn.encode()
        arr[i].regs, arr[i].desc = regs.ctypes.data, desc.ctypes.data
        arr[i].n, arr[i].dim, arr[i].stride = len(regs), dim, desc.shape[1]
    _check(lib().modsx_save_regions(path.encode(), arr, len(classes)), "save_regions")


def load_regions(path, det_name="", desc_name=""):
    """ImageRepresentation::LoadRegions for one class: returns (det_name, desc_name, regs, desc [n, dim])."""
    regs, desc = C.c_void_p(), C.c_void_p()
    dim = C.c_int(0)
    fd, fs = C.create_string_buffer(64), C.create_string_buffer(64)
    n = _check(lib().modsx_load_regions(path.encode(), det_name.encode(), desc_name.encode(), C.byref(regs), C.byref(desc),
                                        C.byref(dim), fd, fs), "load_regions")
    r = _take(regs, n, REGION)
    d = _take(desc, n * dim.value, np.dtype(np.float32)).reshape(n, dim.value)
    return fd.value.decode(), fs.value.decode(), r, d


def set_vs_pars(scale_set, tilt_set, phi_base, init_sigma=0.5, do_blur=1, prev=None):
    """SetVSPars (host): returns the new views of this step; `prev` (list of View) is extended in place."""
    prev = [] if prev is None else prev
    ss = np.ascontiguousarray(scale_set, np.float64)
    ts = np.ascontiguousarray(tilt_set, np.float64)
    cap = 4096
    par = (View * cap)()
    pv = (View * cap)(*prev)
    npv = C.c_int(len(prev))
    n = _check(lib().modsx_set_vs_pars(_p(ss), len(ss), _p(ts), len(ts), C.c_double(phi_base), C.c_double(init_sigma),
                                       int(do_blur), par, cap, pv, C.byref(npv), cap), "set_vs_pars")
    del prev[:]
    for i in range(npv.value):
        prev.append(make_view(pv[i].tilt, pv[i].phi, pv[i].zoom, pv[i].InitSigma, pv[i].doBlur))
    return [make_view(par[i].tilt, par[i].phi, par[i].zoom, par[i].InitSigma, par[i].doBlur) for i in range(n)]


# ---- device path -------------------------------------------------------------------------------
class Image(object):
    def __init__(self, ctx, handle, rows, cols):
        self.ctx, self.h, self.rows, self.cols = ctx, handle, rows, cols

    def free(self):
        if self.h:
            lib().modsx_image_free(self.ctx.h, self.h)
            self.h = None

    def update(self, pixels):
        """modsx_image_update: new pixels (u8 or f32, 1 or 3 channels) for this uploaded image, same size, no allocation."""
        a = np.ascontiguousarray(pixels)
        if a.dtype != np.uint8:
            a = np.ascontiguousarray(a, np.float32)
        ch = 1 if a.ndim == 2 else a.shape[2]
        _check(lib().modsx_image_update(C.c_void_p(self.ctx.h), C.c_void_p(self.h), _p(a), a.shape[0], a.shape[1], ch,
                                        0 if a.dtype == np.uint8 else 1), "image_update")

    def download(self):
        out = np.empty((self.rows, self.cols), np.float32)
        _check(lib().modsx_image_download(C.c_void_p(self.ctx.h), C.c_void_p(self.h), _p(out)), "image_download")
        return out


class Db(object):
    """A descriptor database resident in HBM (modsx_db): the background set of MatchFlannFGINNPlusDB."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def rows(self):
        return int(lib().modsx_db_rows(self.h)) if self.h else 0

    def free(self):
        if self.h:
            lib().modsx_db_free(self.ctx.h, self.h)
            self.h = None


def _ladder_steps(steps):
    """(views, match_ratio[, detector[, descs]]) tuples -> (LadderStep array, the view arrays it points into)."""
    arr = (LadderStep * len(steps))()
    keep = []
    for i, st in enumerate(steps):
        va = _view_array(st[0])
        keep.append(va)
        arr[i].views = C.cast(va, C.c_void_p)
        arr[i].nviews = len(st[0])
        arr[i].match_ratio = float(st[1])
        arr[i].detector = int(st[2]) if len(st) > 2 else 0
        if len(st) > 3 and st[3] is not None:
            _set_descs(arr[i], st[3])
    return arr, keep


class Rep(object):
    """A stored image representation (modsx_rep): the regions and descriptors of one image per (detector, descriptor) class,
    resident in HBM with their packed matcher form.  Describe once with add_views / append, match against many with
    match_reps."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.h = lib().modsx_rep_create(ctx.h)
        if not self.h:
            raise RuntimeError("modsx_rep_create failed: " + _err())

    def add_views(self, img, views, params, detector=0, descs=None, ctx=None):
        """One step of SynthDetectDescribeKeypoints + AddRegions; descs = [(descriptor type, ratio), ...] as in match_ladder's
        steps (the ratios are not used here).  Returns the regions added to each class of the step."""
        arr, keep = _ladder_steps([(views, 0.0, detector, descs)])
        return _check(lib().modsx_rep_add_views((ctx or self.ctx).h, self.h, img.h, arr, C.addressof(params)), "rep_add_views")

    def append(self, regs, desc, detector=0, desc_type=1, ctx=None):
        """LoadRegions: regions (REGION records) and their [n][128] descriptors (uint8, or anything convertible to float32)."""
        regs = np.ascontiguousarray(regs, REGION)
        d = np.ascontiguousarray(desc)
        if d.dtype != np.uint8:
            d = np.ascontiguousarray(d, np.float32)
        if d.shape != (len(regs), 128):
            raise ValueError("rep.append: [n][128] descriptors for n regions are expected")
        return _check(lib().modsx_rep_append((ctx or self.ctx).h, self.h, int(detector), int(desc_type), _p(regs), _p(d),
                                             0 if d.dtype == np.uint8 else 1, len(regs)), "rep_append")

    def regions(self, detector=0, desc_type=1, want_desc=True):
        """(regions, [n][128] uint8 descriptors) of one class; want_desc=False: the regions only."""
        regs, desc = C.c_void_p(), C.c_void_p()
        n = _check(lib().modsx_rep_class(self.ctx.h, self.h, int(detector), int(desc_type), C.byref(regs),
                                         C.byref(desc) if want_desc else None), "rep_class")
        r = _take(regs, n, REGION)
        if not want_desc:
            return r
        return r, _take(desc, n * 128, np.dtype(np.uint8)).reshape(n, 128)

    def count(self, detector=0, desc_type=1):
        return _check(lib().modsx_rep_class(self.ctx.h, self.h, int(detector), int(desc_type), None, None), "rep_class")

    # ---- float classes (DESC_CAFFE .. DESC_SURF; detector DET_HESSIAN, DET_MSER or DET_SURF) ----
    def append_f32(self, regs, rows, detector=0, desc_type=DESC_CAFFE, ctx=None):
        """LoadRegions for a float class: regions (REGION records) and their dense [n][dim] float32 rows.  Returns n."""
        regs = np.ascontiguousarray(regs, REGION)
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or len(rows) != len(regs):
            raise ValueError("rep.append_f32: [n][dim] rows for n regions are expected")
        return _check(lib().modsx_rep_append_f32((ctx or self.ctx).h, self.h, int(detector), int(desc_type), _p(regs), _p(rows),
                                                 rows.shape[1], len(regs)), "rep_append_f32")

    def append_f32_device(self, regs, rows_ptr, dim, detector=0, desc_type=DESC_CAFFE, ctx=None):
        """append_f32 with the dense [n][dim] float32 rows in HBM (a 4-byte aligned device pointer).  Returns n."""
        regs = np.ascontiguousarray(regs, REGION)
        return _check(lib().modsx_rep_append_f32_device((ctx or self.ctx).h, self.h, int(detector), int(desc_type), _p(regs),
                                                        C.c_void_p(rows_ptr), int(dim), len(regs)), "rep_append_f32_device")

    def describe_append(self, img, regs, detector=0, desc_type=DESC_SURF, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1,
                        daisy_par=None, ctx=None):
        """Describes the (oriented) regions of one view image with the class's extractor (DESC_SURF, DESC_LIOP, DESC_DAISY) and
        appends regions and rows; daisy_par = (rad, radq, thq, histq, nrm_type) for DAISY.  Returns n."""
        regs = np.ascontiguousarray(regs, REGION)
        dp = None if daisy_par is None else np.ascontiguousarray(daisy_par, np.int32)
        if dp is not None and dp.shape != (5,):
            raise ValueError("rep.describe_append: daisy_par = (rad, radq, thq, histq, nrm_type)")
        return _check(lib().modsx_rep_describe_append((ctx or self.ctx).h, self.h, int(detector), int(desc_type), C.c_void_p(img.h),
                                                      _p(regs), len(regs), C.c_double(mr_size), int(patch_size), int(fast),
                                                      int(photo_norm), None if dp is None else _p(dp)), "rep_describe_append")

    def class_f32(self, detector=0, desc_type=DESC_CAFFE):
        """(regions, dense [n][dim] float32 rows) of one float class; dim = 0 while the class is empty."""
        regs, rows, dim = C.c_void_p(), C.c_void_p(), C.c_int(0)
        n = _check(lib().modsx_rep_class_f32(self.ctx.h, self.h, int(detector), int(desc_type), C.byref(regs), C.byref(rows),
                                             C.byref(dim)), "rep_class_f32")
        return _take(regs, n, REGION), _take(rows, n * dim.value, np.dtype(np.float32)).reshape(n, dim.value)

    def count_f32(self, detector=0, desc_type=DESC_CAFFE):
        return _check(lib().modsx_rep_class_f32(self.ctx.h, self.h, int(detector), int(desc_type), None, None, None), "rep_class_f32")

    # ---- binary classes (DESC_BRISK, DESC_FREAK, DESC_ORB; detector DET_HESSIAN, DET_MSER, DET_ORB or DET_SURF) ----
    def append_bin(self, regs, rows, detector=DET_ORB, desc_type=DESC_ORB, ctx=None, dtype=None):
        """LoadRegions for a binary class: regions (REGION records) and their dense [n][nbytes] rows (uint8, or anything convertible
        to float32 holding the integers 0..255).  dtype overrides the dtype code handed to the library.  Returns n."""
        regs = np.ascontiguousarray(regs, REGION)
        d = np.ascontiguousarray(rows)
        if d.dtype != np.uint8:
            d = np.ascontiguousarray(d, np.float32)
        if d.ndim != 2 or len(d) != len(regs):
            raise ValueError("rep.append_bin: [n][nbytes] rows for n regions are expected")
        code = (0 if d.dtype == np.uint8 else 1) if dtype is None else int(dtype)
        return _check(lib().modsx_rep_append_bin((ctx or self.ctx).h, self.h, int(detector), int(desc_type), _p(regs), _p(d),
                                                 d.shape[1], code, len(regs)), "rep_append_bin")

    def append_bin_device(self, regs, dev_ptr, nbytes, detector=DET_ORB, desc_type=DESC_ORB, ctx=None):
        """The same from dense [n][nbytes] uint8 rows in HBM at address dev_ptr (any alignment); the regions come from the host."""
        regs = np.ascontiguousarray(regs, REGION)
        return _check(lib().modsx_rep_append_bin_device((ctx or self.ctx).h, self.h, int(detector), int(desc_type), _p(regs),
                                                        C.c_void_p(dev_ptr), int(nbytes), len(regs)), "rep_append_bin_device")

    def regions_bin(self, detector=DET_ORB, desc_type=DESC_ORB, want_desc=True):
        """(regions, dense [n][nbytes] uint8 rows) of one binary class, nbytes = 0 while it is empty; want_desc=False: the regions."""
        regs, rows, nb = C.c_void_p(), C.c_void_p(), C.c_int(0)
        n = _check(lib().modsx_rep_class_bin(self.ctx.h, self.h, int(detector), int(desc_type), C.byref(regs),
                                             C.byref(rows) if want_desc else None, C.byref(nb)), "rep_class_bin")
        r = _take(regs, n, REGION)
        if not want_desc:
            return r
        return r, _take(rows, n * nb.value, np.dtype(np.uint8)).reshape(n, nb.value)

    def count_bin(self, detector=DET_ORB, desc_type=DESC_ORB):
        return _check(lib().modsx_rep_class_bin(self.ctx.h, self.h, int(detector), int(desc_type), None, None, None), "rep_class_bin")

    def free(self):
        if self.h:
            lib().modsx_rep_free(self.ctx.h, self.h)
            self.h = None


class Context(object):
    """One modsx_ctx (one HIP stream).  Raises if no gfx950 device is available."""

    def __init__(self, device=0):
        self.device = int(device)
        self.h = lib().modsx_create(int(device))
        if not self.h:
            raise RuntimeError("modsx_create failed: " + _err())

    def close(self):
        if self.h:
            lib().modsx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self):
        return C.c_void_p(self.h)

    def upload(self, pixels):
        a = np.ascontiguousarray(pixels)
        if a.dtype == np.uint8:
            dtype = 0
        else:
            a = np.ascontiguousarray(a, np.float32)
            dtype = 1
        ch = 1 if a.ndim == 2 else a.shape[2]
        h = lib().modsx_image_upload(self._c(), _p(a), a.shape[0], a.shape[1], ch, dtype)
        if not h:
            raise RuntimeError("modsx_image_upload failed: " + _err())
        return Image(self, h, a.shape[0], a.shape[1])

    def wrap_device(self, dev_ptr, rows, cols):
        h = lib().modsx_image_wrap_device(self._c(), C.c_void_p(dev_ptr), rows, cols)
        if not h:
            raise RuntimeError("modsx_image_wrap_device failed: " + _err())
        return Image(self, h, rows, cols)

    def synchronize(self):
        _check(lib().modsx_synchronize(self._c()), "synchronize")

    def gaussian_blur(self, img, sigma):
        out = np.empty((img.rows, img.cols), np.float32)
        _check(lib().modsx_gaussian_blur(self._c(), C.c_void_p(img.h), C.c_float(sigma), _p(out)), "gaussian_blur")
        return out

    def response(self, img, detector_type, norm):
        out = np.zeros((img.rows, img.cols), np.float32)
        _check(lib().modsx_response(self._c(), C.c_void_p(img.h), int(detector_type), C.c_float(norm), _p(out)), "response")
        return out

    def resize_half(self, img):
        r, c = C.c_int(), C.c_int()
        _check(lib().modsx_resize_half(self._c(), C.c_void_p(img.h), None, C.byref(r), C.byref(c)), "resize_half")
        out = np.empty((r.value, c.value), np.float32)
        _check(lib().modsx_resize_half(self._c(), C.c_void_p(img.h), _p(out), C.byref(r), C.byref(c)), "resize_half")
        return out

    def octave_levels(self, img, params):
        L = params.numberOfScales + 2
        blurs = np.empty((L, img.rows, img.cols), np.float32)
        resps = np.empty((L, img.rows, img.cols), np.float32)
        _check(lib().modsx_octave_levels(self._c(), C.c_void_p(img.h), C.byref(params), _p(blurs), _p(resps)),
               "octave_levels")
        return blurs, resps

    def detect_scalespace(self, img, params):
        out = C.c_void_p()
        n = _check(lib().modsx_detect_scalespace(self._c(), C.c_void_p(img.h), C.byref(params), C.byref(out)),
                   "detect_scalespace")
        return _take(out, n, SSKP)

    def detect_affine_keypoints(self, img, params, tilt=1.0, zoom=1.0):
        out = C.c_void_p()
        n = _check(lib().modsx_detect_affine_keypoints(self._c(), C.c_void_p(img.h), C.byref(params),
                                                       C.c_double(tilt), C.c_double(zoom), C.byref(out)),
                   "detect_affine_keypoints")
        return _take(out, n, KEYPOINT)

    def debug_baumberg(self, planes, plane_of, xyspd, params, variant=0, chunk=0):
        """modsx_debug_baumberg: one Baumberg launch for a job list (planes: Images of this context; plane_of[k], xyspd[k] = x, y,
        s, pixelDistance of job k).  -> dict(u [n, 4] f32, ok, iters, geometry, handed_out): geometry as baumberg_geometry() gives
        it, handed_out the keypoints the queue's counters handed out (variant 3; 0 otherwise)."""
        plane_of = np.ascontiguousarray(plane_of, np.int32)
        xyspd = np.ascontiguousarray(xyspd, np.float32).reshape(-1, 4)
        n = len(plane_of)
        assert len(xyspd) == n
        ptrs = (C.c_void_p * max(1, len(planes)))(*[im.h for im in planes])
        u = np.zeros((max(n, 1), 4), np.float32)
        ok, iters = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        geo = np.zeros(4, np.int32)
        handed = C.c_int(0)
        _check(lib().modsx_debug_baumberg(self._c(), ptrs, len(planes), _p(plane_of), _p(xyspd), n, C.byref(params), int(variant),
                                          int(chunk), _p(u), _p(ok), _p(iters), _p(geo), C.byref(handed)), "debug_baumberg")
        return dict(u=u[:n], ok=ok[:n], iters=iters[:n], geometry=dict(zip(BAUMBERG_GEOMETRY, (int(x) for x in geo))),
                    handed_out=handed.value)

    def baumberg_geometry(self, n, W=19, variant=0, chunk=0):
        """baumberg_geometry() as this context launches: the production rule of the queue form (variant 3, chunk 0) is one resident
        set of wavefronts of the context's device, which the module-level function cannot know."""
        geo = np.zeros(4, np.int32)
        _check(lib().modsx_debug_baumberg_geometry_ctx(self._c(), int(n), int(W), int(variant), int(chunk), _p(geo)), "baumberg_geometry")
        return dict(zip(BAUMBERG_GEOMETRY, (int(x) for x in geo)))

    def detect_orientation(self, img, regs, mr_size=1.0, patch_size=41, half=0, max_ang=1, th=0.8, upright=0):
        regs = np.ascontiguousarray(regs, REGION)
        out = C.c_void_p()
        n = _check(lib().modsx_detect_orientation(self._c(), C.c_void_p(img.h), _p(regs), len(regs),
                                                  C.c_double(mr_size), patch_size, half, max_ang, C.c_double(th),
                                                  upright, C.byref(out)), "detect_orientation")
        return _take(out, n, REGION)

    def describe_regions(self, img, regs, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1, desc_type=1,
                         max_bin=0.2):
        regs = np.ascontiguousarray(regs, REGION)
        desc = np.zeros((len(regs), 128), np.float32)
        _check(lib().modsx_describe_regions(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size),
                                            patch_size, fast, photo_norm, desc_type, C.c_double(max_bin), _p(desc)),
               "describe_regions")
        return desc

    # ---- normalised patches and LIOP (engine_liop.hip) ----
    def extract_patches(self, img, regs, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1, out_ptr=None):
        """The patches DescribeRegions<> hands to its functor: [n][41][41] float32.  out_ptr: a device pointer that receives them
        instead (4-byte aligned, n * 1681 floats); the call then returns None."""
        regs = np.ascontiguousarray(regs, REGION)
        if out_ptr is not None:
            _check(lib().modsx_extract_patches_device(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size),
                                                      int(patch_size), int(fast), int(photo_norm), C.c_void_p(out_ptr)),
                   "extract_patches_device")
            return None
        out = np.zeros((len(regs), 41, 41), np.float32)
        _check(lib().modsx_extract_patches(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size), int(patch_size),
                                           int(fast), int(photo_norm), _p(out)), "extract_patches")
        return out

    def liop_patches(self, patches, patch_size=41):
        """vl_liopdesc_process on [n][41][41] float32 patches (finite values) -> [n][144] float32."""
        patches = _patch_rows(patches)
        desc = np.zeros((len(patches), LIOP_DIM), np.float32)
        _check(lib().modsx_liop_patches(self._c(), _p(patches), len(patches), int(patch_size), _p(desc)), "liop_patches")
        return desc

    def liop_patches_device(self, patches_ptr, n, desc_ptr, patch_size=41):
        """The same on dense [n][1681] float32 rows in HBM -> [n][144] float32 rows in HBM (device pointers, 4-byte aligned)."""
        _check(lib().modsx_liop_patches_device(self._c(), C.c_void_p(patches_ptr), int(n), int(patch_size), C.c_void_p(desc_ptr)),
               "liop_patches_device")

    def describe_regions_liop(self, img, regs, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1, out_ptr=None):
        """DescribeRegions<LIOPDescriptor>: [n][144] float32 (out_ptr: into that device pointer instead, returns None)."""
        regs = np.ascontiguousarray(regs, REGION)
        if out_ptr is not None:
            _check(lib().modsx_describe_regions_liop_device(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size),
                                                            int(patch_size), int(fast), int(photo_norm), C.c_void_p(out_ptr)),
                   "describe_regions_liop_device")
            return None
        desc = np.zeros((len(regs), LIOP_DIM), np.float32)
        _check(lib().modsx_describe_regions_liop(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size),
                                                 int(patch_size), int(fast), int(photo_norm), _p(desc)), "describe_regions_liop")
        return desc

    def debug_liop(self, patches, patch_size=41):
        """dict(desc [n][144], path [n] (0: no tie group across a bin cut, 1: the reference's quicksort was replayed), perm [n][673]
        = measurement pixel of every rank, the permutation the spatial bins were cut from)."""
        patches = _patch_rows(patches)
        n = len(patches)
        desc = np.zeros((n, LIOP_DIM), np.float32)
        path, perm = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), LIOP_PIXELS), np.int32)
        _check(lib().modsx_debug_liop(self._c(), _p(patches), n, int(patch_size), _p(desc), _p(path), _p(perm)), "debug_liop")
        return dict(desc=desc, path=path[:n], perm=perm[:n])

    # ---- SURF (engine_surf.hip) ----
    def surf_patches(self, patches, mr_size=5.1962, patch_size=41):
        """The SURF functor (OpenSURF U-SURF-64 of the fixed point of scale patch_size / mr_size) on [n][41][41] float32 patches
        (finite values) -> [n][64] float32; a row of NaN where every response is zero."""
        patches = _patch_rows(patches)
        desc = np.zeros((len(patches), SURF_DIM), np.float32)
        _check(lib().modsx_surf_patches(self._c(), _p(patches), len(patches), int(patch_size), C.c_double(mr_size), _p(desc)),
               "surf_patches")
        return desc

    def surf_patches_device(self, patches_ptr, n, desc_ptr, mr_size=5.1962, patch_size=41):
        """surf_patches from a device pointer to [n][1681] float32 into a device pointer to [n][64] float32 (4-byte aligned)."""
        _check(lib().modsx_surf_patches_device(self._c(), C.c_void_p(patches_ptr), int(n), int(patch_size), C.c_double(mr_size),
                                               C.c_void_p(desc_ptr)), "surf_patches_device")

    def describe_regions_surf(self, img, regs, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1, out_ptr=None):
        """DescribeRegions<SURFDescriptor>: [n][64] float32 (out_ptr: into that device pointer instead, returns None).  mr_size
        sets the measurement window and the scale of the described point, as in the reference."""
        regs = np.ascontiguousarray(regs, REGION)
        if out_ptr is not None:
            _check(lib().modsx_describe_regions_surf_device(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size),
                                                            int(patch_size), int(fast), int(photo_norm), C.c_void_p(out_ptr)),
                   "describe_regions_surf_device")
            return None
        desc = np.zeros((len(regs), SURF_DIM), np.float32)
        _check(lib().modsx_describe_regions_surf(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size),
                                                 int(patch_size), int(fast), int(photo_norm), _p(desc)), "describe_regions_surf")
        return desc

    def describe_regions_surf_device(self, img, regs, out_ptr, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1):
        """describe_regions_surf into a device pointer to [n][64] float32 (4-byte aligned)."""
        return self.describe_regions_surf(img, regs, mr_size, patch_size, fast, photo_norm, out_ptr=out_ptr)

    # ---- the SURF detector (engine_surfdet.hip) ----
    def detect_surf(self, img, params=None):
        """OpenSURF's FastHessian on the image: KEYPOINT records in the reference's push order (x, y, s and the frame of
        orientation 0)."""
        params = params or surfdet_params()
        out = C.c_void_p()
        n = _check(lib().modsx_detect_surf(self._c(), C.c_void_p(img.h), C.byref(params), C.byref(out)), "detect_surf")
        return _take(out, n, KEYPOINT)

    def detect_surf_batch(self, imgs, params=None):
        """detect_surf of several images (any sizes) with shared launches: a list of KEYPOINT arrays."""
        params = params or surfdet_params()
        ptrs = (C.c_void_p * max(1, len(imgs)))(*[im.h for im in imgs])
        counts = np.zeros(max(1, len(imgs)), np.int32)
        out = C.c_void_p()
        n = _check(lib().modsx_detect_surf_batch(self._c(), ptrs, len(imgs), C.byref(params), C.byref(out), _p(counts)),
                   "detect_surf_batch")
        allk = _take(out, n, KEYPOINT)
        ends = np.cumsum(counts[:len(imgs)])
        return [allk[e - k:e].copy() for e, k in zip(ends, counts[:len(imgs)])]

    def debug_surfdet(self, img, params=None):
        """modsx_debug_surfdet: dict(layers [n][4], integral, resp / lap: lists of planes, extrema [m][4] (o, i, r, c), dD [m][3],
        H [m][6], x [m][3], accepted [m], laplacian [m]) -- the stages of detect_surf for one image."""
        params = params or surfdet_params()
        layers = surfdet_geometry(img.rows, img.cols, params)
        sizes = layers[:, 0].astype(np.int64) * layers[:, 1]
        integral = np.zeros((img.rows, img.cols), np.float32)
        resp, lap = np.zeros(int(sizes.sum()), np.float32), np.zeros(int(sizes.sum()), np.uint8)
        lay = np.zeros((SURFDET_MAX_LAYERS, 4), np.int32)
        cap = 4096
        while True:
            ext, dD, H, x = np.zeros((cap, 4), np.int32), np.zeros((cap, 3)), np.zeros((cap, 6)), np.zeros((cap, 3))
            acc, lp = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            n_ext = C.c_int(0)
            nl = _check(lib().modsx_debug_surfdet(self._c(), C.c_void_p(img.h), C.byref(params), _p(integral), _p(lay), _p(resp), _p(lap),
                                                  _p(ext), _p(dD), _p(H), _p(x), _p(acc), _p(lp), cap, C.byref(n_ext)), "debug_surfdet")
            if n_ext.value <= cap:
                break
            cap = n_ext.value
        assert nl == len(layers) and np.array_equal(lay[:nl], layers)
        m, ofs = n_ext.value, np.concatenate([[0], np.cumsum(sizes)])
        plane = lambda a, k: a[ofs[k]:ofs[k + 1]].reshape(layers[k, 1], layers[k, 0])      # noqa: E731
        return dict(layers=layers, integral=integral, resp=[plane(resp, k) for k in range(nl)], lap=[plane(lap, k) for k in range(nl)],
                    extrema=ext[:m], dD=dD[:m], H=H[:m], x=x[:m], accepted=acc[:m].astype(bool), laplacian=lp[:m])

    # ---- the KAZE detector (engine_kaze.hip) ----
    def detect_kaze(self, img, params=None):
        """AKAZE's nonlinear scale space and Hessian extrema on the image: KEYPOINT records in the reference's order (x, y, s =
        size / 3, response, octave_number and the frame of orientation 0)."""
        params = params or kaze_params()
        out = C.c_void_p()
        n = _check(lib().modsx_detect_kaze(self._c(), C.c_void_p(img.h), C.byref(params), C.byref(out)), "detect_kaze")
        return _take(out, n, KEYPOINT)

    def detect_kaze_batch(self, imgs, params=None):
        """detect_kaze of several images (any sizes) with shared launches: a list of KEYPOINT arrays."""
        params = params or kaze_params()
        ptrs = (C.c_void_p * max(1, len(imgs)))(*[im.h for im in imgs])
        counts = np.zeros(max(1, len(imgs)), np.int32)
        out = C.c_void_p()
        n = _check(lib().modsx_detect_kaze_batch(self._c(), ptrs, len(imgs), C.byref(params), C.byref(out), _p(counts)),
                   "detect_kaze_batch")
        allk = _take(out, n, KEYPOINT)
        ends = np.cumsum(counts[:len(imgs)])
        return [allk[e - k:e].copy() for e, k in zip(ends, counts[:len(imgs)])]

    @staticmethod
    def _kaze_lists(call, cap=4096):
        while True:
            raw, rawv = np.zeros((cap, 3), np.int32), np.zeros(cap, np.float32)
            aux, upper, fin = (np.zeros(cap, KAZE_POINT) for _ in range(3))
            counts = np.zeros(4, np.int32)
            nl = call(_p(raw), _p(rawv), _p(aux), _p(upper), _p(fin), cap, _p(counts))
            if counts.max() <= cap:
                break
            cap = int(counts.max())
        n = [int(v) for v in counts]
        return nl, dict(raw=raw[:n[0]].copy(), rawv=rawv[:n[0]].copy(), aux=aux[:n[1]].copy(), upper=upper[:n[2]].copy(),
                        final=fin[:n[3]].copy())

    def debug_kaze(self, img, params=None):
        """modsx_debug_kaze: dict(geometry, kcontrast, hmax, hist, Lt / Lsmooth / Lflow / Ldet: lists of planes, raw [m][3] (level,
        row, col), rawv [m], aux, upper, final: KAZE_POINT arrays) -- the stages of detect_kaze for one image."""
        params = params or kaze_params()
        geo = kaze_geometry(img.rows, img.cols, params)
        lv = geo["levels"]
        sizes = lv[:, 2].astype(np.int64) * lv[:, 3]
        kc, hist = np.zeros(2, np.float32), np.zeros(params.kcontrast_nbins, np.int64)
        planes = [np.zeros(int(sizes.sum()), np.float32) for _ in range(4)]
        nl, out = self._kaze_lists(lambda *a: _check(lib().modsx_debug_kaze(self._c(), C.c_void_p(img.h), C.byref(params), _p(kc), _p(hist),
                                                                             *[_p(a_) for a_ in planes], *a), "debug_kaze"))
        assert nl == len(lv)
        ofs = np.concatenate([[0], np.cumsum(sizes)])
        for name, a in zip(("Lt", "Lsmooth", "Lflow", "Ldet"), planes):
            out[name] = [a[ofs[k]:ofs[k + 1]].reshape(lv[k, 2], lv[k, 3]) for k in range(nl)]
        out.update(geometry=geo, kcontrast=kc[0], hmax=kc[1], hist=hist)
        return out

    def debug_kaze_scan(self, rows, cols, planes, params=None):
        """modsx_debug_kaze_scan: the extrema scan, both filter passes and the refinement on the given Ldet planes (one per level
        of a rows x cols image): dict(raw, rawv, aux, upper, final)."""
        params = params or kaze_params()
        lv = kaze_geometry(rows, cols, params)["levels"]
        if len(planes) != len(lv) or any(np.shape(a) != (L[2], L[3]) for a, L in zip(planes, lv)):
            raise ValueError("debug_kaze_scan: one plane per level, of the level's size")
        flat = np.concatenate([np.ascontiguousarray(a, np.float32).reshape(-1) for a in planes])
        nl, out = self._kaze_lists(lambda *a: _check(lib().modsx_debug_kaze_scan(self._c(), int(rows), int(cols), C.byref(params), _p(flat),
                                                                                  *a), "debug_kaze_scan"))
        assert nl == len(lv)
        return out

    def kaze_counters(self):
        """dict of KAZE_COUNTERS: KAZE detector work of this context since it was created (cumulative)."""
        return self._counters("modsx_kaze_counters", KAZE_COUNTERS)

    # ---- external affine adaptation (engine_detect.hip: DetectAffineShape) ----
    def detect_affine_shape(self, img, regs, params=None):
        """DetectAffineShape on a finished region list: the regions whose Baumberg iteration on the image converges, in input
        order, det_kp.a11 .. a22 replaced by the shape found (every other field as given)."""
        params = params or default_affshape_params()
        regs = np.ascontiguousarray(regs, REGION)
        out = C.c_void_p()
        n = _check(lib().modsx_detect_affine_shape(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.byref(params), C.byref(out)),
                   "detect_affine_shape")
        return _take(out, n, REGION)

    @staticmethod
    def _affshape_lists(imgs, regs):
        assert len(imgs) == len(regs)
        regs = [np.ascontiguousarray(r, REGION) for r in regs]
        ptrs = (C.c_void_p * max(1, len(imgs)))(*[im.h for im in imgs])
        counts = np.array([len(r) for r in regs] + [0], np.int32)
        flat = np.concatenate(regs + [np.zeros(0, REGION)]) if regs else np.zeros(0, REGION)
        return ptrs, counts, np.ascontiguousarray(flat, REGION)

    def detect_affine_shape_batch(self, imgs, regs, params=None):
        """detect_affine_shape of several images (any sizes; regs: one REGION array per image) in one launch: a list of REGION arrays."""
        params = params or default_affshape_params()
        ptrs, counts, flat = self._affshape_lists(imgs, regs)
        out_counts = np.zeros(len(imgs) + 1, np.int32)
        out = C.c_void_p()
        n = _check(lib().modsx_detect_affine_shape_batch(self._c(), ptrs, len(imgs), _p(flat), _p(counts), C.byref(params), C.byref(out),
                                                         _p(out_counts)), "detect_affine_shape_batch")
        allr = _take(out, n, REGION)
        ends = np.cumsum(out_counts[:len(imgs)])
        return [allr[e - k:e].copy() for e, k in zip(ends, out_counts[:len(imgs)])]

    def debug_affine_shape(self, imgs, regs, params=None, variant=-1):
        """modsx_debug_affine_shape: the launch of detect_affine_shape_batch reported per INPUT region (image 0's, then image 1's,
        ...) -> dict(border bool [n], u [n, 4] f32, ok, iters (-1 for a border-refused region), geometry, launched).  variant -1 =
        the production rule, 0..3 as baumberg_geometry."""
        params = params or default_affshape_params()
        ptrs, counts, flat = self._affshape_lists(imgs, regs)
        n = len(flat)
        border, u = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 4), np.float32)
        ok, iters, geo = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(4, np.int32)
        launched = _check(lib().modsx_debug_affine_shape(self._c(), ptrs, len(imgs), _p(flat), _p(counts), C.byref(params), int(variant),
                                                         _p(border), _p(u), _p(ok), _p(iters), _p(geo)), "debug_affine_shape")
        return dict(border=border[:n].astype(bool), u=u[:n], ok=ok[:n], iters=iters[:n],
                    geometry=dict(zip(BAUMBERG_GEOMETRY, (int(x) for x in geo))), launched=launched)

    def affshape_counters(self):
        """dict of AFFSHAPE_COUNTERS: external affine adaptation work of this context since it was created (cumulative)."""
        return self._counters("modsx_affshape_counters", AFFSHAPE_COUNTERS)

    # ---- CLAHE (engine_clahe.hip: the drivers' doCLAHE step) ----
    def clahe(self, img, clip_limit=4.0, tiles=(8, 8), variant=0, out=None):
        """cv::CLAHE::apply (clip 4, 8 x 8 as the drivers set it) on an uploaded image: a new Image, or `out` (same size; may be
        img itself) filled and returned.  The result holds the integers 0..255 as f32."""
        par = clahe_params(clip_limit, tiles, variant)
        if out is None:
            h = lib().modsx_image_clahe_new(self._c(), C.c_void_p(img.h), C.byref(par))
            if not h:
                raise RuntimeError("clahe failed: " + _err())
            return Image(self, h, img.rows, img.cols)
        _check(lib().modsx_image_clahe(self._c(), C.c_void_p(img.h), C.byref(par), C.c_void_p(out.h)), "clahe")
        return out

    def clahe_batch(self, imgs, clip_limit=4.0, tiles=(8, 8), variant=0, out=None):
        """clahe of several images of any sizes in ONE launch set (three launches): out[i] (default: imgs[i], in place) is
        filled; returns the list of outputs."""
        out = list(imgs) if out is None else list(out)
        assert len(out) == len(imgs)
        n = len(imgs)
        src = (C.c_void_p * max(1, n))(*[im.h for im in imgs])
        dst = (C.c_void_p * max(1, n))(*[im.h for im in out])
        _check(lib().modsx_image_clahe_batch(self._c(), src, dst, n, C.byref(clahe_params(clip_limit, tiles, variant))), "clahe_batch")
        return out

    def debug_clahe(self, img, clip_limit=4.0, tiles=(8, 8), variant=0):
        """modsx_debug_clahe -> dict(hist [tiles][256] int32: the counts of every tile before clipping, lut [tiles][256] uint8),
        tiles in row-major order."""
        nt = int(tiles[0]) * int(tiles[1])
        hist, lut = np.zeros((max(nt, 1), 256), np.int32), np.zeros((max(nt, 1), 256), np.uint8)
        _check(lib().modsx_debug_clahe(self._c(), C.c_void_p(img.h), C.byref(clahe_params(clip_limit, tiles, variant)), _p(hist), _p(lut)),
               "debug_clahe")
        return dict(hist=hist, lut=lut)

    def clahe_last_ms(self):
        """(hist, lut, apply) HIP-event times in ms of the last clahe / clahe_batch / debug_clahe launches of this context, recorded
        while profile(True) is on (zeros before)."""
        ms = np.zeros(3, np.float64)
        _check(lib().modsx_debug_clahe_last_ms(self._c(), _p(ms)), "clahe_last_ms")
        return tuple(float(x) for x in ms)

    def clahe_counters(self):
        """dict of CLAHE_COUNTERS: CLAHE work of this context since it was created (cumulative)."""
        return self._counters("modsx_clahe_counters", CLAHE_COUNTERS)

    # ---- the learned-descriptor front end (engine_caffe.hip: the reference's "CAFFE" branch around its network) ----
    def caffe_patches(self, planes, regs, par=None, out_ptr=None, want_flags=False):
        """The network's input blob for the regions' reproj_kp on the ORIGINAL image: [n][3][P][P] float32, byte - mean.  planes:
        one Image (gray) or three (B, G, R).  out_ptr: a device pointer that receives the blob instead (4-byte aligned); the blob
        returned is then None.  want_flags: return (blob, flags [n] uint8: bit 0 border branch, bit 1 a sample outside)."""
        planes = [planes] if isinstance(planes, Image) else list(planes)
        par = par or caffe_params()
        regs = np.ascontiguousarray(regs, REGION)
        n, P = len(regs), par.patchSize
        hs = (C.c_void_p * max(len(planes), 1))(*[im.h for im in planes])
        flags = np.zeros(max(n, 1), np.uint8)
        fp = _p(flags) if want_flags else None
        blob = None
        if out_ptr is not None:
            _check(lib().modsx_caffe_patches_device(self._c(), hs, len(planes), _p(regs), n, C.byref(par), C.c_void_p(out_ptr), fp),
                   "caffe_patches_device")
        else:
            blob = np.zeros((n, 3, max(P, 0), max(P, 0)), np.float32)
            buf = blob if blob.size else np.zeros(1, np.float32)
            _check(lib().modsx_caffe_patches(self._c(), hs, len(planes), _p(regs), n, C.byref(par), _p(buf), fp), "caffe_patches")
        return (blob, flags[:n]) if want_flags else blob

    def caffe_norm_rows(self, rows, norm=CAFFE_NORM_L2):
        """L2normalize / L1normalize / RootNormalize / a copy (CAFFE_NORM_*) of [n][dim] float32 rows -> [n][dim] float32."""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2:
            raise ValueError("caffe_norm_rows: [n][dim] rows are expected")
        out = np.zeros(rows.shape, np.float32)
        a, b = (rows, out) if rows.size else (np.zeros(1, np.float32),) * 2
        _check(lib().modsx_caffe_norm_rows(self._c(), _p(a), rows.shape[0], rows.shape[1], int(norm), _p(b)), "caffe_norm_rows")
        return out

    def caffe_norm_rows_device(self, rows_ptr, n, dim, norm=CAFFE_NORM_L2, out_ptr=None):
        """the same on dense [n][dim] float32 rows in HBM (4-byte aligned); out_ptr = None: in place"""
        _check(lib().modsx_caffe_norm_rows_device(self._c(), C.c_void_p(rows_ptr), int(n), int(dim), int(norm),
                                                  C.c_void_p(rows_ptr if out_ptr is None else out_ptr)), "caffe_norm_rows_device")

    def caffe_counters(self):
        """dict of CAFFE_COUNTERS: front-end work of this context since it was created (cumulative)."""
        return self._counters("modsx_caffe_counters", CAFFE_COUNTERS)

    def surfdet_counters(self):
        """dict of SURFDET_COUNTERS: SURF detector work of this context since it was created (cumulative)."""
        return self._counters("modsx_surfdet_counters", SURFDET_COUNTERS)

    def _counters(self, fn_name, names):
        v = (C.c_long * len(names))()
        n = _check(getattr(lib(), fn_name)(self._c(), v, len(names)), fn_name[len("modsx_"):])
        assert n == len(names), n
        return dict(zip(names, (int(x) for x in v)))

    def surf_counters(self):
        """dict of SURF_COUNTERS: SURF work of this context since it was created (cumulative)."""
        return self._counters("modsx_surf_counters", SURF_COUNTERS)

    # ---- DAISY (engine_daisy.hip) ----
    def daisy_patches(self, patches, rad=15, radq=3, thq=8, histq=8, nrm_type=0, patch_size=41):
        """The DAISY functor (libdaisy's descriptor of the patch centre at orientation 0) on [n][41][41] float32 patches ->
        [n][(radq * thq + 1) * 8] float32.  nrm_type: 0 partial, 1 full, 2 sift."""
        patches = _patch_rows(patches)
        desc = np.zeros((len(patches), (int(radq) * int(thq) + 1) * int(histq)), np.float32)
        _check(lib().modsx_daisy_patches(self._c(), _p(patches), len(patches), int(patch_size), int(rad), int(radq), int(thq), int(histq),
                                         int(nrm_type), _p(desc)), "daisy_patches")
        return desc

    def daisy_patches_device(self, patches_ptr, n, desc_ptr, rad=15, radq=3, thq=8, histq=8, nrm_type=0, patch_size=41):
        """daisy_patches from a device pointer to [n][1681] float32 into a device pointer to [n][dim] float32 (4-byte aligned)."""
        _check(lib().modsx_daisy_patches_device(self._c(), C.c_void_p(patches_ptr), int(n), int(patch_size), int(rad), int(radq), int(thq),
                                                int(histq), int(nrm_type), C.c_void_p(desc_ptr)), "daisy_patches_device")

    def describe_regions_daisy(self, img, regs, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1, rad=15, radq=3, thq=8, histq=8,
                               nrm_type=0, out_ptr=None):
        """DescribeRegions<DAISYDescriptor>: [n][(radq * thq + 1) * 8] float32 (out_ptr: into that device pointer instead, returns
        None).  mr_size only sets the measurement window."""
        regs = np.ascontiguousarray(regs, REGION)
        args = (int(patch_size), int(fast), int(photo_norm), int(rad), int(radq), int(thq), int(histq), int(nrm_type))
        if out_ptr is not None:
            _check(lib().modsx_describe_regions_daisy_device(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size), *args,
                                                             C.c_void_p(out_ptr)), "describe_regions_daisy_device")
            return None
        desc = np.zeros((len(regs), (int(radq) * int(thq) + 1) * int(histq)), np.float32)
        _check(lib().modsx_describe_regions_daisy(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size), *args, _p(desc)),
               "describe_regions_daisy")
        return desc

    def describe_regions_daisy_device(self, img, regs, out_ptr, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1, rad=15, radq=3,
                                      thq=8, histq=8, nrm_type=0):
        """describe_regions_daisy into a device pointer to [n][dim] float32 (4-byte aligned)."""
        return self.describe_regions_daisy(img, regs, mr_size, patch_size, fast, photo_norm, rad, radq, thq, histq, nrm_type,
                                           out_ptr=out_ptr)

    def daisy_counters(self):
        """dict of DAISY_COUNTERS: DAISY work of this context since it was created (cumulative)."""
        return self._counters("modsx_daisy_counters", DAISY_COUNTERS)

    def liop_counters(self):
        """dict of LIOP_COUNTERS: LIOP work of this context since it was created (cumulative)."""
        return self._counters("modsx_liop_counters", LIOP_COUNTERS)

    # ---- raw SIFT histograms, the f32 SIFT norm and DSP-SIFT (engine_dsp.hip) ----
    def describe_regions_raw(self, img, regs, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1, out_ptr=None):
        """DescribeRegions<SIFTDescriptor{doNorm = false}>: the raw histograms, [n][128] float32 (out_ptr: into that device
        pointer instead, 4-byte aligned; returns None)."""
        regs = np.ascontiguousarray(regs, REGION)
        if out_ptr is not None:
            _check(lib().modsx_describe_regions_raw_device(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size),
                                                           int(patch_size), int(fast), int(photo_norm), C.c_void_p(out_ptr)),
                   "describe_regions_raw_device")
            return None
        hist = np.zeros((len(regs), 128), np.float32)
        _check(lib().modsx_describe_regions_raw(self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size),
                                                int(patch_size), int(fast), int(photo_norm), _p(hist)), "describe_regions_raw")
        return hist

    def sift_norm_rows(self, rows, max_bin=0.2):
        """SIFTnorm(std::vector<float>&) on [n][128] float32 rows (finite values) -> [n][128] float32 holding 0..255."""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[1] != 128:
            raise ValueError("SIFT rows are [n][128] float32")
        out = np.zeros(rows.shape, np.float32)
        _check(lib().modsx_sift_norm_rows(self._c(), _p(rows), len(rows), C.c_double(max_bin), _p(out)), "sift_norm_rows")
        return out

    def sift_norm_rows_device(self, rows_ptr, n, out_ptr, max_bin=0.2):
        """The same on dense [n][128] float32 rows in HBM (device pointers, 4-byte aligned; out_ptr may be rows_ptr)."""
        _check(lib().modsx_sift_norm_rows_device(self._c(), C.c_void_p(rows_ptr), int(n), C.c_double(max_bin), C.c_void_p(out_ptr)),
               "sift_norm_rows_device")

    def describe_regions_dspsift(self, img, regs, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1, num_scales=3, start_coef=0.5,
                                 end_coef=1.5, max_bin=0.2, out_ptr=None):
        """The reference's "DSPSIFT" branch: raw SIFT histograms at num_scales + 1 measurement sizes, pooled in f32, then the f32
        SIFT norm: [n][128] float32 holding 0..255 (out_ptr: into that device pointer instead, returns None).  The defaults are
        DomainSizePolingParams' (matching/siftdesc.h:21-31)."""
        regs = np.ascontiguousarray(regs, REGION)
        args = (self._c(), C.c_void_p(img.h), _p(regs), len(regs), C.c_double(mr_size), int(patch_size), int(fast), int(photo_norm),
                int(num_scales), C.c_double(start_coef), C.c_double(end_coef), C.c_double(max_bin))
        if out_ptr is not None:
            _check(lib().modsx_describe_regions_dspsift_device(*args, C.c_void_p(out_ptr)), "describe_regions_dspsift_device")
            return None
        desc = np.zeros((len(regs), 128), np.float32)
        _check(lib().modsx_describe_regions_dspsift(*args, _p(desc)), "describe_regions_dspsift")
        return desc

    def dsp_counters(self):
        """dict of DSP_COUNTERS: DSP-SIFT work of this context since it was created (cumulative)."""
        return self._counters("modsx_dsp_counters", DSP_COUNTERS)

    def describe_counters(self):
        """dict of DESCRIBE_COUNTERS: what the description stage planned on this context since it was created (cumulative), and
        of DESCRIBE_DEVICE_COUNTERS: `ordered_workgroups`, read from the device (the call waits for the context's stream)."""
        return self._counters("modsx_describe_counters", DESCRIBE_COUNTERS + DESCRIBE_DEVICE_COUNTERS)

    def describe_slim_counters(self):
        """dict of DESCRIBE_SLIM_COUNTERS: SIFT launch sets of this context that took the slim form of the describe kernel / the
        full kernel, and the slim form's workgroups that its redo launch ran again (the call waits for the context's stream)."""
        return self._counters("modsx_describe_slim_counters", DESCRIBE_SLIM_COUNTERS)

    def detect_counters(self):
        """dict of DETECT_COUNTERS: what the pyramid and the extrema scan launched on this context since it was created (the
        last_* entries describe its last scan / candidate set)."""
        return self._counters("modsx_detect_counters", DETECT_COUNTERS)

    def debug_pyramids(self, images, params):
        """modsx_debug_pyramids: the pyramids of a batch of Images (sizes may differ) -> per image a list of (blurs, resps) per
        octave, each [numberOfScales + 2, rows, cols] f32."""
        n, L = len(images), params.numberOfScales + 2
        ptrs = (C.c_void_p * max(1, n))(*[im.h for im in images])
        geo = np.zeros((max(1, n), 49), np.int32)
        need = C.c_ulonglong(0)
        _check(lib().modsx_debug_pyramids(self._c(), ptrs, n, C.byref(params), _p(geo), None, 0, C.byref(need)), "debug_pyramids")
        planes = np.empty(max(1, need.value), np.float32)
        _check(lib().modsx_debug_pyramids(self._c(), ptrs, n, C.byref(params), _p(geo), _p(planes), need.value, C.byref(need)),
               "debug_pyramids")
        out, at = [], 0
        for i in range(n):
            octs = []
            for o in range(int(geo[i, 0])):
                r, c = int(geo[i, 1 + 2 * o]), int(geo[i, 2 + 2 * o])
                m = L * r * c
                octs.append((planes[at:at + m].reshape(L, r, c), planes[at + m:at + 2 * m].reshape(L, r, c)))
                at += 2 * m
            out.append(octs)
        assert at == need.value
        return out

    def debug_scan_levels(self, resps, blurs, params):
        """modsx_debug_scan_levels: the production extrema scan on the numberOfScales + 2 response / blur planes ([L, rows, cols])
        of one octave -> (raw accepted CANDIDATE records in device order, SSKP keypoints after detection order and claim)."""
        resps, blurs = np.ascontiguousarray(resps, np.float32), np.ascontiguousarray(blurs, np.float32)
        assert resps.ndim == 3 and resps.shape == blurs.shape
        L, rows, cols = resps.shape
        cands, out, nc = C.c_void_p(), C.c_void_p(), C.c_int(0)
        n = _check(lib().modsx_debug_scan_levels(self._c(), _p(resps), _p(blurs), L, rows, cols, C.byref(params), C.byref(cands),
                                                 C.byref(nc), C.byref(out)), "debug_scan_levels")
        return _take(cands, nc.value, CANDIDATE), _take(out, n, SSKP)

    def debug_detect_scalespace_batch(self, images, params):
        """modsx_debug_detect_scalespace_batch: detect_scalespace of up to 32 Images in one launch set -> list of SSKP arrays."""
        n = len(images)
        ptrs = (C.c_void_p * max(1, n))(*[im.h for im in images])
        outs = (C.c_void_p * max(1, n))()
        counts = np.zeros(max(1, n), np.int32)
        _check(lib().modsx_debug_detect_scalespace_batch(self._c(), ptrs, n, C.byref(params), outs, _p(counts)),
               "debug_detect_scalespace_batch")
        return [_take(C.c_void_p(outs[i]), int(counts[i]), SSKP) for i in range(n)]

    def match_fginn(self, d1, d2, pos2, ratio=0.8, contrad_dist=30.0, nn=50):
        d1 = np.ascontiguousarray(d1, np.float32)
        d2 = np.ascontiguousarray(d2, np.float32)
        pos2 = np.ascontiguousarray(pos2, np.float64)
        out = C.c_void_p()
        n = _check(lib().modsx_match_fginn(self._c(), _p(d1), len(d1), _p(d2), len(d2), _p(pos2), C.c_double(ratio),
                                           C.c_double(contrad_dist), nn, C.byref(out)), "match_fginn")
        return _take(out, n, TENT)

    def db_create(self, rows):
        """modsx_db_create: [n][128] descriptors holding the integers 0..255 (uint8, or anything convertible to float32)."""
        a = np.ascontiguousarray(rows)
        if a.dtype != np.uint8:
            a = np.ascontiguousarray(a, np.float32)
        if a.ndim != 2 or a.shape[1] != 128:
            raise ValueError("db_create: an [n][128] array is expected")
        h = lib().modsx_db_create(self._c(), _p(a), a.shape[0], 0 if a.dtype == np.uint8 else 1)
        if not h:
            raise RuntimeError("modsx_db_create failed: " + _err())
        return Db(self, h)

    def db_nearest(self, db, desc):
        """Squared L2 distance of every descriptor to its nearest database row (float32, exact integers)."""
        d = np.ascontiguousarray(desc, np.float32)
        out = np.empty(len(d), np.float32)
        _check(lib().modsx_db_nearest(self._c(), C.c_void_p(db.h), _p(d), len(d), _p(out)), "db_nearest")
        return out

    def match_fginn_db(self, d1, d2, pos2, db, ratio=0.8, contrad_dist=30.0, nn=50):
        """MatchFlannFGINNPlusDB: (tentatives, d2byDB)."""
        d1 = np.ascontiguousarray(d1, np.float32)
        d2 = np.ascontiguousarray(d2, np.float32)
        pos2 = np.ascontiguousarray(pos2, np.float64)
        out, dd = C.c_void_p(), C.c_void_p()
        n = _check(lib().modsx_match_fginn_db(self._c(), _p(d1), len(d1), _p(d2), len(d2), _p(pos2), C.c_double(ratio),
                                              C.c_double(contrad_dist), nn, C.c_void_p(db.h if db is not None else None),
                                              C.byref(out), C.byref(dd)), "match_fginn_db")
        return _take(out, n, TENT), _take(dd, n, np.dtype("f8"))

    def match_fginn_db_device(self, d1_ptr, n1, d2_ptr, n2, pos2, db, ratio=0.8, contrad_dist=30.0, nn=50):
        pos2 = np.ascontiguousarray(pos2, np.float64)
        out, dd = C.c_void_p(), C.c_void_p()
        n = _check(lib().modsx_match_fginn_db_device(self._c(), C.c_void_p(d1_ptr), int(n1), C.c_void_p(d2_ptr), int(n2),
                                                     _p(pos2), C.c_double(ratio), C.c_double(contrad_dist), nn,
                                                     C.c_void_p(db.h), C.byref(out), C.byref(dd)), "match_fginn_db_device")
        return _take(out, n, TENT), _take(dd, n, np.dtype("f8"))

    def set_fginn_db(self, db):
        """MatchPars::useDBforFGINN for the fused callers of this context; None detaches."""
        _check(lib().modsx_set_fginn_db(self._c(), C.c_void_p(db.h) if db is not None else None), "set_fginn_db")

    def synth_view(self, img, view):
        H = np.zeros(9)
        ident = C.c_int(0)
        h = lib().modsx_synth_view(self._c(), C.c_void_p(img.h), C.byref(view), _p(H), C.byref(ident))
        if not h:
            raise RuntimeError("modsx_synth_view failed: " + _err())
        rows, cols = C.c_int(), C.c_int()
        out = Image(self, h, 0, 0)
        # query the size through the resize tap (cheap): rows/cols live in the handle; read them via download size
        out.rows, out.cols = _image_dims(h)
        return out, H.reshape(3, 3), bool(ident.value)

    def synth_views(self, imgs, views):
        """modsx_debug_synth_views: the (image, view) items as ONE launch set (at most MAXB).  -> [(Image, is_identity)]; an
        identity view's Image aliases its source.  Free every Image."""
        n = len(views)
        assert n == len(imgs)
        hs = (C.c_void_p * n)(*[im.h for im in imgs])
        out = (C.c_void_p * n)()
        ident = (C.c_int * n)()
        _check(lib().modsx_debug_synth_views(self._c(), hs, _view_array(views), n, out, ident), "synth_views")
        res = []
        for i in range(n):
            im = Image(self, out[i], 0, 0)
            im.rows, im.cols = _image_dims(out[i])
            res.append((im, bool(ident[i])))
        return res

    def detect_describe_views(self, img, views, params, view_begin=0, view_step=1, want_desc=True, dev_desc=None,
                              dev_cap=0, want_counts=False):
        arr = _view_array(views)
        regs = C.c_void_p()
        desc = C.c_void_p()
        counts = (C.c_int * len(views))()
        n = _check(lib().modsx_detect_describe_views(self._c(), C.c_void_p(img.h), arr, len(views), C.byref(params),
                                                     int(view_begin), int(view_step), C.byref(regs),
                                                     C.byref(desc) if want_desc else None,
                                                     C.c_void_p(dev_desc) if dev_desc else None, C.c_long(dev_cap),
                                                     counts),
                   "detect_describe_views")
        r = _take(regs, n, REGION)
        d = None
        if want_desc:
            d = _take(desc, n * 128, np.dtype("f4")).reshape(n, 128) if n else np.zeros((0, 128), np.float32)
        if want_counts:
            return r, d, np.array(list(counts), np.int64)
        return r, d

    def match_fginn_device(self, d1_ptr, n1, d2_ptr, n2, pos2, ratio=0.8, contrad_dist=30.0, nn=50):
        pos2 = np.ascontiguousarray(pos2, np.float64)
        out = C.c_void_p()
        n = _check(lib().modsx_match_fginn_device(self._c(), C.c_void_p(d1_ptr), int(n1), C.c_void_p(d2_ptr), int(n2),
                                                  _p(pos2), C.c_double(ratio), C.c_double(contrad_dist), nn,
                                                  C.byref(out)), "match_fginn_device")
        return _take(out, n, TENT)

    def match_hamming(self, d1, d2, distance_threshold):
        """MatchFLANNDistance (exact Hamming search): [n][nbytes] rows, uint8 or anything convertible to float32 holding 0..255."""
        d1, d2, nbytes, dtype = _hamming_rows(d1, d2)
        out = C.c_void_p()
        n = _check(lib().modsx_match_hamming(self._c(), _p(d1), len(d1), _p(d2), len(d2), nbytes, dtype,
                                             C.c_double(distance_threshold), C.byref(out)), "match_hamming")
        return _take(out, n, TENT)

    def match_hamming_device(self, p1, n1, p2, n2, nbytes, distance_threshold):
        """The same on dense [n][nbytes] u8 rows in HBM (device pointers, any alignment)."""
        out = C.c_void_p()
        n = _check(lib().modsx_match_hamming_device(self._c(), C.c_void_p(p1), int(n1), C.c_void_p(p2), int(n2), int(nbytes),
                                                    C.c_double(distance_threshold), C.byref(out)), "match_hamming_device")
        return _take(out, n, TENT)

    def debug_match_hamming(self, p1, n1, p2, n2, nbytes, splits=0):
        """(nn2 [n1][4] = first, d(first), second, d(second); dict(tile, splits, workgroups, W)) of the device search with the train
        axis forced into `splits` parts (0 = production geometry)."""
        nn2 = np.zeros((max(int(n1), 1), 4), np.int32)
        geo = np.zeros(4, np.int32)
        _check(lib().modsx_debug_match_hamming(self._c(), C.c_void_p(p1), int(n1), C.c_void_p(p2), int(n2), int(nbytes), int(splits),
                                               _p(nn2), _p(geo)), "debug_match_hamming")
        return nn2[:int(n1)], dict(zip(HAMMING_GEOMETRY, (int(x) for x in geo)))

    def hamming_last_ms(self):
        """(packing ms, search ms) of this context's last Hamming search, HIP events; filled while profile() is on."""
        ms = np.zeros(2, np.float64)
        _check(lib().modsx_debug_hamming_last_ms(self._c(), _p(ms)), "hamming_last_ms")
        return float(ms[0]), float(ms[1])

    def match_regions_hamming(self, regs1, d1, regs2, d2, distance_threshold, params):
        """One binary-descriptor step on caller-supplied regions: MatchFLANNDistance + DuplicateFiltering + LO-RANSAC."""
        regs1 = np.ascontiguousarray(regs1, REGION)
        regs2 = np.ascontiguousarray(regs2, REGION)
        d1, d2, nbytes, dtype = _hamming_rows(d1, d2)
        if len(regs1) != len(d1) or len(regs2) != len(d2):
            raise ValueError("match_regions_hamming: one descriptor row per region is expected")
        res = PairResult()
        _check(lib().modsx_match_regions_hamming(self._c(), _p(regs1), _p(d1), len(d1), _p(regs2), _p(d2), len(d2), nbytes, dtype,
                                                 C.c_double(distance_threshold), C.byref(params), C.byref(res)),
               "match_regions_hamming")
        return _unpack_pair_result(res)

    def match_fginn_f32(self, d1, d2, pos2, ratio=0.8, contrad_dist=30.0, nn=50, dist=DIST_L2):
        """MatchFlannFGINN on float rows of any width: [n][dim] float32, dim % 4 == 0, dim <= 256; pos2 [n2][2].  dist: DIST_L2 (the
        default: the entry without a distance argument) or DIST_L1 (vector_dist = L1)."""
        d1, d2, dim = _f32_rows(d1, d2)
        pos2 = np.ascontiguousarray(pos2, np.float64)
        out = C.c_void_p()
        head = (self._c(), _p(d1), len(d1), _p(d2), len(d2), dim, _p(pos2), C.c_double(ratio), C.c_double(contrad_dist), int(nn))
        if dist == DIST_L2:
            n = _check(lib().modsx_match_fginn_f32(*head, C.byref(out)), "match_fginn_f32")
        else:
            n = _check(lib().modsx_match_fginn_f32_dist(*head, int(dist), C.byref(out)), "match_fginn_f32_dist")
        return _take(out, n, TENT)

    def match_fginn_f32_device(self, p1, n1, p2, n2, dim, pos2, ratio=0.8, contrad_dist=30.0, nn=50, dist=DIST_L2):
        """The same on dense [n][dim] float32 rows in HBM (device pointers, 4-byte aligned)."""
        pos2 = np.ascontiguousarray(pos2, np.float64)
        out = C.c_void_p()
        head = (self._c(), C.c_void_p(p1), int(n1), C.c_void_p(p2), int(n2), int(dim), _p(pos2), C.c_double(ratio),
                C.c_double(contrad_dist), int(nn))
        if dist == DIST_L2:
            n = _check(lib().modsx_match_fginn_f32_device(*head, C.byref(out)), "match_fginn_f32_device")
        else:
            n = _check(lib().modsx_match_fginn_f32_dist_device(*head, int(dist), C.byref(out)), "match_fginn_f32_dist_device")
        return _take(out, n, TENT)

    def debug_match_fginn_f32(self, d1, d2, pos2, ratio=0.8, contrad_dist=30.0, nn=50, splits=0, stage_mask=3, dist=DIST_L2):
        """dict(tentatives, top4 [n1][4] uint64 keys, stage [n1] (0 host walk, 1 resolve sweep, 2 its count: the nn ran out), geometry,
        resolve, by_count, records, flag) of the matcher with the train axis forced into `splits` parts (0 = production) and the
        stages of `stage_mask` (1 = top-4 search + host walk, 3 = + resolve sweep)."""
        d1, d2, dim = _f32_rows(d1, d2)
        head = (self._c(), _p(d1), len(d1), _p(d2), len(d2), dim)
        if dist == DIST_L2:
            return self._debug_fginn(lib().modsx_debug_match_fginn_f32, "debug_match_fginn_f32", head, len(d1), pos2, ratio,
                                     contrad_dist, (int(nn),), splits, stage_mask)
        return self._debug_fginn(lib().modsx_debug_match_fginn_f32_dist, "debug_match_fginn_f32_dist", head, len(d1), pos2, ratio,
                                 contrad_dist, (int(nn), int(dist)), splits, stage_mask)

    def _debug_fginn(self, fn, name, head, n1, pos2, ratio, contrad_dist, nn_dist, splits, stage_mask):
        pos2 = np.ascontiguousarray(pos2, np.float64)
        top4 = np.zeros((max(n1, 1), 4), np.uint64)
        stage = np.zeros(max(n1, 1), np.uint8)
        geo, cnt = np.zeros(6, np.int32), np.zeros(4, np.int32)
        out = C.c_void_p()
        n = _check(fn(*head, _p(pos2), C.c_double(ratio), C.c_double(contrad_dist), *nn_dist, int(splits), int(stage_mask), _p(top4),
                      _p(stage), _p(geo), _p(cnt), C.byref(out)), name)
        return dict(tentatives=_take(out, n, TENT), top4=top4[:n1], stage=stage[:n1],
                    geometry=dict(zip(FGINN32_GEOMETRY, (int(x) for x in geo))), resolve=int(cnt[0]), by_count=int(cnt[1]),
                    records=int(cnt[2]), flag=int(cnt[3]))

    def match_fginn_l1(self, d1, d2, pos2, ratio=0.8, contrad_dist=30.0, nn=50):
        """MatchFlannFGINN under vector_dist = L1 on [n][128] rows holding the integers 0..255 (the domain of match_fginn), searched
        as bytes: the records of match_fginn_f32(dist=DIST_L1) on the same rows, bit for bit."""
        d1, d2, dim = _f32_rows(d1, d2)
        if dim != 128:
            raise ValueError("match_fginn_l1: [n][128] rows are expected")
        pos2 = np.ascontiguousarray(pos2, np.float64)
        out = C.c_void_p()
        n = _check(lib().modsx_match_fginn_l1(self._c(), _p(d1), len(d1), _p(d2), len(d2), _p(pos2), C.c_double(ratio),
                                              C.c_double(contrad_dist), int(nn), C.byref(out)), "match_fginn_l1")
        return _take(out, n, TENT)

    def match_fginn_l1_device(self, p1, n1, p2, n2, pos2, ratio=0.8, contrad_dist=30.0, nn=50):
        """The same on dense [n][128] uint8 rows in HBM (device pointers, any alignment)."""
        pos2 = np.ascontiguousarray(pos2, np.float64)
        out = C.c_void_p()
        n = _check(lib().modsx_match_fginn_l1_device(self._c(), C.c_void_p(p1), int(n1), C.c_void_p(p2), int(n2), _p(pos2),
                                                     C.c_double(ratio), C.c_double(contrad_dist), int(nn), C.byref(out)),
                   "match_fginn_l1_device")
        return _take(out, n, TENT)

    def debug_match_fginn_l1(self, d1, d2, pos2, ratio=0.8, contrad_dist=30.0, nn=50, splits=0, stage_mask=3):
        """debug_match_fginn_f32 for match_fginn_l1; geometry["DK"] is the row width in 32-bit words."""
        d1, d2, dim = _f32_rows(d1, d2)
        if dim != 128:
            raise ValueError("debug_match_fginn_l1: [n][128] rows are expected")
        return self._debug_fginn(lib().modsx_debug_match_fginn_l1, "debug_match_fginn_l1", (self._c(), _p(d1), len(d1), _p(d2), len(d2)),
                                 len(d1), pos2, ratio, contrad_dist, (int(nn),), splits, stage_mask)

    def fginn32_last_ms(self):
        """(packing ms, search ms) of this context's last f32 FGINN search or L1 search on byte rows, HIP events; filled while
        profile() is on."""
        ms = np.zeros(2, np.float64)
        _check(lib().modsx_debug_fginn32_last_ms(self._c(), _p(ms)), "fginn32_last_ms")
        return float(ms[0]), float(ms[1])

    def match_regions_f32(self, regs1, d1, regs2, d2, params, dist=DIST_L2):
        """One float-descriptor step on caller-supplied regions: MatchFlannFGINN (params.match_ratio, contradDist, nn; positions
        = reproj_kp of regs2) + DuplicateFiltering + LO-RANSAC.  dist: DIST_L2 or DIST_L1."""
        regs1 = np.ascontiguousarray(regs1, REGION)
        regs2 = np.ascontiguousarray(regs2, REGION)
        d1, d2, dim = _f32_rows(d1, d2)
        if len(regs1) != len(d1) or len(regs2) != len(d2):
            raise ValueError("match_regions_f32: one descriptor row per region is expected")
        res = PairResult()
        head = (self._c(), _p(regs1), _p(d1), len(d1), _p(regs2), _p(d2), len(d2), dim, C.byref(params))
        if dist == DIST_L2:
            _check(lib().modsx_match_regions_f32(*head, C.byref(res)), "match_regions_f32")
        else:
            _check(lib().modsx_match_regions_f32_dist(*head, int(dist), C.byref(res)), "match_regions_f32_dist")
        return _unpack_pair_result(res)

    def match_regions_l1(self, regs1, d1, regs2, d2, params):
        """match_regions_f32 with match_fginn_l1 as the matcher: [n][128] rows holding the integers 0..255."""
        regs1 = np.ascontiguousarray(regs1, REGION)
        regs2 = np.ascontiguousarray(regs2, REGION)
        d1, d2, dim = _f32_rows(d1, d2)
        if dim != 128 or len(regs1) != len(d1) or len(regs2) != len(d2):
            raise ValueError("match_regions_l1: one [128] descriptor row per region is expected")
        res = PairResult()
        _check(lib().modsx_match_regions_l1(self._c(), _p(regs1), _p(d1), len(d1), _p(regs2), _p(d2), len(d2), C.byref(params),
                                            C.byref(res)), "match_regions_l1")
        return _unpack_pair_result(res)

    def rep_match_fginn(self, rep1, rep2, detector=0, desc_type=1, ratio=0.8, contrad_dist=30.0, nn=50):
        """MatchFlannFGINN of one class of two stored representations: rep1 the queries, rep2 (pre-packed) the trains."""
        out = C.c_void_p()
        n = _check(lib().modsx_rep_match_fginn(self.h, rep1.h, rep2.h, int(detector), int(desc_type), C.c_double(ratio),
                                               C.c_double(contrad_dist), int(nn), C.byref(out)), "rep_match_fginn")
        return _take(out, n, TENT)

    def rep_match_fginn_f32(self, rep1, rep2, detector=0, desc_type=DESC_CAFFE, ratio=0.8, contrad_dist=30.0, nn=50):
        """MatchFlannFGINN of one float class of two stored representations: rep1 the queries, rep2 the trains."""
        out = C.c_void_p()
        n = _check(lib().modsx_rep_match_fginn_f32(self.h, rep1.h, rep2.h, int(detector), int(desc_type), C.c_double(ratio),
                                                   C.c_double(contrad_dist), int(nn), C.byref(out)), "rep_match_fginn_f32")
        return _take(out, n, TENT)

    def rep_match_group_f32(self, rep1, reps2, detector=0, desc_type=DESC_CAFFE, ratio=0.8, contrad_dist=30.0, nn=50):
        """The grouped launch set: one float class of rep1 against that class of 1..4 partners; a list of TENT arrays."""
        G = len(reps2)
        rarr = (C.c_void_p * max(1, G))(*[r.h for r in reps2])
        outs = (C.c_void_p * max(1, G))()
        counts = (C.c_int * max(1, G))()
        _check(lib().modsx_rep_match_group_f32(self.h, rep1.h, rarr, G, int(detector), int(desc_type), C.c_double(ratio),
                                               C.c_double(contrad_dist), int(nn), outs, counts), "rep_match_group_f32")
        return [_take(C.c_void_p(outs[g]), counts[g], TENT) for g in range(G)]

    def fginn32_group_counters(self):
        """dict(launch_sets, problems, resolve_queries, resolve_launches) of the grouped f32 matcher on this context, cumulative."""
        out = np.zeros(4, np.int64)
        _check(lib().modsx_fginn32_group_counters(self.h, _p(out), 4), "fginn32_group_counters")
        return dict(zip(("launch_sets", "problems", "resolve_queries", "resolve_launches"), (int(x) for x in out)))

    def rep_match_hamming(self, rep1, rep2, detector=DET_ORB, desc_type=DESC_ORB, distance_threshold=64.0):
        """MatchFLANNDistance of one binary class of two stored representations: rep1 the queries, rep2 the trains."""
        out = C.c_void_p()
        n = _check(lib().modsx_rep_match_hamming(self.h, rep1.h, rep2.h, int(detector), int(desc_type), C.c_double(distance_threshold),
                                                 C.byref(out)), "rep_match_hamming")
        return _take(out, n, TENT)

    def rep_match_group_hamming(self, rep1, reps2, detector=DET_ORB, desc_type=DESC_ORB, distance_threshold=64.0):
        """The grouped launch set: one binary class of rep1 against that class of 1..4 partners; a list of TENT arrays."""
        G = len(reps2)
        rarr = (C.c_void_p * max(1, G))(*[r.h for r in reps2])
        outs = (C.c_void_p * max(1, G))()
        counts = (C.c_int * max(1, G))()
        _check(lib().modsx_rep_match_group_hamming(self.h, rep1.h, rarr, G, int(detector), int(desc_type),
                                                   C.c_double(distance_threshold), outs, counts), "rep_match_group_hamming")
        return [_take(C.c_void_p(outs[g]), counts[g], TENT) for g in range(G)]

    def hamming_group_counters(self):
        """dict of HAMMING_GROUP_COUNTERS: grouped Hamming launch sets, problems in them, rows packed by appends and pack launches
        issued at match time (none for stored matches) on this context, cumulative."""
        out = np.zeros(4, np.int64)
        _check(lib().modsx_hamming_group_counters(self.h, _p(out), 4), "hamming_group_counters")
        return dict(zip(HAMMING_GROUP_COUNTERS, (int(x) for x in out)))

    def match_pair_views(self, img1, img2, views, params):
        arr = _view_array(views)
        res = PairResult()
        _check(lib().modsx_match_pair_views(self._c(), C.c_void_p(img1.h), C.c_void_p(img2.h), arr, len(views),
                                            C.byref(params), C.byref(res)), "match_pair_views")
        return _unpack_pair_result(res)

    # ---- view-sharded path (engine_shard.hip): `comm` is a handle from modsx_comm_create on this context ----
    def comm_create(self, id128, rank, world):
        h = lib().modsx_comm_create(self._c(), id128, int(rank), int(world))
        if not h:
            raise RuntimeError("modsx_comm_create failed: " + _err())
        return h

    def detect_describe_views_sharded(self, comm, img, views, params):
        """All regions in reference order on every rank + the device pointer of their [n][128] u8 descriptors."""
        arr = _view_array(views)
        regs, dptr = C.c_void_p(), C.c_void_p()
        counts = (C.c_int * len(views))()
        n = _check(lib().modsx_detect_describe_views_sharded(self._c(), C.c_void_p(comm), C.c_void_p(img.h), arr, len(views),
                                                             C.byref(params), C.byref(regs), C.byref(dptr), counts),
                   "detect_describe_views_sharded")
        return _take(regs, n, REGION), dptr.value, np.array(list(counts), np.int64)

    def match_fginn_sharded(self, comm, d1_ptr, n1, d2_ptr, n2, pos2, ratio=0.8, contrad_dist=30.0, nn=50):
        pos2 = np.ascontiguousarray(pos2, np.float64)
        out = C.c_void_p()
        n = _check(lib().modsx_match_fginn_sharded(self._c(), C.c_void_p(comm), C.c_void_p(d1_ptr), int(n1), C.c_void_p(d2_ptr),
                                                   int(n2), _p(pos2), C.c_double(ratio), C.c_double(contrad_dist), nn,
                                                   C.byref(out)), "match_fginn_sharded")
        return _take(out, n, TENT)

    def match_pair_views_sharded(self, comm, img1, img2, views, params, owner=0):
        arr = _view_array(views)
        res = PairResult()
        _check(lib().modsx_match_pair_views_sharded(self._c(), C.c_void_p(comm), C.c_void_p(img1.h), C.c_void_p(img2.h), arr,
                                                    len(views), C.byref(params), int(owner), C.byref(res)),
               "match_pair_views_sharded")
        return _unpack_pair_result(res)

    def match_pairs_views_sharded(self, comm, imgs1, imgs2, views, params, owner_base=0, arrays=True):
        """modsx_match_pairs_views_sharded: len(imgs1) <= 16 pairs in one sharded call; pair g is matched and verified by rank
        (owner_base + g) % world alone (owner_base < 0: every rank returns every pair).  Returns the list of per-pair results."""
        n = len(imgs1)
        a1 = (C.c_void_p * n)(*[im.h for im in imgs1])
        a2 = (C.c_void_p * n)(*[im.h for im in imgs2])
        arr = _view_array(views)
        res = (PairResult * n)()
        _check(lib().modsx_match_pairs_views_sharded(self._c(), C.c_void_p(comm), a1, a2, n, arr, len(views), C.byref(params),
                                                     int(owner_base), res), "match_pairs_views_sharded")
        return [_unpack_pair_result(res[i], arrays) for i in range(n)]

    def shard_device_pack(self, regs, descs, row_format=SHARD_ROW_REGION):
        """k_pack_rows on host-provided regions + descriptors: the rows part of a block, [n, R + 128 * ndesc] u8 (R = 200 or 56)."""
        L = lib()
        L.modsx_shard_device_pack.restype = C.c_long
        regs = np.ascontiguousarray(regs, REGION)
        descs = [np.ascontiguousarray(d, np.uint8) for d in descs]
        out = np.zeros((len(regs), shard_region_bytes(row_format) + 128 * len(descs)), np.uint8)
        _check(L.modsx_shard_device_pack(self._c(), _p(regs), _ptr_array(descs), len(descs), len(regs), int(row_format), _p(out)),
               "shard_device_pack")
        return out

    def shard_device_unpack(self, blocks, world, items, block_rows, ndesc=1, row_format=SHARD_ROW_REGION):
        """k_unpack_blocks on gathered blocks: (regs [world * block_rows] -- REGION records, or [.., 7] f64 for SHARD_ROW_KP --,
        [desc per class], pos [.., 2]); rows past the list's end are zero."""
        L = lib()
        L.modsx_shard_device_unpack.restype = C.c_long
        blocks = np.ascontiguousarray(blocks, np.uint8)
        cap = world * block_rows
        regs = np.zeros(cap, REGION) if row_format == SHARD_ROW_REGION else np.zeros((cap, 7), np.float64)
        descs = [np.zeros((cap, 128), np.uint8) for _ in range(ndesc)]
        pos = np.zeros((cap, 2), np.float64)
        _check(L.modsx_shard_device_unpack(self._c(), _p(blocks), int(world), int(items), int(block_rows), int(ndesc), int(row_format),
                                           _p(regs), _ptr_array(descs), _p(pos), C.c_long(cap)), "shard_device_unpack")
        return regs, descs, pos

    def detect_msers(self, img, params=None, tilt=1.0, zoom=1.0):
        params = params or default_mser_params()
        out = C.c_void_p()
        n = _check(lib().modsx_detect_msers(self._c(), C.c_void_p(img.h), C.byref(params), C.c_double(tilt),
                                            C.c_double(zoom), C.byref(out)), "detect_msers")
        return _take(out, n, KEYPOINT)

    def debug_mser_front(self, views):
        """modsx_debug_mser_front: the device half of the MSER view loop (u8 truncation, bin sort, block layout, one download)
        for ONE launch set of f32 views (2-d arrays, any sizes from 1 x 1, at most 32) -> per view (u8 [rows, cols], start [257]
        int32, order [rows * cols] int32: padded offsets (r + 1) * (cols + 2) + c + 1 by grey level, raster order in a level)."""
        views = [np.ascontiguousarray(v, np.float32) for v in views]
        n = len(views)
        if any(v.ndim != 2 for v in views):
            raise ValueError("debug_mser_front: 2-d views are expected")
        ptrs = (C.c_void_p * max(1, n))(*[v.ctypes.data for v in views])
        rows = np.array([v.shape[0] for v in views] or [0], np.int32)
        cols = np.array([v.shape[1] for v in views] or [0], np.int32)
        npx = [v.size for v in views]
        u8, order = np.zeros(max(1, sum(npx)), np.uint8), np.zeros(max(1, sum(npx)), np.int32)
        start = np.zeros((max(1, n), 257), np.int32)
        _check(lib().modsx_debug_mser_front(self._c(), ptrs, _p(rows), _p(cols), n, _p(u8), _p(start), _p(order)), "debug_mser_front")
        out, at = [], 0
        for i, v in enumerate(views):
            out.append((u8[at:at + npx[i]].reshape(v.shape), start[i], order[at:at + npx[i]]))
            at += npx[i]
        return out

    def match_ladder(self, img1, img2, steps, params, min_matches=10, comm=None):
        """steps: list of (views, match_ratio[, detector[, descs]]); descs = [(descriptor type, FGINN ratio), ...] is the
        section's Descriptors / FGINNThreshold lists (None: the parameter block's).  Returns (result dict, steps executed).
        comm: a communicator handle => modsx_match_ladder_sharded (every step's views sharded over the ranks)."""
        arr = (LadderStep * len(steps))()
        keep = []
        for i, st in enumerate(steps):
            views, ratio = st[0], st[1]
            va = _view_array(views)
            keep.append(va)
            arr[i].views = C.cast(va, C.c_void_p)
            arr[i].nviews = len(views)
            arr[i].match_ratio = float(ratio)
            arr[i].detector = int(st[2]) if len(st) > 2 else 0
            if len(st) > 3 and st[3] is not None:
                _set_descs(arr[i], st[3])
        res = PairResult()
        done = C.c_int(0)
        if comm is not None:
            _check(lib().modsx_match_ladder_sharded(self._c(), C.c_void_p(comm), C.c_void_p(img1.h), C.c_void_p(img2.h), arr,
                                                    len(steps), int(min_matches), C.byref(params), C.byref(res),
                                                    C.byref(done)), "match_ladder_sharded")
        else:
            _check(lib().modsx_match_ladder(self._c(), C.c_void_p(img1.h), C.c_void_p(img2.h), arr, len(steps),
                                            int(min_matches), C.byref(params), C.byref(res), C.byref(done)), "match_ladder")
        return _unpack_pair_result(res), done.value

    def match_pair(self, img1, img2, params):
        res = PairResult()
        _check(lib().modsx_match_pair(self._c(), C.c_void_p(img1.h), C.c_void_p(img2.h), C.byref(params),
                                      C.byref(res)), "match_pair")
        return _unpack_pair_result(res)

    def last_timings(self):
        t = (C.c_double * 6)()
        _check(lib().modsx_last_timings(self._c(), t), "last_timings")
        return dict(zip(["detect", "orient", "describe", "match", "verify", "total"], list(t)))

    def profile(self, enable=True):
        _check(lib().modsx_profile(self._c(), int(enable)), "profile")

    def kernel_stats(self):
        n = len(KERNEL_CLASSES)
        ms, work = (C.c_double * n)(), (C.c_double * n)()
        launches = (C.c_long * n)()
        _check(lib().modsx_kernel_stats(self._c(), ms, work, launches, n), "kernel_stats")
        return {k: dict(ms=ms[i], work=work[i], launches=launches[i]) for i, k in enumerate(KERNEL_CLASSES)}


class _ImageStruct(C.Structure):   # mirrors struct modsx_image (engine.hpp) for reading rows/cols of a handle
    _fields_ = [("d", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("owned", C.c_bool)]


def last_batch_verify_each():
    """Verification time in ms of every pair of the last batch call (completion order)."""
    n = lib().modsx_debug_last_batch_verify_each(None, 0)
    out = np.zeros(max(n, 1), np.float64)
    n = min(n, lib().modsx_debug_last_batch_verify_each(_p(out), len(out)))
    return out[:n]


def last_batch_verify():
    """(summed ms of DuplicateFiltering + LO-RANSAC, pairs verified, working contexts) of the last batch call: match_pairs,
    match_pairs_views, match_reps, or the last round of match_one_to_many."""
    ms, n, t = C.c_double(), C.c_int(), C.c_int()
    lib().modsx_last_batch_verify(C.byref(ms), C.byref(n), C.byref(t))
    return ms.value, n.value, t.value


def last_match_geometry():
    """dict(qs, fat, S, tiles_per_split, ntiles_ub): the shape the process's last matcher launch used for its first problem."""
    v = [C.c_int() for _ in range(5)]
    lib().modsx_last_match_geometry(*[C.byref(x) for x in v])
    return dict(zip(("qs", "fat", "S", "tiles_per_split", "ntiles_ub"), (x.value for x in v)))


HAMMING_GEOMETRY = ("tile", "splits", "workgroups", "W")   # include/modsx.h: modsx_debug_match_hamming, in its order


def _hamming_rows(d1, d2):
    """the two sides as contiguous [n][nbytes] arrays of one dtype: uint8 if both are, float32 otherwise"""
    d1, d2 = np.asarray(d1), np.asarray(d2)
    dt = np.uint8 if d1.dtype == np.uint8 and d2.dtype == np.uint8 else np.float32
    d1, d2 = np.ascontiguousarray(d1, dt), np.ascontiguousarray(d2, dt)
    if d1.ndim != 2 or d2.ndim != 2 or d1.shape[1] != d2.shape[1]:
        raise ValueError("hamming: two [n][nbytes] arrays of one width are expected")
    return d1, d2, d1.shape[1], 0 if dt == np.uint8 else 1


def hamming_geometry(n1, n2, nbytes, splits=0):
    """dict(tile, splits, workgroups, W): what the Hamming search launches for these sizes (host only, no GPU); splits = 0 is the
    production geometry, more splits than tiles are cut down to one per tile."""
    geo = np.zeros(4, np.int32)
    _check(lib().modsx_debug_hamming_geometry(int(n1), int(n2), int(nbytes), int(splits), _p(geo)), "hamming_geometry")
    return dict(zip(HAMMING_GEOMETRY, (int(x) for x in geo)))


def hamming_tentatives(nn2, distance_threshold):
    """The record rule of MatchFLANNDistance (matching.cpp:647-661) on a search result nn2 = [n1][4] = first, d(first), second,
    d(second) (host only, no GPU)."""
    nn2 = np.ascontiguousarray(nn2, np.int32).reshape(-1, 4)
    out = C.c_void_p()
    n = _check(lib().modsx_hamming_tentatives(_p(nn2), len(nn2), C.c_double(distance_threshold), C.byref(out)), "hamming_tentatives")
    return _take(out, n, TENT)


def blur_geometry(shapes):
    """modsx_blur_geometry (host only): (tile rows, tiles) of the pyramid's blur launch over planes of the given (rows, cols):
    32-row tiles from 2560 tiles on, 16-row tiles below."""
    sh = np.ascontiguousarray(shapes, np.int32).reshape(-1, 2)
    rows, cols = np.ascontiguousarray(sh[:, 0]), np.ascontiguousarray(sh[:, 1])
    geo = np.zeros(2, np.int32)
    _check(lib().modsx_blur_geometry(_p(rows), _p(cols), len(sh), _p(geo)), "blur_geometry")
    return int(geo[0]), int(geo[1])


FGINN32_GEOMETRY = ("tile", "splits", "workgroups", "DK", "tiles", "tiles_per_split")   # include/modsx.h, in its order


def _f32_rows(d1, d2):
    """the two sides as contiguous [n][dim] float32 arrays of one width"""
    d1, d2 = np.ascontiguousarray(d1, np.float32), np.ascontiguousarray(d2, np.float32)
    if d1.ndim != 2 or d2.ndim != 2 or d1.shape[1] != d2.shape[1]:
        raise ValueError("fginn_f32: two [n][dim] arrays of one width are expected")
    return d1, d2, d1.shape[1]


def fginn32_geometry(n1, n2, dim, splits=0):
    """dict(tile, splits, workgroups, DK, tiles, tiles_per_split): what the f32 FGINN search launches for these sizes (host only, no
    GPU); splits = 0 is the production geometry, more splits than tiles are cut down to one per tile."""
    geo = np.zeros(6, np.int32)
    _check(lib().modsx_debug_fginn32_geometry(int(n1), int(n2), int(dim), int(splits), _p(geo)), "fginn32_geometry")
    return dict(zip(FGINN32_GEOMETRY, (int(x) for x in geo)))


def fginn_l1_geometry(n1, n2, splits=0):
    """fginn32_geometry for the L1 search on byte rows (match_fginn_l1): DK is the row width in 32-bit words (host only, no GPU)."""
    geo = np.zeros(6, np.int32)
    _check(lib().modsx_debug_fginn_l1_geometry(int(n1), int(n2), int(splits), _p(geo)), "fginn_l1_geometry")
    return dict(zip(FGINN32_GEOMETRY, (int(x) for x in geo)))


def rep_class_rank(detector, desc_type):
    """The position of a class in the order match_reps concatenates the classes in (descriptor name, then detector name, as the
    reference's std::map walks them); -1 when there is no such class (host only)."""
    return int(lib().modsx_rep_class_rank(int(detector), int(desc_type)))


def fginn32_group_geometry(n1, n2, dim):
    """The train axis of the grouped f32 search for n1 queries against len(n2) <= 4 partners of n2[g] rows (host only): dict(tile,
    DK, gx, splits = [(partner, first tile, end tile), ...] in launch order, per_problem = [(tiles, splits, tiles per split), ...])."""
    n2 = np.ascontiguousarray(n2, np.int32)
    geo, per = np.zeros(4, np.int32), np.zeros((max(1, len(n2)), 3), np.int32)
    total = _check(lib().modsx_debug_fginn32_group_geometry(int(n1), _p(n2), len(n2), int(dim), _p(geo), _p(per), None, 0),
                   "fginn32_group_geometry")
    sp = np.zeros((max(1, total), 3), np.int32)
    _check(lib().modsx_debug_fginn32_group_geometry(int(n1), _p(n2), len(n2), int(dim), _p(geo), _p(per), _p(sp), total),
           "fginn32_group_geometry")
    return dict(tile=int(geo[0]), DK=int(geo[1]), gx=int(geo[2]), splits=[tuple(int(v) for v in r) for r in sp[:total]],
                per_problem=[tuple(int(v) for v in r) for r in per[:len(n2)]])


def rep_class_order(detector, desc_type):
    """The position of a class in the order match_reps concatenates ALL kinds of classes in, the binary ones included: 4 x the
    place of the descriptor's name + the place of the detector's name among the reference's names; -1 when a representation has
    no such class (host only)."""
    return int(lib().modsx_rep_class_order(int(detector), int(desc_type)))


def hamming_group_geometry(n1, n2, nbytes):
    """The table of the grouped Hamming search for n1 queries against len(n2) <= 4 partners of n2[g] rows (host only): dict(tile,
    WK, gx, splits = [(partner, first tile, end tile), ...] in launch order, per_problem = [(tiles, splits, tiles per split), ...])."""
    n2 = np.ascontiguousarray(n2, np.int32)
    geo, per = np.zeros(4, np.int32), np.zeros((max(1, len(n2)), 3), np.int32)
    total = _check(lib().modsx_debug_hamming_group_geometry(int(n1), _p(n2), len(n2), int(nbytes), _p(geo), _p(per), None, 0),
                   "hamming_group_geometry")
    sp = np.zeros((max(1, total), 3), np.int32)
    _check(lib().modsx_debug_hamming_group_geometry(int(n1), _p(n2), len(n2), int(nbytes), _p(geo), _p(per), _p(sp), total),
           "hamming_group_geometry")
    return dict(tile=int(geo[0]), WK=int(geo[1]), gx=int(geo[2]), splits=[tuple(int(v) for v in r) for r in sp[:total]],
                per_problem=[tuple(int(v) for v in r) for r in per[:len(n2)]])


def fginn32_dpass(d0, ratio):
    """the smallest float32 d > 0 with float64(float32(d0) / d) <= ratio^2 per pair, by the library's bisection (host only)"""
    d0 = np.ascontiguousarray(d0, np.float32).reshape(-1)
    ratio = np.ascontiguousarray(ratio, np.float64).reshape(-1)
    if len(d0) != len(ratio):
        raise ValueError("fginn32_dpass: one ratio per d0 is expected")
    out = np.zeros(len(d0), np.float32)
    _check(lib().modsx_debug_fginn32_dpass(_p(d0), _p(ratio), len(d0), _p(out)), "fginn32_dpass")
    return out


BAUMBERG_GEOMETRY = ("kernel", "chunk", "nchunks", "grid")   # include/modsx.h: modsx_debug_baumberg_geometry, in its order


def baumberg_geometry(n, W=19, variant=0, chunk=0):
    """dict(kernel, chunk, nchunks, grid): what a Baumberg launch of n keypoints at window W runs (host only, no GPU).  kernel 0 =
    the two-slot stream kernel on static chunks, 1 = k_baumberg<19>, 2 = k_baumberg<0>, 3 = the stream kernel fed from the launch-wide
    queue (variant 3: chunk = wavefronts per range, nchunks = 8 ranges; its production rule, chunk 0, depends on the device:
    Context.baumberg_geometry); raises where there is no such launch."""
    geo = np.zeros(4, np.int32)
    _check(lib().modsx_debug_baumberg_geometry(int(n), int(W), int(variant), int(chunk), _p(geo)), "baumberg_geometry")
    return dict(zip(BAUMBERG_GEOMETRY, (int(x) for x in geo)))


def baumberg_production_variant(W=19):
    """the variant detect_affine_keypoints launches at window W (3 = the queue form, 0 = static chunks; MODSX_BAUMBERG_QUEUE=0 / 1 in
    the environment, read once per process, forces one or the other)"""
    return int(lib().modsx_debug_baumberg_variant(int(W)))


def check_borders(tuples):
    """interpolateCheckBorders as the kernels evaluate it (kmath.hpp check_borders, host build; no GPU) for an [n, 9] array of
    (cols, rows, ofsx, ofsy, a11, a12, a21, a22, W) -> bool [n]."""
    t = np.ascontiguousarray(tuples, np.float32).reshape(-1, 9)
    out = np.zeros(max(1, len(t)), np.uint8)
    _check(lib().modsx_debug_check_borders(_p(t), len(t), _p(out)), "check_borders")
    return out[:len(t)].astype(bool)


DESCRIBE_LANE_PHASES = ("sample", "rows", "cols_fused", "cols")   # include/modsx.h: modsx_debug_describe_lanes, in its order


def describe_lanes(P):
    """Lane slots of the LDS describe kernels for one P x P window (host only, no GPU): dict(ksize, NC, rows0, ro1) plus, per
    phase of DESCRIBE_LANE_PHASES, (useful, issued, issued_parent): slots that hold a sample or an output pair, slots this
    build issues, slots the rule before it issued."""
    k = np.zeros(16, np.int64)
    _check(lib().modsx_debug_describe_lanes(int(P), _p(k)), "describe_lanes")
    out = dict(zip(("ksize", "NC", "rows0", "ro1"), (int(x) for x in k[:4])))
    for q, name in enumerate(DESCRIBE_LANE_PHASES):
        out[name] = tuple(int(x) for x in k[4 + 3 * q:7 + 3 * q])
    return out


def describe_lane_map(rows, nc=0):
    """The tap slots of one parked chunk of the sampling kernel (host only): dict(cols, stride, park_words, magic, slots) for a
    row pass of `rows` rows and, for a chunk of nc columns, map = int32 [rows * nc, 3] of (row, column, park word) per sample e
    (lane e % 64 of slot e / 64)."""
    rule = np.zeros(5, np.int32)
    m = np.zeros((max(1, int(rows) * int(nc)), 3), np.int32)
    n = lib().modsx_debug_describe_lane_map(int(rows), int(nc), _p(rule), _p(m), len(m))
    if n < 0:
        _check(n, "describe_lane_map")
    out = dict(zip(("cols", "stride", "park_words", "magic", "slots"), (int(x) for x in rule)))
    out["map"] = m[:n]
    return out


def orientation_counts(reset=False):
    """(launched, skipped): orientation jobs launched by the pair / view pipelines of this process and regions left out of
    the launch because their reprojection is certain to drop them, since the last reset."""
    a, b = C.c_ulonglong(), C.c_ulonglong()
    lib().modsx_debug_orientation_counts(C.byref(a), C.byref(b), int(reset))
    return a.value, b.value


def orientation_launches(reset=False):
    """(lds_table, global_table): launches of the orientation kernel by this process since the last reset, by the instance that
    ran -- bin table copied to LDS (fewer than 8192 regions) or read in global memory."""
    a, b = C.c_ulonglong(), C.c_ulonglong()
    lib().modsx_debug_orientation_launches(C.byref(a), C.byref(b), int(reset))
    return a.value, b.value


def views_counters(reset=False):
    """(views_fused, groups, rotated_pixels): non-identity views this process sent through the fused view kernel, the groups of
    shared rotations they formed and the pixels those groups rotate (w_rot x h_rot per group), since the last reset."""
    a, b, d = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
    lib().modsx_debug_views_counters(C.byref(a), C.byref(b), C.byref(d), int(reset))
    return a.value, b.value, d.value


VIEW_GROUP_CAP = 8      # csrc/engine.hpp: most views that share one rotated tile


def view_plan(rows, cols, view):
    """modsx_debug_view_plan (host only): dict(identity, w_rot, h_rot, cols, rows, kx, ky, kind, rinv [6] f64, winv [6] f64) of
    one view of a rows x cols image; kind 2 = the fused launch."""
    g = np.zeros(8, np.int32)
    rinv, winv = np.zeros(6), np.zeros(6)
    _check(lib().modsx_debug_view_plan(int(rows), int(cols), C.byref(view), _p(g), _p(rinv), _p(winv)), "view_plan")
    return dict(identity=bool(g[0]), w_rot=int(g[1]), h_rot=int(g[2]), cols=int(g[3]), rows=int(g[4]), kx=int(g[5]), ky=int(g[6]),
                kind=int(g[7]), rinv=rinv, winv=winv, src_rows=int(rows), src_cols=int(cols))


def views_groups(plans, sources=None, cap=0):
    """modsx_debug_views_groups (host only): the grouping rule of the fused view launch on the non-identity views `plans`
    (dicts as view_plan returns them; sources[i]: which source image view i is of, default all 0).
    -> dict(group [n] (-1: not on the fused launch), order [n], views_fused, groups, tiles, rotated_pixels, rotated_pixels_alone)."""
    n = len(plans)
    assert not any(p["identity"] for p in plans), "identity views are not part of a launch set's job table"
    src = np.ascontiguousarray(np.zeros(n, np.int32) if sources is None else sources, np.int32)
    dims = np.ascontiguousarray([[p["src_rows"], p["src_cols"], p["h_rot"], p["w_rot"], p["kind"]] for p in plans], np.int32).reshape(n, 5)
    rinv = np.ascontiguousarray([p["rinv"] for p in plans], np.float64).reshape(n, 6)
    group, order = np.zeros(max(1, n), np.int32), np.zeros(max(1, n), np.int32)
    tot = np.zeros(5, np.int64)
    _check(lib().modsx_debug_views_groups(_p(src), _p(dims), _p(rinv), n, int(cap), _p(group), _p(order), _p(tot)), "views_groups")
    return dict(group=group[:n], order=order[:n], views_fused=int(tot[0]), groups=int(tot[1]), tiles=int(tot[2]),
                rotated_pixels=int(tot[3]), rotated_pixels_alone=int(tot[4]))


def orientation_tables():
    """The tables the orientation kernel reads, as the library builds them on the host (no device needed): dict(bin_table [2049]
    uint8 -- entry code * 256 + idx, [2048] the special case --, index_raster / index_lanes [1344] uint16 (row * stride + column of
    the voting pixels, raster order / the uploaded lane-major order), weight_raster / weight_lanes [1344] float32, n_real, length,
    stride, global_table_from)."""
    tab = np.zeros(2049, np.uint8)
    ir, il = np.zeros(1344, np.uint16), np.zeros(1344, np.uint16)
    wr, wl = np.zeros(1344, np.float32), np.zeros(1344, np.float32)
    k = np.zeros(4, np.int32)
    if lib().modsx_orientation_tables(None, None, None, None, None, _p(k)) != 0 or k[1] != 1344:
        raise RuntimeError("orientation_tables failed: " + _err())
    if lib().modsx_orientation_tables(_p(tab), _p(ir), _p(wr), _p(il), _p(wl), _p(k)) != 0:
        raise RuntimeError("orientation_tables failed: " + _err())
    return dict(bin_table=tab, index_raster=ir, weight_raster=wr, index_lanes=il, weight_lanes=wl, n_real=int(k[0]),
                length=int(k[1]), stride=int(k[2]), global_table_from=int(k[3]))


def reproject_certain_drop(regs, H, w, h, boxk=2 * 3.0 * 3.0 ** 0.5):
    """bool per region: reproject_regions(.., H, w, h) (boxk: the box factor, default k_sigma) removes it whatever its orientation."""
    regs = np.ascontiguousarray(regs, REGION)
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    drop = np.zeros(max(1, len(regs)), np.uint8)
    _check(lib().modsx_debug_reproject_certain_drop(_p(regs), len(regs), _p(H), int(w), int(h), C.c_double(boxk), _p(drop)),
           "reproject_certain_drop")
    return drop[:len(regs)].astype(bool)


DEFAULT_ARENA_FLOATS = 192 << 18    # the window arena of a describe chunk without MODSX_ARENA_MB: 192 MiB


def describe_plan(regs, mr_size, fast=0, arena_floats=DEFAULT_ARENA_FLOATS, max_cuts=4096):
    """modsx_debug_describe_plan: what the description stage plans for one call, on the host alone (no GPU, no context).
    regs: the region list of one image, or a list of them (one per image).  -> dict(rc, error, counters, cuts): rc 0 or the
    refusal's code with its text in `error`; counters (DESCRIBE_COUNTERS: what the device counts is not among them) as
    Context.describe_counters() of a fresh context shows them after that call; cuts: the flat index of the first region of every chunk after the first."""
    lists = [regs] if isinstance(regs, np.ndarray) else list(regs)
    counts = np.array([len(r) for r in lists], np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(r).view(REGION) for r in lists]) if lists else np.zeros(0, REGION), REGION)
    cnt = (C.c_long * len(DESCRIBE_COUNTERS))()
    cuts = (C.c_long * max(1, max_cuts))()
    ncuts = C.c_int(0)
    rc = lib().modsx_debug_describe_plan(_p(flat), _p(counts), len(lists), C.c_double(mr_size), int(fast), int(arena_floats), cnt,
                                         len(DESCRIBE_COUNTERS), cuts, max_cuts, C.byref(ncuts))
    assert ncuts.value <= max_cuts, "describe_plan: %d cuts, room for %d" % (ncuts.value, max_cuts)
    return dict(rc=rc, error=_err() if rc else "", counters=dict(zip(DESCRIBE_COUNTERS, (int(x) for x in cnt))),
                cuts=[int(cuts[i]) for i in range(ncuts.value)])


def describe_plan_slim(regs, mr_size, fast=0, arena_floats=DEFAULT_ARENA_FLOATS, max_chunks=4096):
    """modsx_debug_describe_plan_slim: per chunk of describe_plan's walk, whether it holds no region of the direct branch (the
    launch set may take the slim form of the describe kernel).  -> list of bool, one per chunk."""
    lists = [regs] if isinstance(regs, np.ndarray) else list(regs)
    counts = np.array([len(r) for r in lists], np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(r).view(REGION) for r in lists]) if lists else np.zeros(0, REGION), REGION)
    slim = np.zeros(max(1, max_chunks), np.uint8)
    nch = C.c_int(0)
    _check(lib().modsx_debug_describe_plan_slim(_p(flat), _p(counts), len(lists), C.c_double(mr_size), int(fast), int(arena_floats),
                                                _p(slim), max_chunks, C.byref(nch)), "debug_describe_plan_slim")
    assert nch.value <= max_chunks, "describe_plan_slim: %d chunks, room for %d" % (nch.value, max_chunks)
    return [bool(x) for x in slim[:nch.value]]


def view_block_order(counts):
    """modsx_view_block_order: counts [world, nviews] -> (source row of every list position, maxrows)."""
    counts = np.ascontiguousarray(counts, np.int32)
    world, nviews = counts.shape
    total = int(counts.sum())
    src = np.zeros(max(1, total), np.int32)
    mr = C.c_int(0)
    n = _check(lib().modsx_view_block_order(_p(counts), world, nviews, _p(src), len(src), C.byref(mr)), "view_block_order")
    return src[:n].copy(), mr.value


def shard_owner_plan(item_counts, nviews, world, rank, image_owner):
    """modsx_shard_owner_plan: the owner-only exchange of `rank` from the per-item counts (item f = image * nviews + view) ->
    dict(sends, recvs: [k, 4] = peer, image, first row, rows; jobs: [k, 4] = receive row, list row, rows, 0; recv_rows, list_rows)."""
    cnt = np.ascontiguousarray(item_counts, np.int32)
    own = np.ascontiguousarray(image_owner, np.int32)
    nimg = len(own)
    assert len(cnt) == nimg * nviews
    cap = max(1, len(cnt), nimg * world)
    sends, recvs, jobs = (np.zeros((cap, 4), np.int32) for _ in range(3))
    n = (C.c_long * 5)()
    L = lib()
    L.modsx_shard_owner_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    _check(L.modsx_shard_owner_plan(_p(cnt), nimg, nviews, world, rank, _p(own), _p(sends), _p(recvs), _p(jobs), cap, n), "shard_owner_plan")
    return {"sends": sends[:n[0]].copy(), "recvs": recvs[:n[1]].copy(), "jobs": jobs[:n[2]].copy(), "recv_rows": int(n[3]), "list_rows": int(n[4])}


def _ptr_array(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def shard_region_bytes(row_format):
    return REGION.itemsize if row_format == SHARD_ROW_REGION else 56


def shard_kp_rows(regs):
    """The SHARD_ROW_KP slice of a region array: [n, 7] f64 = x, y, a11, a12, a21, a22, s of reproj_kp."""
    k = np.asarray(regs)["reproj_kp"]
    return np.stack([k[f] for f in KP_FIELDS], 1).astype(np.float64) if len(k) else np.zeros((0, 7))


def shard_block_bytes(items, block_rows, ndesc=1, row_format=SHARD_ROW_REGION):
    L = lib()
    L.modsx_shard_block_bytes.restype = C.c_long
    return int(L.modsx_shard_block_bytes(int(items), int(block_rows), int(ndesc), int(row_format)))


def shard_block_pack(regs, descs, counts, block_rows, rc_local=0, row_format=SHARD_ROW_REGION):
    """This rank's block of one exchange (host statement of the wire format): regs in item order, descs = list of [n, 128] u8
    arrays (one per descriptor class), counts[f] per (image, view) item.  Returns the block as a uint8 array."""
    L = lib()
    L.modsx_shard_block_pack.restype = C.c_long
    regs = np.ascontiguousarray(regs, REGION)
    descs = [np.ascontiguousarray(d, np.uint8) for d in descs]
    counts = np.ascontiguousarray(counts, np.int32)
    out = np.zeros(shard_block_bytes(len(counts), block_rows, len(descs), row_format), np.uint8)
    n = _check(L.modsx_shard_block_pack(_p(regs), _ptr_array(descs), len(descs), len(regs), _p(counts), len(counts), int(rc_local),
                                        int(block_rows), int(row_format), _p(out)), "shard_block_pack")
    assert n == len(out)
    return out


def shard_blocks_unpack(blocks, world, items, block_rows, ndesc=1, cap=None, row_format=SHARD_ROW_REGION):
    """The reference's list from `world` gathered blocks (host): (regs -- REGION records, or [n, 7] f64 for SHARD_ROW_KP --,
    [desc per class], item_counts).  Raises on a failed rank; returns (None, None, need_rows) when a block was too small."""
    L = lib()
    L.modsx_shard_blocks_unpack.restype = C.c_long
    blocks = np.ascontiguousarray(blocks, np.uint8)
    cap = int(cap if cap is not None else world * block_rows)
    regs = np.zeros(max(1, cap), REGION) if row_format == SHARD_ROW_REGION else np.zeros((max(1, cap), 7), np.float64)
    descs = [np.zeros((max(1, cap), 128), np.uint8) for _ in range(ndesc)]
    cnt = np.zeros(items, np.int32)
    need = C.c_int(0)
    n = L.modsx_shard_blocks_unpack(_p(blocks), int(world), int(items), int(block_rows), int(ndesc), int(row_format), _p(regs),
                                    _ptr_array(descs), C.c_long(cap), _p(cnt), C.byref(need))
    if n == -5:      # MODSX_ERR_CAPACITY
        return None, None, need.value
    _check(n, "shard_blocks_unpack")
    return regs[:n].copy(), [d[:n].copy() for d in descs], cnt


def comm_unique_id():
    buf = C.create_string_buffer(128)
    _check(lib().modsx_comm_unique_id(buf), "comm_unique_id")
    return buf.raw


def comm_loopback_id(world):
    """Id of an in-process communicator group: `world` ranks of THIS process on one device (one context + thread each)."""
    buf = C.create_string_buffer(128)
    _check(lib().modsx_comm_loopback_id(buf, int(world)), "comm_loopback_id")
    return buf.raw


COMM_STATS = ["collectives", "bytes_gathered", "block_retries", "agreements", "lanes", "loopback", "dead", "turn_wait_us", "bytes_received",
              "exchanges"]


def comm_stats(comm):
    out = (C.c_long * len(COMM_STATS))()
    lib().modsx_comm_stats(C.c_void_p(comm), out, len(COMM_STATS))
    return dict(zip(COMM_STATS, list(out)))


def _image_dims(handle):
    st = _ImageStruct.from_address(handle)
    return st.rows, st.cols


def _handles(objs):
    """the handles (.h) of contexts, images or representations as a void* array; an empty list gives one unused entry"""
    return (C.c_void_p * max(1, len(objs)))(*[o.h for o in objs])


def match_pairs(ctxs, imgs1, imgs2, params):
    """modsx_match_pairs: a batch of pairs pipelined over several contexts (threads + streams)."""
    n = len(imgs1)
    res = (PairResult * max(1, n))()
    _check(lib().modsx_match_pairs(_handles(ctxs), len(ctxs), _handles(imgs1), _handles(imgs2), n, C.byref(params), res), "match_pairs")
    return [_unpack_pair_result(res[i]) for i in range(n)]


def match_pairs_views(ctxs, imgs1, imgs2, views, params, arrays=True):
    """modsx_match_pairs_views: a batch of multi-view pairs over several contexts, verification on helper threads.
    arrays=False returns the counts and H only (the tentative / flag arrays are released without being copied out)."""
    n = len(imgs1)
    arr = _view_array(views)
    res = (PairResult * max(1, n))()
    _check(lib().modsx_match_pairs_views(_handles(ctxs), len(ctxs), _handles(imgs1), _handles(imgs2), n, arr, len(views), C.byref(params), res),
           "match_pairs_views")
    return [_unpack_pair_result(res[i], arrays) for i in range(n)]


def match_reps(ctxs, rep1, reps2, params, classes=None, arrays=True):
    """modsx_match_reps: MatchImgReps + verification of rep1 against every representation of reps2 over several contexts.
    classes = [(detector, descriptor type, ratio), ...]; None: every non-empty class with the ratio params gives its descriptor.
    For a binary class (DESC_BRISK, DESC_FREAK, DESC_ORB) `ratio` is its DistanceThreshold; binary classes are matched only when
    they are listed."""
    n = len(reps2)
    classes = classes or []
    sel = (RepClassSel * max(1, len(classes)))()
    for i, (det, typ, ratio) in enumerate(classes):
        sel[i].detector, sel[i].desc_type, sel[i].ratio = int(det), int(typ), float(ratio)
    res = (PairResult * max(1, n))()
    _check(lib().modsx_match_reps(_handles(ctxs), len(ctxs), rep1.h, _handles(reps2), n, sel, len(classes), C.addressof(params), res), "match_reps")
    return [_unpack_pair_result(res[i], arrays) for i in range(n)]


def match_one_to_many(ctxs, img1, imgs2, steps, params, min_matches=10, arrays=True):
    """modsx_match_one_to_many (the loop of mods_multi.cpp): img1 against every image of imgs2 over the ladder `steps` (as in
    Context.match_ladder); the loop ends after the first step in which any partner reached min_matches verified.
    Returns (list of per-partner results, steps executed)."""
    n = len(imgs2)
    arr, keep = _ladder_steps(steps)
    res = (PairResult * max(1, n))()
    done = C.c_int(0)
    _check(lib().modsx_match_one_to_many(_handles(ctxs), len(ctxs), img1.h, _handles(imgs2), n, arr, len(steps), int(min_matches),
                                         C.addressof(params), res, C.byref(done)), "match_one_to_many")
    return [_unpack_pair_result(res[i], arrays) for i in range(n)], done.value


def _unpack_pair_result(res, arrays=True):
    T = res.n_unique if arrays else 0
    out = dict(n_regions=(res.n_regions1, res.n_regions2), n_tentatives=res.n_tentatives, n_unique=res.n_unique,
               n_ransac_inliers=res.n_ransac_inliers, n_verified=res.n_verified,
               ransac_samples=res.ransac_samples, ransac_lo=res.ransac_lo,
               H=np.array(list(res.H)).reshape(3, 3))
    if T > 0:
        out["tentatives"] = np.frombuffer((C.c_char * (T * TENT.itemsize)).from_address(res.tentatives),
                                          dtype=TENT, count=T).copy()
        out["ransac_inlier"] = np.frombuffer((C.c_char * T).from_address(res.ransac_inlier), np.uint8, T).astype(bool)
        out["verified"] = np.frombuffer((C.c_char * T).from_address(res.verified), np.uint8, T).astype(bool)
    else:
        out["tentatives"] = np.zeros(0, TENT)
        out["ransac_inlier"] = np.zeros(0, bool)
        out["verified"] = np.zeros(0, bool)
    lib().modsx_pair_result_release(C.byref(res))
    return out

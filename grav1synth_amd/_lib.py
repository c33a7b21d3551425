"""ctypes binding of libg1s_diff.so (include/g1s_diff.h).

The shared library is built in-tree by `__graft_entry__.build()` (or
`make -C grav1synth_amd/csrc`).  There is NO fallback: if the library is
missing, importing the compute entry points raises, loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (importing this package changes nobody's environment: the number of hardware queues the HIP runtime gives the process,
#  INTEGRATION.md section 3, is the host's setting)
LIB_PATH = os.environ.get("G1S_LIB") or os.path.join(_HERE, "libg1s_diff.so")  # (G1S_LIB: an instrumented build, tools/ only)

G1S_OK = 0
G1S_DENOISE_JOINT_CHROMA = 1
G1S_AUTO_PRIOR, G1S_AUTO_STRENGTH = 1, 2
G1S_ERR_CAPACITY = -8
ERRORS = {
    -1: "G1S_ERR_INVALID",
    -2: "G1S_ERR_DIM_MISMATCH",
    -3: "G1S_ERR_NOT_ENOUGH_FLAT",
    -4: "G1S_ERR_SOLVE",
    -5: "G1S_ERR_NO_DEVICE",
    -6: "G1S_ERR_HIP",
    -7: "G1S_ERR_STATE",
    -8: "G1S_ERR_CAPACITY",
    -9: "G1S_ERR_UNSUPPORTED",
}


class G1SFrame(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("bytes_per_sample", C.c_uint8),
        ("xdec", C.c_uint8),
        ("ydec", C.c_uint8),
        ("nplanes", C.c_uint8),
        ("data", C.c_void_p * 3),
        ("stride_bytes", C.c_size_t * 3),
        ("on_device", C.c_int32),
    ]


class G1SSegment(C.Structure):
    _fields_ = [
        ("start_time", C.c_uint64),
        ("end_time", C.c_uint64),
        ("random_seed", C.c_uint16),
        ("num_y_points", C.c_uint8),
        ("num_cb_points", C.c_uint8),
        ("num_cr_points", C.c_uint8),
        ("scaling_points_y", (C.c_uint8 * 2) * 14),
        ("scaling_points_cb", (C.c_uint8 * 2) * 10),
        ("scaling_points_cr", (C.c_uint8 * 2) * 10),
        ("scaling_shift", C.c_uint8),
        ("ar_coeff_lag", C.c_uint8),
        ("num_y_coeffs", C.c_uint8),
        ("num_uv_coeffs", C.c_uint8),
        ("ar_coeffs_y", C.c_int8 * 24),
        ("ar_coeffs_cb", C.c_int8 * 25),
        ("ar_coeffs_cr", C.c_int8 * 25),
        ("ar_coeff_shift", C.c_uint8),
        ("cb_mult", C.c_uint8),
        ("cb_luma_mult", C.c_uint8),
        ("cb_offset", C.c_uint16),
        ("cr_mult", C.c_uint8),
        ("cr_luma_mult", C.c_uint8),
        ("cr_offset", C.c_uint16),
        ("chroma_scaling_from_luma", C.c_uint8),
        ("grain_scale_shift", C.c_uint8),
        ("overlap_flag", C.c_uint8),
    ]


class G1SOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("ar_coeff_lag", C.c_uint32),
        ("luma_only", C.c_uint32),
        ("batch_frames", C.c_uint32),
        ("records_only", C.c_uint32),
    ]


class G1SStats(C.Structure):
    _fields_ = [
        ("frames", C.c_uint64),
        ("blocks", C.c_uint64),
        ("flat_blocks", C.c_uint64),
        ("ms_flat_features", C.c_double),
        ("ms_flat_select", C.c_double),
        ("ms_ar_accumulate", C.c_double),
        ("ms_total_gpu", C.c_double),
        ("launches_flat_features", C.c_uint64),
        ("launches_flat_select", C.c_uint64),
        ("launches_ar_accumulate", C.c_uint64),
        ("ms_host_fold", C.c_double),
        ("ms_residual", C.c_double),
        ("literal_blocks", C.c_uint64),
        ("ms_chain", C.c_double),
        ("chain_batches", C.c_uint64),
    ]


class G1SY4MInfo(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("bit_depth", C.c_uint32),
        ("xdec", C.c_uint32),
        ("ydec", C.c_uint32),
        ("nplanes", C.c_uint32),
        ("fps_num", C.c_int64),
        ("fps_den", C.c_int64),
    ]


class G1SFilterDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("top", C.c_uint64),
        ("bottom", C.c_uint64),
        ("left", C.c_uint64),
        ("right", C.c_uint64),
        ("width", C.c_uint64),
        ("height", C.c_uint64),
        ("alg", C.c_char * 16),
    ]


class G1SGrainOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("batch_frames", C.c_uint32),
        ("clip_to_restricted_range", C.c_uint32),
        ("mc_identity", C.c_uint32),
    ]


class G1SDenoiseOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("batch_frames", C.c_uint32),
        ("search_radius", C.c_uint32),
        ("patch_radius", C.c_uint32),
        ("strength", C.c_double),
        ("chroma_strength", C.c_double),
    ]


class G1SMeasureOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("batch_frames", C.c_uint32),
    ]


class G1SMeasureRecord(C.Structure):
    _fields_ = [
        ("n", (C.c_uint64 * 32) * 3),
        ("s1", (C.c_int64 * 32) * 3),
        ("s2", (C.c_uint64 * 32) * 3),
        ("r", (C.c_int64 * 25) * 3),
    ]


class G1SMeasureTRecord(C.Structure):
    _fields_ = [
        ("n", (C.c_uint64 * 32) * 3),
        ("x", (C.c_int64 * 32) * 3),
        ("u", (C.c_uint64 * 32) * 3),
        ("v", (C.c_uint64 * 32) * 3),
        ("c", (C.c_int64 * 25) * 3),
    ]


class G1SMeasureXRecord(C.Structure):
    # g1s_measure_xrecord_t: the temporal record's layout with the pairing where the plane is
    _fields_ = list(G1SMeasureTRecord._fields_)


G1S_MEASURE_TEMPORAL, G1S_MEASURE_CROSS = 1, 2


class G1SMeasureSRecord(C.Structure):
    # g1s_measure_srecord_t: [plane][k - 1][bin]
    _fields_ = [
        ("n", ((C.c_uint64 * 32) * 5) * 3),
        ("s1", ((C.c_int64 * 32) * 5) * 3),
        ("s2", ((C.c_uint64 * 32) * 5) * 3),
    ]


class G1SNlfOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("batch_frames", C.c_uint32),
    ]


class G1SEstimateLaunch(C.Structure):
    _fields_ = [
        ("strip_rows", C.c_uint32),
        ("row_strips", C.c_uint32),
        ("packed", C.c_int32),
        ("launched", C.c_int32),
        ("cus", C.c_int32),
        ("wgs_per_cu", C.c_int32),
    ]


class G1SNlfRecord(C.Structure):
    _fields_ = [
        ("n", (C.c_uint64 * 32) * 3),
        ("a", (C.c_uint64 * 32) * 3),
        ("q", (C.c_uint64 * 32) * 3),
    ]


class G1SNlfTRecord(C.Structure):
    _fields_ = [
        ("n", (C.c_uint64 * 32) * 3),
        ("s", (C.c_int64 * 32) * 3),
        ("q", (C.c_uint64 * 32) * 3),
    ]


class G1SNlfLRecord(C.Structure):
    _fields_ = [
        ("n", (C.c_uint64 * 46) * 3),
        ("r", (C.c_int64 * 46) * 3),
        ("s", C.c_int64 * 3),
        ("xn", (C.c_uint64 * 25) * 2),
        ("xr", (C.c_int64 * 25) * 2),
        ("ln", C.c_uint64),
        ("ls", C.c_int64),
        ("l2", C.c_uint64),
    ]


class G1SSurface(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("bytes_per_sample", C.c_uint8),
        ("xdec", C.c_uint8),
        ("ydec", C.c_uint8),
        ("nplanes", C.c_uint8),
        ("bit_depth", C.c_uint8),
        ("msb_aligned", C.c_uint8),
        ("data", C.c_void_p * 3),
        ("stride_bytes", C.c_size_t * 3),
        ("on_device", C.c_int32),
    ]


class G1SSurfaceOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("batch_frames", C.c_uint32),
    ]


NEXT_FRAME_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(G1SFrame))

# every symbol include/g1s_diff.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("g1s_diff_new", C.c_void_p, [C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, C.POINTER(G1SOpts)]),
    ("g1s_last_global_error", C.c_char_p, []),
    ("g1s_diff_frame", C.c_int, [C.c_void_p, C.POINTER(G1SFrame), C.POINTER(G1SFrame)]),
    ("g1s_diff_frames", C.c_int, [C.c_void_p, C.POINTER(G1SFrame), C.POINTER(G1SFrame), C.c_size_t]),
    ("g1s_diff_sync", C.c_int, [C.c_void_p]),
    ("g1s_diff_finish", C.c_int, [C.c_void_p, C.POINTER(G1SSegment), C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_diff_free", None, [C.c_void_p]),
    ("g1s_diff_last_error", C.c_char_p, [C.c_void_p]),
    ("g1s_record_size", C.c_size_t, [C.c_uint32] * 6),
    ("g1s_record_init", C.c_int, [C.c_void_p, C.c_size_t] + [C.c_uint32] * 6),
    ("g1s_diff_take_records", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_fold_new", C.c_void_p, [C.c_int64, C.c_int64, C.c_uint32]),
    ("g1s_fold_push", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("g1s_diff_take_latest", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_latest_size", C.c_size_t, [C.c_uint32]),
    ("g1s_shard_msg_size", C.c_size_t, [C.c_uint32, C.c_uint32]),
    ("g1s_shard_pack", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    ("g1s_shard_msg_from_latest", C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
    ("g1s_shard_msg_from_latest_at", C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t]),
    ("g1s_shard_merge", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32]),
    ("g1s_latest_from_record", C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t]),
    ("g1s_latest_from_records", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t]),
    ("g1s_usable_cpus", C.c_uint, []),
    ("g1s_shard_flush_rounds", C.c_uint, []),
    ("g1s_fold_push_latest", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]),
    ("g1s_fold_push_many", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]),
    ("g1s_fold_finish", C.c_int, [C.c_void_p, C.POINTER(G1SSegment), C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_fold_free", None, [C.c_void_p]),
    ("g1s_fold_last_error", C.c_char_p, [C.c_void_p]),
    ("g1s_format_tbl", C.c_long, [C.POINTER(G1SSegment), C.c_size_t, C.c_char_p, C.c_size_t]),
    ("g1s_write_tbl", C.c_int, [C.c_char_p, C.POINTER(G1SSegment), C.c_size_t]),
    ("g1s_parse_tbl", C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(G1SSegment), C.c_size_t, C.POINTER(C.c_size_t),
                                C.c_char_p, C.c_size_t]),
    ("g1s_tbl_segment_for", C.c_long, [C.POINTER(G1SSegment), C.c_size_t, C.c_uint64]),
    ("g1s_diff_get_stats", C.c_int, [C.c_void_p, C.POINTER(G1SStats)]),
    ("g1s_diff_set_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("g1s_diff_kernel_times", C.c_long, [C.c_void_p, C.c_char_p, C.c_size_t]),
    ("g1s_diff_frames_released", C.c_uint64, [C.c_void_p]),
    ("g1s_diff_frames_copied", C.c_uint64, [C.c_void_p, C.c_uint64]),
    ("g1s_diff_set_flat_finder", C.c_int, [C.c_void_p, C.c_int]),
    ("g1s_diff_last_record", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("g1s_record_geometry", C.c_int, [C.c_void_p] + [C.POINTER(C.c_uint32)] * 4),
    ("g1s_record_flat_mask", C.POINTER(C.c_uint8), [C.c_void_p]),
    ("g1s_record_scores", C.POINTER(C.c_float), [C.c_void_p]),
    ("g1s_record_ar_sums", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(C.c_int64)),
                                      C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.c_int64)]),
    ("g1s_record_block_stats", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(C.c_uint32)),
                                          C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_uint32))]),
    ("g1s_diff_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    ("g1s_filters_new", C.c_void_p, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("g1s_filters_len", C.c_size_t, [C.c_void_p]),
    ("g1s_filters_get", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(G1SFilterDesc)]),
    ("g1s_filters_apply", C.c_int, [C.c_void_p, C.POINTER(G1SFrame), C.POINTER(G1SFrame), C.c_char_p, C.c_size_t]),
    ("g1s_filters_apply_bd", C.c_int, [C.c_void_p, C.POINTER(G1SFrame), C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(G1SFrame), C.c_char_p,
                                        C.c_size_t]),
    ("g1s_filters_has_resize", C.c_int, [C.c_void_p]),
    ("g1s_fold_frames", C.c_uint64, [C.c_void_p]),
    ("g1s_resize_plan", C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_size_t]),
    ("g1s_resize_frame_to_host", C.c_int, [C.c_char_p, C.POINTER(G1SFrame), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
    ("g1s_filters_free", None, [C.c_void_p]),
    ("g1s_diff_run_filtered", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    ("g1s_estimate_new", C.c_void_p, [C.c_uint32, C.c_int32, C.c_uint32]),
    ("g1s_estimate_frame", C.c_int, [C.c_void_p, C.POINTER(G1SFrame)]),
    ("g1s_estimate_finish", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_estimate_set_timing", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_estimate_last_launch", C.c_int, [C.c_void_p, C.POINTER(G1SEstimateLaunch), C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_estimate_last_error", C.c_char_p, [C.c_void_p]),
    ("g1s_estimate_free", None, [C.c_void_p]),
    ("g1s_format_estimates", C.c_long, [C.POINTER(C.c_double), C.c_size_t, C.c_char_p, C.c_size_t]),
    ("g1s_nlf_new", C.c_void_p, [C.c_uint32, C.POINTER(G1SNlfOpts)]),
    ("g1s_nlf_frame", C.c_int, [C.c_void_p, C.POINTER(G1SFrame)]),
    ("g1s_nlf_finish", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_nlf_set_timing", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_nlf_last_error", C.c_char_p, [C.c_void_p]),
    ("g1s_nlf_free", None, [C.c_void_p]),
    ("g1s_nlf_sum", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("g1s_nlf_sigma", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]),
    ("g1s_nlf_strength", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
    ("g1s_denoise_curve_sigma", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("g1s_format_noise_levels", C.c_long, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_char_p, C.c_size_t]),
    ("g1s_nlf_y4m_file", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SNlfOpts), C.c_uint64, C.c_void_p, C.c_char_p, C.c_size_t]),
    ("g1s_nlf_new_temporal", C.c_void_p, [C.c_uint32, C.POINTER(G1SNlfOpts)]),
    ("g1s_nlf_cut", C.c_int, [C.c_void_p]),
    ("g1s_nlf_finish_temporal", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_nlf_temporal_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_nlf_sum_temporal", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("g1s_nlf_new_lags", C.c_void_p, [C.c_uint32, C.POINTER(G1SNlfOpts)]),
    ("g1s_nlf_finish_lags", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_nlf_lag_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_nlf_sum_lags", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("g1s_nlf_table", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]),
    ("g1s_format_noise_lags", C.c_long, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_char_p, C.c_size_t]),
    ("g1s_nlf_y4m_file_table", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SNlfOpts), C.c_uint64, C.c_uint32, C.c_uint64,
                                           C.c_void_p, C.c_char_p, C.c_size_t]),
    ("g1s_nlf_ar", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("g1s_nlf_sigma_temporal", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]),
    ("g1s_nlf_chroma_sigma_temporal", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    ("g1s_nlf_strength_temporal", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
    ("g1s_format_noise_levels_temporal", C.c_long, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_char_p, C.c_size_t]),
    ("g1s_nlf_y4m_file_temporal", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SNlfOpts), C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p,
                                              C.c_size_t]),
    ("g1s_denoise_y4m_file_auto_temporal", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32,
                                                       C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double,
                                                       C.c_uint32, C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_file_denoised_auto_temporal", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.POINTER(G1SDenoiseOpts), C.c_uint32,
                                                           C.c_uint32, C.c_char_p, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                                           C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("g1s_y4m_open", C.c_void_p, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("g1s_y4m_get_info", C.c_int, [C.c_void_p, C.POINTER(G1SY4MInfo)]),
    ("g1s_y4m_next", C.c_int, [C.c_void_p, C.POINTER(G1SFrame)]),
    ("g1s_y4m_bind", C.c_int, [C.c_void_p, C.c_void_p]),
    ("g1s_y4m_last_error", C.c_char_p, [C.c_void_p]),
    ("g1s_y4m_close", None, [C.c_void_p]),
    ("g1s_diff_y4m_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_files_filtered", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.c_char_p,
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_files_sharded", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.c_char_p,
                                              C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int),
                                              C.c_char_p, C.c_size_t]),
    ("g1s_grain_new", C.c_void_p, [C.c_uint32, C.POINTER(G1SGrainOpts)]),
    ("g1s_grain_frame", C.c_int, [C.c_void_p, C.POINTER(G1SSegment), C.POINTER(G1SFrame), C.POINTER(G1SFrame)]),
    ("g1s_grain_sync", C.c_int, [C.c_void_p]),
    ("g1s_grain_templates", C.c_int, [C.c_void_p, C.POINTER(G1SSegment), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    ("g1s_grain_gaussian_sequence", C.POINTER(C.c_int16), []),
    ("g1s_grain_set_timing", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_grain_last_error", C.c_char_p, [C.c_void_p]),
    ("g1s_grain_free", None, [C.c_void_p]),
    ("g1s_grain_y4m_file", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SGrainOpts), C.c_char_p, C.c_size_t]),
    ("g1s_denoise_new", C.c_void_p, [C.c_uint32, C.POINTER(G1SDenoiseOpts)]),
    ("g1s_denoise_new_temporal", C.c_void_p, [C.c_uint32, C.POINTER(G1SDenoiseOpts), C.c_uint32]),
    ("g1s_denoise_new_ex", C.c_void_p, [C.c_uint32, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32]),
    ("g1s_denoise_weights_ex", C.c_int, [C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("g1s_denoise_y4m_file_ex", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_file_denoised_ex", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32,
                                                C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("g1s_denoise_new_curve", C.c_void_p, [C.c_uint32, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("g1s_denoise_curve", C.c_int, [C.POINTER(G1SSegment), C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("g1s_denoise_y4m_file_curve", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int32,
                                               C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_file_denoised_curve", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32,
                                                   C.c_char_p, C.c_uint32, C.c_int32, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("g1s_denoise_new_motion", C.c_void_p, [C.c_uint32, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("g1s_denoise_motion_search", C.c_int, [C.c_void_p, C.POINTER(G1SFrame), C.POINTER(G1SFrame), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("g1s_denoise_motion_time", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("g1s_denoise_y4m_file_motion", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int32,
                                                C.c_uint32, C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_file_denoised_motion", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32,
                                                    C.c_char_p, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("g1s_denoise_y4m_file_auto", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int32,
                                              C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_file_denoised_auto", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32,
                                                  C.c_char_p, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64),
                                                  C.c_char_p, C.c_size_t]),
    ("g1s_denoise_new_gain", C.c_void_p, [C.c_uint32, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("g1s_denoise_chroma_gain", C.c_int, [C.POINTER(G1SSegment), C.c_size_t, C.c_uint32, C.c_void_p]),
    ("g1s_denoise_chroma_gain_sigma", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    ("g1s_nlf_chroma_sigma", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    ("g1s_denoise_y4m_file_chroma", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int32,
                                                C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_file_denoised_chroma", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32,
                                                    C.c_char_p, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32,
                                                    C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("g1s_denoise_new_levels", C.c_void_p, [C.c_uint32, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                            C.c_uint32, C.c_double]),
    ("g1s_denoise_level_time", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("g1s_denoise_level_kernel_time", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("g1s_denoise_y4m_file_levels", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int32,
                                                C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_file_denoised_levels", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_uint32,
                                                    C.c_char_p, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                                    C.c_double, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("g1s_denoise_drain", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("g1s_denoise_frame", C.c_int, [C.c_void_p, C.POINTER(G1SFrame), C.POINTER(G1SFrame)]),
    ("g1s_denoise_sync", C.c_int, [C.c_void_p]),
    ("g1s_denoise_set_timing", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_denoise_last_error", C.c_char_p, [C.c_void_p]),
    ("g1s_denoise_free", None, [C.c_void_p]),
    ("g1s_denoise_weights", C.c_int, [C.c_uint32, C.c_uint32, C.c_double, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("g1s_denoise_y4m_file", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SDenoiseOpts), C.c_char_p, C.c_size_t]),
    ("g1s_denoise_y4m_file_temporal", C.c_int64, [C.c_char_p, C.c_char_p, C.POINTER(G1SDenoiseOpts), C.c_uint32, C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_file_denoised_temporal", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.POINTER(G1SDenoiseOpts), C.c_uint32,
                                             C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("g1s_diff_y4m_file_denoised", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SOpts), C.POINTER(G1SDenoiseOpts),
                                             C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("g1s_measure_new", C.c_void_p, [C.c_uint32, C.POINTER(G1SMeasureOpts)]),
    ("g1s_measure_frame", C.c_int, [C.c_void_p, C.POINTER(G1SFrame), C.POINTER(G1SFrame)]),
    ("g1s_measure_finish", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_measure_sum", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("g1s_format_measure", C.c_long, [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_uint32] * 6 + [C.c_char_p, C.c_size_t]),
    ("g1s_measure_set_timing", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_measure_last_error", C.c_char_p, [C.c_void_p]),
    ("g1s_measure_free", None, [C.c_void_p]),
    ("g1s_measure_y4m_files", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SMeasureOpts), C.POINTER(C.c_int), C.c_char_p,
                                          C.c_size_t]),
    ("g1s_check_y4m_files", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SMeasureOpts), C.POINTER(G1SGrainOpts),
                                        C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    ("g1s_measure_new_temporal", C.c_void_p, [C.c_uint32, C.POINTER(G1SMeasureOpts)]),
    ("g1s_measure_cut", C.c_int, [C.c_void_p]),
    ("g1s_measure_finish_temporal", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_measure_sum_temporal", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("g1s_format_measure_temporal", C.c_long, [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_uint32] * 6 + [C.c_char_p, C.c_size_t]),
    ("g1s_measure_temporal_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_measure_y4m_files_temporal", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SMeasureOpts), C.POINTER(C.c_int),
                                                   C.c_char_p, C.c_size_t]),
    ("g1s_check_y4m_files_temporal", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SMeasureOpts),
                                                 C.POINTER(G1SGrainOpts), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    ("g1s_measure_new_modes", C.c_void_p, [C.c_uint32, C.POINTER(G1SMeasureOpts), C.c_uint32]),
    ("g1s_measure_finish_cross", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_measure_sum_cross", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("g1s_format_measure_cross", C.c_long, [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_uint32] * 5 + [C.c_char_p, C.c_size_t]),
    ("g1s_measure_cross_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_measure_chroma_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("g1s_measure_y4m_files_modes", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SMeasureOpts),
                                                C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    ("g1s_check_y4m_files_modes", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(G1SMeasureOpts),
                                              C.POINTER(G1SGrainOpts), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    ("g1s_measure_new_scales", C.c_void_p, [C.c_uint32, C.POINTER(G1SMeasureOpts), C.c_uint32]),
    ("g1s_measure_finish_scales", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("g1s_measure_sum_scales", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("g1s_format_measure_scales", C.c_long, [C.c_void_p] * 4 + [C.c_uint64, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]),
    ("g1s_measure_scales_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_measure_y4m_files_scales", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                                 C.POINTER(G1SMeasureOpts), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    ("g1s_check_y4m_files_scales", C.c_int64, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                               C.POINTER(G1SMeasureOpts), C.POINTER(G1SGrainOpts), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    ("g1s_surface_new", C.c_void_p, [C.c_uint32, C.POINTER(G1SSurfaceOpts)]),
    ("g1s_surface_unpack", C.c_int, [C.c_void_p, C.POINTER(G1SSurface), C.POINTER(G1SFrame)]),
    ("g1s_surface_pack", C.c_int, [C.c_void_p, C.POINTER(G1SFrame), C.POINTER(G1SSurface)]),
    ("g1s_surface_sync", C.c_int, [C.c_void_p]),
    ("g1s_surface_set_timing", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("g1s_surface_last_error", C.c_char_p, [C.c_void_p]),
    ("g1s_surface_free", None, [C.c_void_p]),
]

_lib = None


def lib() -> C.CDLL:
    """Load libg1s_diff.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C grav1synth_amd/csrc). "
            "grav1synth_amd has no CPU fallback for the diff path."
        )
    # PyTorch-ROCm ships its own libamdhip64: it must be the HIP runtime of the process (device pointers of
    # torch tensors are handed to the kernels), so it has to be mapped before libg1s_diff.so asks the
    # dynamic linker for that soname -- two runtimes in one process do not see each other's device state.
    try:
        import torch  # noqa: F401
    except ImportError:  # host-only use (fold, .tbl writer): the system HIP runtime will do
        pass
    L = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(L, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


class G1SError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{ERRORS.get(code, code)}: {message}")
        self.code = code
        self.message = message

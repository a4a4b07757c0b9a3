"""ctypes view of include/svtvp9_hip.h -- used by tests/, bench.py and __graft_entry__.py.

This module only declares the C structs of the public header and loads the product library
(svt-vp9_amd/libsvtvp9_hip.so).  It contains no compute and no fallback: if the library (or, for a
compute call, a GPU) is missing, the call fails loudly.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SVT_HIP_LIB: experiment aid (tools/build_variant.sh), never set by the tests or the bench contract run
LIB_PATH = os.environ.get("SVT_HIP_LIB") or os.path.join(HERE, "libsvtvp9_hip.so")

SVT_ME_PU_COUNT = 85


class Plane(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("stride", C.c_int32), ("origin_x", C.c_int32), ("origin_y", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32)]


class PaPicture(C.Structure):
    _fields_ = [("full", Plane), ("quarter", Plane), ("sixteenth", Plane)]


class MeParams(C.Structure):
    _fields_ = [(n, C.c_uint8) for n in (
        "num_ref_lists", "temporal_layer_index", "hierarchical_levels", "enable_hme_flag",
        "enable_hme_level_0_flag", "enable_hme_level_1_flag", "enable_hme_level_2_flag", "cu8x8_mode",
        "cu16x16_mode", "same_ref_poc", "rate_control_mode", "fractional_search_method",
        "fractional_search_model", "fractional_search64x64", "single_hme_quadrant", "search_area_width",
        "search_area_height")] + [
        ("number_hme_search_region_in_width", C.c_uint16), ("number_hme_search_region_in_height", C.c_uint16),
        ("hme_level0_total_search_area_width", C.c_uint16), ("hme_level0_total_search_area_height", C.c_uint16),
        ("hme_level0_search_area_in_width_array", C.c_uint16 * 2),
        ("hme_level0_search_area_in_height_array", C.c_uint16 * 2),
        ("hme_level1_search_area_in_width_array", C.c_uint16 * 2),
        ("hme_level1_search_area_in_height_array", C.c_uint16 * 2),
        ("hme_level2_search_area_in_width_array", C.c_uint16 * 2),
        ("hme_level2_search_area_in_height_array", C.c_uint16 * 2)]


# numpy view of svt_me_pu_result (40 bytes)
ME_RESULT_DTYPE = np.dtype([("x_mv_l0", "<i2"), ("y_mv_l0", "<i2"), ("x_mv_l1", "<i2"), ("y_mv_l1", "<i2"),
                            ("dist0", "<u4"), ("dir0", "<u4"), ("dist1", "<u4"), ("dir1", "<u4"),
                            ("dist2", "<u4"), ("dir2", "<u4"), ("total", "u1"), ("pad", "u1", (7,))])
assert ME_RESULT_DTYPE.itemsize == 40


class SadLoopJob(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("ref_off", C.c_uint64), ("src_stride", C.c_int32),
                ("ref_stride", C.c_int32), ("ref_stride_raw", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("search_w", C.c_int32), ("search_h", C.c_int32)]


SAD_LOOP_JOB_DTYPE = np.dtype([("src_off", "<u8"), ("ref_off", "<u8"), ("src_stride", "<i4"), ("ref_stride", "<i4"),
                               ("ref_stride_raw", "<i4"), ("width", "<i4"), ("height", "<i4"),
                               ("search_w", "<i4"), ("search_h", "<i4")], align=True)
SAD_LOOP_RESULT_DTYPE = np.dtype([("best_sad", "<u4"), ("x", "<i2"), ("y", "<i2")])


class QuantTables(C.Structure):
    _fields_ = [("zbin", C.c_int16 * 2), ("round", C.c_int16 * 2), ("quant", C.c_int16 * 2),
                ("quant_shift", C.c_int16 * 2), ("dequant", C.c_int16 * 2)]


QUANT_DTYPE = np.dtype([("zbin", "<i2", (2,)), ("round", "<i2", (2,)), ("quant", "<i2", (2,)),
                        ("quant_shift", "<i2", (2,)), ("dequant", "<i2", (2,))])

TQ_BLOCK_DTYPE = np.dtype([("src_off", "<u4"), ("pred_off", "<u4"), ("recon_off", "<u4"), ("coeff_off", "<u4"),
                           ("iscan_off", "<u4"), ("src_stride", "<u2"), ("pred_stride", "<u2"), ("recon_stride", "<u2"),
                           ("tx_size", "u1"), ("tx_type", "u1"), ("qtab", "u1"), ("do_recon", "u1"),
                           ("partial32", "u1"), ("pad", "u1", (1,))])
assert TQ_BLOCK_DTYPE.itemsize == 32

LF_MASK_DTYPE = np.dtype([("left_y", "<u8", (4,)), ("above_y", "<u8", (4,)), ("int_4x4_y", "<u8"),
                          ("left_uv", "<u2", (4,)), ("above_uv", "<u2", (4,)), ("int_4x4_uv", "<u2"),
                          ("lfl_y", "u1", (64,))], align=True)


LF_MODE_INFO_DTYPE = np.dtype([("sb_type", "u1"), ("tx_size", "u1"), ("skip", "u1"), ("is_inter", "u1"),
                               ("filter_level", "u1"), ("pad", "u1", (3,))])
assert LF_MODE_INFO_DTYPE.itemsize == 8


MC_MODE_INFO_DTYPE = np.dtype([("mv_row", "<i2", (2,)), ("mv_col", "<i2", (2,)), ("ref_list", "i1", (2,)), ("bw8", "u1"), ("bh8", "u1")])
assert MC_MODE_INFO_DTYPE.itemsize == 12


RATE_BLOCK_DTYPE = np.dtype([("coeff_off", "<u4"), ("scan_off", "<u4"), ("eob", "<u2"), ("tx_size", "u1"), ("plane_type", "u1"),
                             ("is_inter", "u1"), ("ctx", "u1"), ("pad", "u1", (2,))])
assert RATE_BLOCK_DTYPE.itemsize == 16
RATE_TABLES_DTYPE = np.dtype([("token_costs", "<u4", (4, 2, 2, 6, 2, 6, 12)), ("value_cost", "<i4", (133,)), ("cat6_low_cost", "<u2", (256,)),
                              ("cat6_high_cost", "<u2", (64,)), ("pad", "<u2", (2,))])
assert RATE_TABLES_DTYPE.itemsize == 56472, RATE_TABLES_DTYPE.itemsize


class LfThresh(C.Structure):
    _fields_ = [("mblim", C.c_uint8 * 64), ("lim", C.c_uint8 * 64), ("hev_thr", C.c_uint8 * 64)]


class YuvPlanes(C.Structure):
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_stride", C.c_int32),
                ("uv_stride", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class McHostRef(C.Structure):
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_stride", C.c_int32), ("uv_stride", C.c_int32),
                ("org_x", C.c_int32), ("org_y", C.c_int32)]


class McPicture(C.Structure):
    _fields_ = [("d_mi", C.c_void_p), ("mi_stride", C.c_int32), ("mi_rows", C.c_int32), ("mi_cols", C.c_int32),
                ("ref", YuvPlanes * 2), ("pred", YuvPlanes), ("use_subpel", C.c_int32)]


class MeSbStatsParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pic_width", "pic_height", "input_resolution", "temporal_layer_index", "slice_type", "run_part2",
                                         "rate_control_mode")]


ME_SB_STATS_DTYPE = np.dtype([("check1", "u1"), ("pm_check1", "u1"), ("check2", "u1"), ("low_dist_logo", "u1"), ("inter_idx", "<u2"), ("intra_idx", "<u2")])
assert ME_SB_STATS_DTYPE.itemsize == 8

class TqPicGeom(C.Structure):
    _fields_ = [("src_off", C.c_uint32 * 3), ("pred_off", C.c_uint32 * 3), ("recon_off", C.c_uint32 * 3), ("src_stride", C.c_uint16 * 2),
                ("pred_stride", C.c_uint16 * 2), ("recon_stride", C.c_uint16 * 2), ("coeff_base", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                ("recon_set", C.c_uint8), ("do_recon", C.c_uint8), ("pic", C.c_uint8), ("pad", C.c_uint8 * 1)]


class EncdecFlagsConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("enc_mode", "tune", "temporal_layer_index", "is_used_as_reference", "recon_file", "loop_filter")]


class EncdecFlags(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("limit_intra", "allow_enc_dec_mismatch", "do_recon", "apply_loop_filter", "pad_reference")]


class EncdecPicture(C.Structure):
    _fields_ = [("d_mc_mi", C.c_void_p), ("d_lf_mi", C.c_void_p), ("src", YuvPlanes), ("ref", YuvPlanes * 2), ("pred", YuvPlanes), ("recon", YuvPlanes),
                ("d_qcoeff", C.c_void_p), ("d_dqcoeff", C.c_void_p), ("d_eob_map", C.c_void_p), ("d_lfm", C.c_void_p), ("d_nz", C.c_void_p),
                ("use_subpel", C.c_int32), ("no_pad", C.c_int32), ("has_intra", C.c_int32), ("pad_", C.c_int32)]


SB_COEFFS = 6144


class TokPicture(C.Structure):
    _fields_ = [("d_lf_mi", C.c_void_p), ("d_qcoeff", C.c_void_p), ("d_eob_map", C.c_void_p), ("d_tokens", C.c_void_p), ("capacity", C.c_uint32),
                ("pad_", C.c_uint32), ("d_tok_off", C.c_void_p), ("d_sb_off", C.c_void_p), ("d_counts", C.c_void_p)]


TOK_COUNTS = 6912
TOK_NONE = 0xFFFFFFFF


# bool coder (svt_bool_tables / svt_bool_segment / svt_bool_stream of include/svtvp9_hip.h)
BOOL_TABLES_DTYPE = np.dtype([("coef_probs", "u1", (576 * 3,)), ("pareto", "u1", (255, 8)), ("cat_probs", "u1", (6, 14))])
assert BOOL_TABLES_DTYPE.itemsize == 576 * 3 + 255 * 8 + 6 * 14
BOOL_SEGMENT_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("kind", "<u4")])
BOOL_MAX_PER_TOKEN = 22
BOOL_SIZE_OVERFLOW = 0xFFFFFFFF
BOOL_MAX_STREAMS = 32


class BoolStream(C.Structure):
    _fields_ = [("d_tokens", C.c_void_p), ("d_bools", C.c_void_p), ("d_segments", C.c_void_p), ("d_n_tokens", C.c_void_p), ("n_segments", C.c_uint32),
                ("n_tokens", C.c_uint32), ("max_bools", C.c_uint32), ("capacity", C.c_uint32), ("d_bytes", C.c_void_p), ("d_size", C.c_void_p)]


# forward coefficient-probability update (svt_cu_result / svt_cu_picture of include/svtvp9_hip.h)
CU_ROWS, CU_PROBS, CU_ENTRIES, CU_MAX_PER_ENTRY, CU_PREFIX_MAX, CU_SUFFIX_MAX, CU_MAX_PICS = 576, 1728, 396, 12, 8, 208, 32
CU_SECTION_MAX = 4 * (1 + CU_ENTRIES * CU_MAX_PER_ENTRY)
CU_RESULT_DTYPE = np.dtype([("updated", "<u4", (4,)), ("sent", "<u4", (4,)), ("hdr_bools", "<u4"), ("tokens", "<u4"), ("savings", "<i8", (4,))])


class CuPicture(C.Structure):
    _fields_ = [("d_tokens", C.c_void_p), ("d_n_tokens", C.c_void_p), ("d_counts", C.c_void_p), ("d_old_probs", C.c_void_p), ("d_eob_branch", C.c_void_p),
                ("d_probs", C.c_void_p), ("d_hdr_bools", C.c_void_p), ("d_n_hdr_bools", C.c_void_p), ("d_segment", C.c_void_p), ("d_result", C.c_void_p),
                ("n_tokens", C.c_uint32), ("max_tokens", C.c_uint32), ("n_prefix", C.c_uint16), ("n_suffix", C.c_uint16), ("prefix", C.c_uint16 * CU_PREFIX_MAX),
                ("suffix", C.c_uint16 * CU_SUFFIX_MAX), ("pad_", C.c_uint32)]


assert C.sizeof(CuPicture) == 528 and CU_RESULT_DTYPE.itemsize == 72


# key-frame mode-info stage (svt_modes_tables / svt_modes_picture of include/svtvp9_hip.h)
MODES_TABLES_DTYPE = np.dtype([("kf_y_mode_prob", "u1", (10, 10, 9)), ("kf_uv_mode_prob", "u1", (10, 9)), ("kf_partition_probs", "u1", (16, 3)), ("skip_probs", "u1", (3,))])
assert MODES_TABLES_DTYPE.itemsize == 900 + 90 + 48 + 3
MODES_BAD_GRID = 0xFFFFFFFF
MODES_UNIT_BOOLS = 48


class ModesPicture(C.Structure):
    _fields_ = [("d_lf_mi", C.c_void_p), ("d_eob_map", C.c_void_p), ("d_tok_off", C.c_void_p), ("d_bools", C.c_void_p), ("d_segments", C.c_void_p),
                ("d_n_bools", C.c_void_p), ("capacity", C.c_uint32), ("pad_", C.c_uint32)]


# inter mode-info stage (svt_modes_inter_tables / svt_mi_inter_ext / svt_modes_inter_picture of include/svtvp9_hip.h)
MODES_MV_COMP_DTYPE = np.dtype([("sign", "u1"), ("classes", "u1", (10,)), ("class0", "u1", (1,)), ("bits", "u1", (10,)), ("class0_fp", "u1", (2, 3)), ("fp", "u1", (3,)),
                                ("class0_hp", "u1"), ("hp", "u1")])
MODES_INTER_TABLES_DTYPE = np.dtype([("partition_prob", "u1", (16, 3)), ("skip_probs", "u1", (3,)), ("intra_inter_prob", "u1", (4,)), ("comp_inter_prob", "u1", (5,)),
                                     ("single_ref_prob", "u1", (5, 2)), ("comp_ref_prob", "u1", (5,)), ("y_mode_prob", "u1", (4, 9)), ("uv_mode_prob", "u1", (10, 9)),
                                     ("inter_mode_probs", "u1", (7, 3)), ("mv_joints", "u1", (3,)), ("mv_comps", MODES_MV_COMP_DTYPE, (2,))])
assert MODES_MV_COMP_DTYPE.itemsize == 33 and MODES_INTER_TABLES_DTYPE.itemsize == 291
MI_INTER_EXT_DTYPE = np.dtype([("ref_mv_row", "<i2", (2,)), ("ref_mv_col", "<i2", (2,)), ("ref_frame", "u1", (2,)), ("mode", "u1"), ("mode_context", "u1")])
assert MI_INTER_EXT_DTYPE.itemsize == 12
MODES_INTER_UNIT_BOOLS = 111
MODES_SINGLE_REFERENCE, MODES_COMPOUND_REFERENCE, MODES_REFERENCE_SELECT = 0, 1, 2


class ModesInterPicture(C.Structure):
    _fields_ = [("d_lf_mi", C.c_void_p), ("d_eob_map", C.c_void_p), ("d_tok_off", C.c_void_p), ("d_bools", C.c_void_p), ("d_segments", C.c_void_p),
                ("d_n_bools", C.c_void_p), ("capacity", C.c_uint32), ("pad_", C.c_uint32), ("d_mc_mi", C.c_void_p), ("d_ext", C.c_void_p),
                ("reference_mode", C.c_uint8), ("allow_hp", C.c_uint8), ("comp_fixed_ref", C.c_uint8), ("comp_var_ref", C.c_uint8 * 2),
                ("ref_frame_sign_bias", C.c_uint8 * 4), ("pad2_", C.c_uint8 * 7)]


# MV-reference derivation (svt_mvref_cand / svt_mvrefs_picture of include/svtvp9_hip.h)
MVREF_CAND_DTYPE = np.dtype([("mv_row", "<i2", (3, 2)), ("mv_col", "<i2", (3, 2)), ("count", "u1", (3,)), ("mode_context", "u1"), ("pad", "u1", (4,))])
assert MVREF_CAND_DTYPE.itemsize == 32


class MvrefsPicture(C.Structure):
    _fields_ = [("d_lf_mi", C.c_void_p), ("d_mc_mi", C.c_void_p), ("d_ext", C.c_void_p), ("d_ext_out", C.c_void_p), ("d_cand", C.c_void_p), ("d_status", C.c_void_p),
                ("ref_mask", C.c_uint8), ("restrict_ref_mvs", C.c_uint8), ("ref_frame_sign_bias", C.c_uint8 * 4), ("pad_", C.c_uint8 * 2)]


# inter mode labelling (svt_md_inter_picture of include/svtvp9_hip.h)
class MdInterPicture(C.Structure):
    _fields_ = [("d_lf_mi", C.c_void_p), ("d_mc_mi", C.c_void_p), ("d_ext_out", C.c_void_p), ("d_cand", C.c_void_p), ("d_status", C.c_void_p),
                ("list_ref_frame", C.c_uint8 * 2), ("ref_frame_sign_bias", C.c_uint8 * 4), ("restrict_ref_mvs", C.c_uint8), ("allow_hp", C.c_uint8),
                ("reference_mode", C.c_uint8), ("comp_fixed_ref", C.c_uint8), ("comp_var_ref", C.c_uint8 * 2), ("ref_mask", C.c_uint8), ("pad_", C.c_uint8 * 3)]


assert C.sizeof(MdInterPicture) == 56

# frame stage (svt_frame_params / svt_frame_packet / svt_frame_entry of include/svtvp9_hip.h)
FRAME_HEADER_MAX = 56
FRAME_SIZE_NONE = 0xFFFFFFFF
FRAME_MAX_PICS = 32
FRAME_ENTRY_DTYPE = np.dtype([("offset", "<u4"), ("size", "<u4")])


class FrameParams(C.Structure):
    _fields_ = [("frame_type", C.c_uint8), ("show_frame", C.c_uint8), ("error_resilient_mode", C.c_uint8), ("intra_only", C.c_uint8),
                ("reset_frame_context", C.c_uint8), ("refresh_frame_context", C.c_uint8), ("frame_parallel_decoding_mode", C.c_uint8),
                ("frame_context_idx", C.c_uint8), ("refresh_frame_mask", C.c_uint8), ("ref_dpb_index", C.c_uint8 * 3), ("ref_frame_sign_bias", C.c_uint8 * 4),
                ("allow_hp", C.c_uint8), ("reference_mode", C.c_uint8), ("allow_comp_inter_inter", C.c_uint8), ("color_space", C.c_uint8),
                ("color_range", C.c_uint8), ("pad0_", C.c_uint8 * 3), ("width", C.c_int32), ("height", C.c_int32), ("render_width", C.c_int32),
                ("render_height", C.c_int32), ("filter_level", C.c_uint8), ("sharpness_level", C.c_uint8), ("mode_ref_delta_enabled", C.c_uint8),
                ("mode_ref_delta_update", C.c_uint8), ("ref_deltas", C.c_int8 * 4), ("mode_deltas", C.c_int8 * 2), ("last_ref_deltas", C.c_int8 * 4),
                ("last_mode_deltas", C.c_int8 * 2), ("base_qindex", C.c_uint8), ("y_dc_delta_q", C.c_int8), ("uv_dc_delta_q", C.c_int8),
                ("uv_ac_delta_q", C.c_int8), ("pad1_", C.c_uint8 * 4)]


class FramePacket(C.Structure):
    _fields_ = [("d_tile", C.c_void_p), ("d_tile_size", C.c_void_p), ("tile_capacity", C.c_uint32), ("header_len", C.c_uint8), ("trailer_len", C.c_uint8),
                ("header", C.c_uint8 * FRAME_HEADER_MAX), ("trailer", C.c_uint8 * 4), ("pad_", C.c_uint8 * 6)]


assert C.sizeof(FrameParams) == 64 and C.sizeof(FramePacket) == 88 and FRAME_ENTRY_DTYPE.itemsize == 8
FRAME_UNCOMPRESSED_MAX = 27


class FramePartsPacket(C.Structure):  # svt_frame_parts_packet: a packet whose compressed header is a device stream too
    _fields_ = [("d_compressed", C.c_void_p), ("d_compressed_size", C.c_void_p), ("d_tile", C.c_void_p), ("d_tile_size", C.c_void_p),
                ("compressed_capacity", C.c_uint32), ("tile_capacity", C.c_uint32), ("size_bit", C.c_uint16), ("header_len", C.c_uint8), ("trailer_len", C.c_uint8),
                ("header", C.c_uint8 * FRAME_UNCOMPRESSED_MAX), ("trailer", C.c_uint8 * 4), ("pad_", C.c_uint8 * 5)]


assert C.sizeof(FramePartsPacket) == 80


# svt_frame_read_info: what svt_hip_frame_read_header_host returns
class FrameReadInfo(C.Structure):
    _fields_ = [("params", FrameParams), ("uncompressed_bytes", C.c_uint32), ("compressed_bytes", C.c_uint32), ("show_existing_frame", C.c_uint8),
                ("show_existing_slot", C.c_uint8), ("interp_filter", C.c_uint8), ("tx_mode", C.c_uint8), ("needs_backward_adaptation", C.c_uint8),
                ("lossless", C.c_uint8), ("pad_", C.c_uint8 * 2)]


assert C.sizeof(FrameReadInfo) == 80


class TileReadParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("mi_stride", C.c_int32), ("intra_only", C.c_uint8), ("reference_mode", C.c_uint8), ("allow_hp", C.c_uint8),
                ("restrict_ref_mvs", C.c_uint8), ("interp_filter", C.c_uint8), ("lossless", C.c_uint8), ("filter_level", C.c_uint8), ("mode_ref_delta_enabled", C.c_uint8),
                ("ref_deltas", C.c_int8 * 4), ("mode_deltas", C.c_int8 * 2), ("ref_frame_sign_bias", C.c_uint8 * 4), ("list_ref_frame", C.c_uint8 * 2)]


TILE_READ_RESULT_DTYPE = np.dtype([(n, "<u4") for n in ("leaves", "inter_leaves", "skipped_leaves", "tokens", "tile_bytes", "past_end", "odd_candidates", "pad")])
assert C.sizeof(TileReadParams) == 32 and TILE_READ_RESULT_DTYPE.itemsize == 32
READ_FILTER_REGULAR, READ_FILTER_SMOOTH, READ_FILTER_SHARP, READ_FILTER_BILINEAR, READ_FILTER_SWITCHABLE = range(5)
ERR_BAD_PARAMETER, ERR_UNSUPPORTED = -1, -4

# svt_ois_block (12 bytes): one open-loop intra search record; SVT_OIS_PER_SB per SB (4 x 32x32, 16 x 16x16, 64 x 8x8, 256 x 4x4, z-order)
OIS_BLOCK_DTYPE = np.dtype([("sad", "<u4"), ("uv_sad", "<u4"), ("mode", "u1"), ("uv_mode", "u1"), ("pad", "u1", (2,))])
assert OIS_BLOCK_DTYPE.itemsize == 12
OIS_PER_SB = 340
OIS_NONE = 0xFFFFFFFF


class MdMixedPicture(C.Structure):  # svt_md_mixed_picture: device pointers of one picture of svt_hip_md_mixed_batch_device
    _fields_ = [("d_results", C.c_void_p), ("d_ois", C.c_void_p), ("d_mc_mi", C.c_void_p), ("d_lf_mi", C.c_void_p)]

# every symbol include/svtvp9_hip.h declares
EXPORTS = [
    "svt_hip_sb_count", "svt_hip_input_resolution", "svt_hip_me_params_derive", "svt_hip_me_params_preset", "svt_hip_ctx_create", "svt_hip_ctx_create_on_stream", "svt_hip_ctx_create_cu_mask", "svt_hip_ctx_stream",
    "svt_hip_ctx_destroy", "svt_hip_ctx_synchronize", "svt_hip_last_error", "svt_hip_last_kernel_ms",
    "svt_hip_mem_alloc", "svt_hip_mem_free", "svt_hip_mem_upload_2d", "svt_hip_mem_upload_2d_async", "svt_hip_mem_upload_planes_async", "svt_hip_mem_download", "svt_hip_mem_set",
    "svt_hip_ctx_marker_record", "svt_hip_ctx_marker_query", "svt_hip_ctx_marker_wait", "svt_hip_minigop_split",
    "svt_hip_me_picture_device", "svt_hip_me_batch_device", "svt_hip_me_batch_layers_device", "svt_hip_me_picture", "svt_hip_sad_loop_batch_device",
    "svt_hip_me_zz_sad_device", "svt_hip_me_similar_collocated", "svt_hip_me_sb_stats_device", "svt_hip_pa_prepare_batch_device", "svt_hip_pa_mean_variance_device",
    "svt_hip_quant_tables_init", "svt_hip_tq_batch_device", "svt_hip_tq_batch_dist_device", "svt_hip_tq_rd_batch_device", "svt_hip_tq_rd_batch_multi_device", "svt_hip_rate_scan4x4_table", "svt_hip_tq_batch", "svt_hip_lf_thresh_init", "svt_hip_lf_level_from_q",
    "svt_hip_lf_frame_device", "svt_hip_lf_batch_device", "svt_hip_lf_frame", "svt_hip_lf_build_masks",
    "svt_hip_inter_pred_batch_device", "svt_hip_inter_pred_frame", "svt_hip_ref_pad_batch_device", "svt_hip_coeff_rate_batch_device", "svt_hip_coeff_rate_batch",
    "svt_hip_gop_owner", "svt_hip_gop_assign", "svt_hip_minigop_reference_source", "svt_hip_device_set_create", "svt_hip_device_set_size",
    "svt_hip_device_set_ctx", "svt_hip_device_set_destroy", "svt_hip_ref_handoff_device",
    "svt_ivf_stream_header", "svt_ivf_packetize",
    "svt_hip_tq_blocks_from_grid", "svt_hip_vp9_iscan_tables", "svt_hip_vp9_qindex_from_qp", "svt_hip_vp9_dc_step", "svt_hip_vp9_ac_step",
    "svt_hip_quant_tables_for_qindex", "svt_hip_encdec_flags_derive", "svt_hip_encdec_work_create", "svt_hip_encdec_work_destroy",
    "svt_hip_encdec_batch_device", "svt_hip_encdec_intra_device", "svt_hip_md_intra_default_device", "svt_hip_encdec_work_status", "svt_hip_encdec_work_download", "svt_hip_md_default_batch_device",
    "svt_hip_md_default_picture", "svt_hip_lf_build_masks_device", "svt_hip_ctx_wait_marker", "svt_hip_host_alloc", "svt_hip_host_free",
    "svt_hip_mem_download_2d_async", "svt_hip_mem_copy_2d_device", "svt_hip_encdec_work_set_stage_hook", "svt_hip_me_params_same_launch", "svt_hip_me_kernel_instance", "svt_hip_ctx_set_intra_workgroups", "svt_hip_ctx_warm", "svt_hip_ctx_warm_scratch", "svt_hip_lf_reserve",
    "svt_hip_me_last_instance", "svt_hip_me_lds_bytes", "svt_hip_vp9_layer_qindex", "svt_hip_mem_upload_2d_direct", "svt_hip_mem_upload_wait", "svt_hip_host_unregister_all", "svt_hip_host_registry_retain", "svt_hip_host_registry_release",
    "svt_hip_intra_search_device", "svt_hip_md_intra_search_device", "svt_hip_md_intra_search_picture",
    "svt_hip_intra_search_batch_device", "svt_hip_md_mixed_batch_device", "svt_hip_md_mixed_picture",
    "svt_hip_pa_noise_params_derive", "svt_hip_pa_noise_batch_device", "svt_hip_pa_histogram_batch_device", "svt_hip_pa_chroma_mean_batch_device",
    "svt_hip_vp9_scan_tables", "svt_hip_tokenize_blocks_device", "svt_hip_tokenize_blocks", "svt_hip_tokenize_blocks_host", "svt_hip_tokenize_batch_device", "svt_hip_tokenize_picture",
    "svt_hip_tokenize_capacity",
    "svt_hip_boolcode_set_tables", "svt_hip_boolcode_batch_device", "svt_hip_boolcode", "svt_hip_boolcode_host", "svt_hip_boolcode_capacity", "svt_hip_boolcode_bools_capacity",
    "svt_hip_boolcode_geometry", "svt_hip_boolcode_batch_tables_device",
    "svt_hip_coef_update_batch_device", "svt_hip_coef_update_picture", "svt_hip_coef_update_bools_capacity", "svt_hip_coef_update_geometry",
    "svt_hip_coef_update_cost_table", "svt_hip_coef_update_remap_tables",
    "svt_hip_frame_header_parts_host", "svt_hip_frame_header_coef_host", "svt_hip_frame_read_header_coef_host",
    "svt_hip_modes_set_tables", "svt_hip_modes_kf_batch_device", "svt_hip_modes_kf_picture", "svt_hip_modes_segments", "svt_hip_modes_bools_capacity",
    "svt_hip_modes_inter_set_tables", "svt_hip_modes_inter_batch_device", "svt_hip_modes_inter_picture", "svt_hip_modes_inter_bools_capacity",
    "svt_hip_mvrefs_batch_device", "svt_hip_mvrefs_picture",
    "svt_hip_md_inter_modes_batch_device", "svt_hip_md_inter_modes_picture",
    "svt_hip_frame_header_host", "svt_hip_frame_show_existing_host", "svt_hip_frame_batch_device", "svt_hip_frame_assemble_host", "svt_hip_frame_geometry",
    "svt_hip_recon_batch_device", "svt_hip_decode_batch_device", "svt_hip_decode_mixed_batch_device", "svt_hip_decode_intra_device", "svt_hip_frame_read_header_host", "svt_hip_tile_read_kf_host", "svt_hip_tile_read_host", "svt_hip_frame_read_host",
    "svt_hip_entropy_limits_worst", "svt_hip_entropy_work_bytes", "svt_hip_entropy_work_create", "svt_hip_entropy_work_destroy", "svt_hip_entropy_batch_device",
    "svt_hip_entropy_work_set_stage_hook", "svt_hip_entropy_work_buffers", "svt_hip_entropy_picture", "svt_hip_entropy_gate_host", "svt_hip_entropy_deliverable",
    "svt_hip_compound_refs_from_sign_bias",
    "svt_hip_frame_header_uncompressed_host", "svt_hip_frame_parts_batch_device", "svt_hip_frame_assemble_parts_host",
    "svt_hip_entropy_work_set_coef_update", "svt_hip_entropy_coef_update_bytes", "svt_hip_entropy_work_coef_buffers", "svt_hip_entropy_picture_coef",
    "svt_hip_frame_read_coef_host",
]

_lib = None


def load():
    """Load the product library.  Raises if it has not been built -- there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # In a process that also uses PyTorch, torch must load ITS HIP runtime first: the product library is linked against
        # the system's libamdhip64, and whichever copy is loaded second finds no device ("no ROCm-capable device" on either
        # side).  Plain C hosts are not affected.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.svt_hip_last_error.restype = C.c_char_p
        _lib.svt_hip_ctx_stream.restype = C.c_void_p
        _lib.svt_hip_ctx_stream.argtypes = [C.c_void_p]
        _lib.svt_hip_last_kernel_ms.restype = C.c_float
        _lib.svt_hip_last_kernel_ms.argtypes = [C.c_void_p]
        _lib.svt_hip_lf_thresh_init.restype = None
        _lib.svt_hip_vp9_iscan_tables.restype = C.POINTER(C.c_int16)
        _lib.svt_hip_vp9_iscan_tables.argtypes = [C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_int32)]
        _lib.svt_hip_vp9_scan_tables.restype = C.POINTER(C.c_int16)
        _lib.svt_hip_vp9_scan_tables.argtypes = [C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_int32)]
        _lib.svt_hip_tokenize_capacity.restype = C.c_uint32
        _lib.svt_hip_boolcode_capacity.restype = C.c_uint32
        _lib.svt_hip_boolcode_capacity.argtypes = [C.c_uint32]
        _lib.svt_hip_boolcode_bools_capacity.restype = C.c_uint32
        _lib.svt_hip_boolcode_bools_capacity.argtypes = [C.c_uint32]
        _lib.svt_hip_boolcode_geometry.restype = None
        _lib.svt_hip_boolcode_batch_tables_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        _lib.svt_hip_coef_update_batch_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        _lib.svt_hip_coef_update_picture.argtypes = [C.c_void_p, C.c_void_p]
        _lib.svt_hip_coef_update_bools_capacity.restype = C.c_uint32
        _lib.svt_hip_coef_update_geometry.restype = None
        _lib.svt_hip_coef_update_cost_table.restype = C.POINTER(C.c_uint16)
        _lib.svt_hip_coef_update_remap_tables.restype = None
        _lib.svt_hip_coef_update_remap_tables.argtypes = [C.c_void_p, C.c_void_p]
        _lib.svt_hip_frame_header_parts_host.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32)]
        _lib.svt_hip_frame_header_coef_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _lib.svt_hip_frame_read_header_coef_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.svt_hip_modes_segments.restype = C.c_uint32
        _lib.svt_hip_modes_bools_capacity.restype = C.c_uint32
        _lib.svt_hip_modes_inter_bools_capacity.restype = C.c_uint32
        _u32 = C.c_uint32
        _lib.svt_hip_boolcode_host.argtypes = [C.c_void_p, C.c_void_p, _u32, C.c_void_p, _u32, C.c_void_p, _u32, C.c_void_p, _u32, C.POINTER(_u32)]
        _lib.svt_hip_boolcode.argtypes = [C.c_void_p] + _lib.svt_hip_boolcode_host.argtypes[1:]
        _lib.svt_hip_frame_header_host.argtypes = [C.c_void_p, C.c_void_p, _u32, C.POINTER(_u32), C.POINTER(_u32)]
        _lib.svt_hip_frame_show_existing_host.argtypes = [C.c_int32, C.c_void_p]
        _lib.svt_hip_frame_batch_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, _u32, C.c_void_p]
        _lib.svt_hip_frame_assemble_host.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, _u32, C.c_void_p]
        _lib.svt_hip_frame_geometry.restype = None
        # (params, out, capacity, bytes, size_bit)
        _lib.svt_hip_frame_header_uncompressed_host.argtypes = [C.c_void_p, C.c_void_p, _u32, C.POINTER(_u32), C.POINTER(_u32)]
        _lib.svt_hip_frame_parts_batch_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, _u32, C.c_void_p]
        _lib.svt_hip_frame_assemble_parts_host.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, _u32, C.c_void_p]
        _lib.svt_hip_encdec_work_destroy.restype = None
        _lib.svt_hip_host_free.restype = None
        _lib.svt_hip_encdec_work_set_stage_hook.restype = None
        _lib.svt_hip_lf_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        _lib.svt_hip_tile_read_kf_host.argtypes = [C.c_void_p, _u32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
        _lib.svt_hip_tile_read_host.argtypes = [C.c_void_p, _u32] + [C.c_void_p] * 10
        _lib.svt_hip_frame_read_host.argtypes = [C.c_void_p, _u32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 11
        _lib.svt_hip_frame_read_header_host.argtypes = [C.c_void_p, _u32, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.svt_hip_frame_read_coef_host.argtypes = _lib.svt_hip_frame_read_host.argtypes + [C.c_void_p]      # (... , tables_out)
        # (ctx, d_pred, d_recon, d_blocks, size_count[4], d_qtabs, d_qcoeff, d_eob, d_overflow)
        _lib.svt_hip_recon_batch_device.argtypes = [C.c_void_p] * 9
        # (ctx, work, n_pics, pics, width, height, mi_stride, q_index, thr, pad_x, pad_y, d_status)
        _lib.svt_hip_decode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        _lib.svt_hip_decode_mixed_batch_device.argtypes = _lib.svt_hip_decode_batch_device.argtypes
        # (ctx, work, pic, width, height, mi_stride, q_index, thr, pad_x, pad_y, d_status)
        _lib.svt_hip_decode_intra_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        # (ctx, n_pics, pics, width, height, lambda, intra_penalty, filter_level, mi_stride, d_intra_units)
        _lib.svt_hip_md_mixed_batch_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, _u32, _u32, C.c_int32, C.c_int32, C.c_void_p]
        # (results, ois, width, height, lambda, intra_penalty, filter_level, mc_mi, lf_mi, mi_stride, intra_units)
        _lib.svt_hip_md_mixed_picture.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _u32, _u32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        # (ctx, n_pics, srcs, width, height, with_4x4, d_out)
        _lib.svt_hip_intra_search_batch_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        # entropy pass
        _lib.svt_hip_entropy_limits_worst.restype = None
        _lib.svt_hip_entropy_limits_worst.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        _lib.svt_hip_entropy_work_bytes.restype = C.c_uint64
        _lib.svt_hip_entropy_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        _lib.svt_hip_entropy_work_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        _lib.svt_hip_entropy_work_destroy.restype = None
        _lib.svt_hip_entropy_work_destroy.argtypes = [C.c_void_p, C.c_void_p]
        # (ctx, work, n_pics, pics, d_arena, arena_capacity, d_table, d_results)
        _lib.svt_hip_entropy_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, _u32, C.c_void_p, C.c_void_p]
        _lib.svt_hip_entropy_work_set_stage_hook.restype = None
        _lib.svt_hip_entropy_work_set_stage_hook.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.svt_hip_entropy_work_buffers.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        # the coefficient-update mode: (ctx, work, on); (limits); (work, pic, out); svt_hip_entropy_picture's arguments + (probs, update)
        _lib.svt_hip_entropy_work_set_coef_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        _lib.svt_hip_entropy_coef_update_bytes.restype = C.c_uint64
        _lib.svt_hip_entropy_coef_update_bytes.argtypes = [C.c_void_p]
        _lib.svt_hip_entropy_work_coef_buffers.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        _lib.svt_hip_entropy_picture_coef.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p, _u32, C.POINTER(_u32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # (bool tables, modes tables, inter tables, pic, mi_stride, limits, packet, packet_capacity, packet_size, result, detail)
        _lib.svt_hip_entropy_picture.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p, _u32, C.POINTER(_u32), C.c_void_p, C.c_void_p]
        # (tok_total, max_tokens, n_bools, bools_capacity, status, size, max_tile_bytes, verdict_a, result)
        _lib.svt_hip_entropy_gate_host.restype = _u32
        _lib.svt_hip_entropy_gate_host.argtypes = [_u32, _u32, _u32, _u32, C.c_void_p, _u32, _u32, C.POINTER(_u32), C.c_void_p]
        _lib.svt_hip_entropy_deliverable.restype = _u32
        _lib.svt_hip_entropy_deliverable.argtypes = [C.c_void_p]
        _lib.svt_hip_compound_refs_from_sign_bias.restype = None
        _lib.svt_hip_compound_refs_from_sign_bias.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(f"svt_hip call failed rc={rc}: {load().svt_hip_last_error().decode()}")


class MePictureConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pic_width", "pic_height", "enc_mode", "tune", "frame_rate", "num_ref_lists",
                                         "temporal_layer_index", "hierarchical_levels", "is_used_as_reference", "same_ref_poc",
                                         "rate_control_mode")]


class PaNoiseParams(C.Structure):
    _fields_ = [("method", C.c_int32), ("noise_detection_th", C.c_int32), ("luma_height", C.c_int32)]


PA_NOISE_FULL, PA_NOISE_HALF, PA_NOISE_QUARTER = 0, 1, 2
# svt_pa_noise_result
PA_NOISE_RESULT_DTYPE = np.dtype([("pic_noise_class", np.uint32), ("sb_count", np.uint32), ("pic_noise_variance_sum", np.uint64)])


def pa_noise_params_derive(tune, enc_mode, width, height):
    p = PaNoiseParams()
    check(load().svt_hip_pa_noise_params_derive(C.byref(p), tune, enc_mode, width, height))
    return p


def me_params_derive(**kw):
    p, c = MeParams(), MePictureConfig(**kw)
    check(load().svt_hip_me_params_derive(C.byref(p), C.byref(c)))
    return p


def me_params_preset(width, height, enc_mode, tune, num_ref_lists, temporal_layer, hierarchical_levels):
    p = MeParams()
    check(load().svt_hip_me_params_preset(C.byref(p), width, height, enc_mode, tune, num_ref_lists,
                                          temporal_layer, hierarchical_levels))
    return p


def plane_desc(arr, origin_x, origin_y, ptr=None):
    """svt_plane for a padded 2-D uint8 array (numpy, or a device pointer given via ptr)."""
    h, w = arr.shape
    p = Plane()
    p.buf = ptr if ptr is not None else arr.ctypes.data
    p.stride = arr.strides[0] if hasattr(arr, "strides") and ptr is None else w
    p.origin_x, p.origin_y = origin_x, origin_y
    p.width, p.height = w - 2 * origin_x, h - 2 * origin_y
    return p


# entropy pass (svt_entropy_limits / svt_entropy_picture / svt_entropy_result / svt_entropy_buffers / svt_entropy_host_detail of include/svtvp9_hip.h)
class EntropyLimits(C.Structure):
    _fields_ = [("max_pics", C.c_uint32), ("max_tokens", C.c_uint32), ("max_bools", C.c_uint32), ("max_tile_bytes", C.c_uint32)]


class EntropyPicture(C.Structure):
    _fields_ = [("d_lf_mi", C.c_void_p), ("d_mc_mi", C.c_void_p), ("d_qcoeff", C.c_void_p), ("d_eob_map", C.c_void_p), ("d_counts", C.c_void_p),
                ("frame", FrameParams), ("list_ref_frame", C.c_uint8 * 2), ("restrict_ref_mvs", C.c_uint8), ("trailer_len", C.c_uint8), ("trailer", C.c_uint8 * 4)]


class EntropyBuffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("d_tok_off", "d_sb_off", "d_tokens", "d_ext", "d_status", "d_bools", "d_segments", "d_n_bools", "d_tile", "d_tile_size",
                                          "d_verdict")] + [("n_segments", C.c_uint32), ("n_sb", C.c_uint32)]


class EntropyHostDetail(C.Structure):
    _fields_ = [("stream_bools", C.c_uint32), ("header_bytes", C.c_uint32), ("coded_size", C.c_uint32), ("pad_", C.c_uint32)]


ENTROPY_RESULT_DTYPE = np.dtype([(n, "<u4") for n in ("flags", "tokens", "mode_bools", "tile_bytes", "inter_leaves", "newmv_leaves", "unfaithful_leaves", "pad")])
assert C.sizeof(EntropyPicture) == 112 and ENTROPY_RESULT_DTYPE.itemsize == 32 and C.sizeof(EntropyLimits) == 16
ENT_BAD_GRID, ENT_TOKENS_OVER, ENT_MODE_BOOLS_OVER, ENT_UNFAITHFUL_MV, ENT_STREAM_OVER, ENT_TILE_OVER = 1, 2, 4, 8, 16, 32
ENT_NEEDS_BACKWARD_ADAPTATION, ENT_LOSSLESS, ENT_COMP_FLAG_MISMATCH, ENT_REFERENCE_MODE_UNREAD = 1, 2, 4, 8
ENT_STAGES = ("headers", "tokens", "labels", "modes", "gate", "boolcode", "result", "frame", "end")
ENT_STAGE_COEF_UPDATE = 9  # reported between "modes" and "gate", in the coefficient-update mode only
ENT_STAGES_COEF = ENT_STAGES + ("coef_update",)


class EntropyCoefBuffers(C.Structure):  # svt_entropy_coef_buffers: a picture's part of the coefficient-update mode's slab
    _fields_ = [(n, C.c_void_p) for n in ("d_counts", "d_eob_branch", "d_probs", "d_hdr_bools", "d_hdr_bytes", "d_result", "d_n_hdr_bools", "d_segment", "d_hdr_size")] + \
               [("hdr_bools_capacity", C.c_uint32), ("hdr_capacity", C.c_uint32)]
ENTROPY_STAGE_HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int32)

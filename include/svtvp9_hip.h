/*
 * svtvp9_hip.h -- C-ABI of the MI355X (gfx950) implementation of SVT-VP9's block-level DSP hot path.
 *
 * Plain C, plain pointers and sizes; no C++/torch types.  This is the boundary a maintainer of the
 * reference binds: three *batched* entry points that replace the places where the
 * reference calls its per-block x86 kernels, plus context management.
 *
 *   svt_hip_me_picture   replaces the SB loop of eb_vp9_motion_estimation_kernel
 *                        (Source/Lib/Codec/EbMotionEstimationProcess.c:964-1044 -> motion_estimate_sb,
 *                         Source/Lib/Codec/EbMotionEstimation.c:4524-5305)
 *   svt_hip_tq_batch     replaces perform_coding_loop's residual -> fwd txfm -> quant -> (inv txfm + recon)
 *                        (Source/Lib/Codec/EbEncDecProcess.c:365-587; kernels VPX/fwd_txfm.c, vp9_dct.c,
 *                         quantize.c, inv_txfm.c, vp9_idct.c)
 *   svt_hip_lf_frame     replaces eb_vp9_loop_filter_frame (Source/Lib/VPX/vp9_loopfilter.c:1521,
 *                        called at Source/Lib/Codec/EbEncDecProcess.c:5678)
 *
 * All functions return 0 on success or a negative svt_hip_status.  Host buffers are caller-owned;
 * device buffers are owned by the context.  A context is bound to one HIP device and one stream;
 * calls on different contexts are independent (the reference runs up to 20 ME threads).
 *
 * Every pointer parameter named d_* is a DEVICE pointer (HBM resident); the *_host convenience
 * wrappers take host pointers and stage through the context's own device buffers.
 */
#ifndef SVTVP9_HIP_H
#define SVTVP9_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------ */
/* status codes (negative = error; values mirror the sign convention of EbErrorType,                 */
/* Source/API/EbSvtVp9Enc.h:100-120, without reusing its 0x8000xxxx numbering)                        */
/* ------------------------------------------------------------------------------------------------ */
typedef enum svt_hip_status {
    SVT_HIP_OK                 = 0,
    SVT_HIP_ERR_BAD_PARAMETER  = -1, /* EB_ErrorBadParameter */
    SVT_HIP_ERR_NO_RESOURCES   = -2, /* EB_ErrorInsufficientResources */
    SVT_HIP_ERR_DEVICE         = -3, /* HIP runtime failure (message via svt_hip_last_error) */
    SVT_HIP_ERR_UNSUPPORTED    = -4
} svt_hip_status;

typedef struct svt_hip_ctx svt_hip_ctx; /* opaque */

/* ------------------------------------------------------------------------------------------------ */
/* Motion estimation                                                                                  */
/* ------------------------------------------------------------------------------------------------ */

#define SVT_ME_PU_COUNT 85 /* MAX_ME_PU_COUNT, Codec/EbMotionEstimationLcuResults.h:14 */
#define SVT_SB_SIZE 64     /* MAX_SB_SIZE */

/* One padded 8-bit luma plane.  Mirrors the fields of EbPictureBufferDesc that ME reads
 * (Codec/EbPictureBufferDesc.h:27-59): buffer_y, stride_y, origin_x/y (= padding), width, height. */
typedef struct svt_plane {
    const uint8_t *buf;      /* first byte of the padded buffer (top-left of the padding) */
    int32_t        stride;   /* bytes per row */
    int32_t        origin_x; /* left padding  (picture column 0 is at buf[origin_y*stride+origin_x]) */
    int32_t        origin_y; /* top padding */
    int32_t        width;    /* unpadded width  */
    int32_t        height;   /* unpadded height */
} svt_plane;

/* The three planes of an EbPaReferenceObject (Codec/EbReferenceObject.h:39-49):
 * padded input, 1/4 (2x2 point-decimated) and 1/16 (4x4 point-decimated) luma. */
typedef struct svt_pa_picture {
    svt_plane full;
    svt_plane quarter;
    svt_plane sixteenth;
} svt_pa_picture;

/* Fractional search method, Codec/EbDefinitions.h:664-666 */
#define SVT_SUB_SAD_SEARCH 0
#define SVT_FULL_SAD_SEARCH 1
#define SVT_SSD_SEARCH 2

/* Everything motion_estimate_sb reads from PictureParentControlSet / SequenceControlSet / MeContext.
 * Field names follow the reference (Codec/EbMotionEstimationContext.h:372-398,
 * Codec/EbMotionEstimation.c:4584-4631). */
typedef struct svt_me_params {
    /* picture level */
    uint8_t  num_ref_lists;        /* 1 = P_SLICE (list 0 only), 2 = B_SLICE */
    uint8_t  temporal_layer_index;
    uint8_t  hierarchical_levels;  /* selects the HME-L0 multiplier row, Codec/EbDefinitions.h:989-1005 */
    uint8_t  enable_hme_flag;
    uint8_t  enable_hme_level_0_flag;
    uint8_t  enable_hme_level_1_flag;
    uint8_t  enable_hme_level_2_flag;
    uint8_t  cu8x8_mode;           /* 0: refine + bipred 8x8 PUs, 1: full-pel only (Codec/EbDefinitions.h:943) */
    uint8_t  cu16x16_mode;         /* 0: refine + bipred 16x16 PUs */
    uint8_t  same_ref_poc;         /* ref_pic_poc_array[0] == ref_pic_poc_array[1] (EbMotionEstimation.c:4952) */
    uint8_t  rate_control_mode;    /* != 0 -> rcme_distortion is produced */
    /* MeContext multi-mode signals */
    uint8_t  fractional_search_method; /* SVT_SUB_SAD_SEARCH / SVT_FULL_SAD_SEARCH / SVT_SSD_SEARCH */
    uint8_t  fractional_search_model;  /* 0 all, 1 selective (su_pel_enable), 2 off */
    uint8_t  fractional_search64x64;
    uint8_t  single_hme_quadrant;
    /* full-pel search area */
    uint8_t  search_area_width;
    uint8_t  search_area_height;
    /* HME */
    uint16_t number_hme_search_region_in_width;  /* 1 or 2 */
    uint16_t number_hme_search_region_in_height; /* 1 or 2 */
    uint16_t hme_level0_total_search_area_width;
    uint16_t hme_level0_total_search_area_height;
    uint16_t hme_level0_search_area_in_width_array[2];
    uint16_t hme_level0_search_area_in_height_array[2];
    uint16_t hme_level1_search_area_in_width_array[2];
    uint16_t hme_level1_search_area_in_height_array[2];
    uint16_t hme_level2_search_area_in_width_array[2];
    uint16_t hme_level2_search_area_in_height_array[2];
} svt_me_params;

/* Result record per (SB, PU); same field order and size (40 bytes) as MeCuResults
 * (Codec/EbMotionEstimationLcuResults.h:39-56).  The reference's 2-bit `direction` bit-field is
 * widened to a full uint32 here (value 0 = UNI_PRED_LIST_0, 1 = UNI_PRED_LIST_1, 2 = BI_PRED);
 * INTEGRATION.md shows the field-wise copy into MeCuResults. */
typedef struct svt_me_dist_dir {
    uint32_t distortion;
    uint32_t direction;
} svt_me_dist_dir;

typedef struct svt_me_pu_result {
    int16_t         x_mv_l0, y_mv_l0, x_mv_l1, y_mv_l1; /* quarter-pel units */
    svt_me_dist_dir distortion_direction[3];
    uint8_t         total_me_candidate_index;
    uint8_t         pad_[7];
} svt_me_pu_result;

/* Geometry helper: number of SBs of a picture (ceil(w/64)*ceil(h/64)). */
int32_t svt_hip_sb_count(int32_t pic_width, int32_t pic_height);

/* INPUT_SIZE_576p_RANGE_OR_LOWER / 1080i / 1080p / 4K_RANGE = 0..3 of a picture size, by luma sample count
 * (eb_vp9_derive_input_resolution, Codec/EbSequenceControlSet.c:489-499).  It is also the index of the non-moving
 * threshold shift that svt_hip_me_zz_sad_device takes. */
int32_t svt_hip_input_resolution(int32_t pic_width, int32_t pic_height);

/* What the reference's parameter derivation reads from the sequence / picture control sets. */
typedef struct svt_me_picture_config {
    int32_t pic_width, pic_height;   /* luma_width / luma_height */
    int32_t enc_mode;                /* 0..12 */
    int32_t tune;                    /* 0 SQ, 1 OQ, 2 VMAF (Codec/EbDefinitions.h:658-660) */
    int32_t frame_rate;              /* static_config.frame_rate >> 16 (frames per second) */
    int32_t num_ref_lists;           /* 1 = P picture, 2 = B picture */
    int32_t temporal_layer_index;
    int32_t hierarchical_levels;
    int32_t is_used_as_reference;    /* is_used_as_reference_flag */
    int32_t same_ref_poc;            /* both lists hold the same picture */
    int32_t rate_control_mode;
} svt_me_picture_config;

/* Fill `p` exactly as the reference derives the ME signals of a picture with use_default_me_hme = 1, for every tune,
 * enc_mode and picture size it accepts: eb_vp9_signal_derivation_pre_analysis_* (HME enables,
 * Codec/EbResourceCoordinationProcess.c:291-460), eb_vp9_signal_derivation_multi_processes_* (use_subpel_flag, cu8x8_mode,
 * Codec/EbPictureDecisionProcess.c:682-925), eb_vp9_set_me_hme_params_* + eb_vp9_signal_derivation_me_kernel_*
 * (Codec/EbMotionEstimationProcess.c:55-324, 541-720). */
int32_t svt_hip_me_params_derive(svt_me_params *p, const svt_me_picture_config *cfg);

/* Shorthand for the reference's default random-access structure at 60 frames/s: every temporal layer but the deepest is
 * used as reference (is_used_as_reference = temporal_layer_index < hierarchical_levels). */
int32_t svt_hip_me_params_preset(svt_me_params *p, int32_t pic_width, int32_t pic_height, int32_t enc_mode,
                                 int32_t tune, int32_t num_ref_lists, int32_t temporal_layer_index,
                                 int32_t hierarchical_levels);

/* diagnostic: which compiled instance of the ME kernel serves a parameter set -- 0 the generic one, > 0 an instance whose search
 * parameters are compile-time constants (one per BASELINE configuration; identical results by construction) */
int32_t svt_hip_me_kernel_instance(const svt_me_params *p);
/* diagnostic: the instance the last ME launch on ctx actually ran -- the index above, + 100 when the launch was served by the
 * driver for single-region level-0 HME presets (csrc/me_fast.h: whole SB columns, level-0 areas up to 256 x 256), + 200 when it was the pair of
 * launches of the compact LDS layout (csrc/me_layout.h: the 64 x 64-area presets at two workgroups per CU) */
int32_t svt_hip_me_last_instance(const svt_hip_ctx *ctx);
/* diagnostic (host only): LDS bytes of a workgroup of the ME kernel for a parameter set -- compact = 0: the plain layout; 1: the compact one (search-area
 * widths that are multiples of 8; the launcher takes it where it buys a workgroup per CU: 160 KB per CU in granules of 1 280 bytes).  Negative: no such layout. */
int32_t svt_hip_me_lds_bytes(const svt_me_params *p, int32_t compact);
/* Deployment knob of the intra encode pass (svt_hip_encdec_intra_device, and the intra blocks of inter pictures) launched on ctx: at most n
 * 64-lane WORKERS (0 = the default: two per compute unit, the lowest latency for a key frame alone).  A worker is one wave; the launch packs four
 * of them into each 256-thread workgroup (n = 128: 32 workgroups), so the name of the call is historical -- until the packing a worker was a
 * workgroup.  A pass that runs BESIDE other work of the device (a key frame of the next GOP beside the current one) leaves more of it to that work
 * with fewer: every CU that hosts one of its WORKGROUPS -- up to four workers, one per SIMD -- has registers and LDS for one motion-estimation
 * workgroup less (128: 7.9 ms alone).  The environment's SVT_HIP_INTRA_WGS sets the process-wide default, in workers as well. */
int32_t svt_hip_ctx_set_intra_workgroups(svt_hip_ctx *ctx, int32_t n);
/* submits an empty kernel to the context's stream and waits: the stream's hardware queue exists afterwards (the runtime creates it at the first
 * submission, 1-3 ms on the submitting thread).  For hosts that time a stream from its first picture (the encoder library's init does this). */
int32_t svt_hip_ctx_warm(svt_hip_ctx *ctx);
/* the same with a kernel that has a private segment of (at least) scratch_bytes per lane, up to 1024: the queue's scratch memory is sized too (the
 * intra pass's kernel needs 752 bytes per lane -- 4 ms on the thread that submits it first; the 32x32 transform 130) */
int32_t svt_hip_ctx_warm_scratch(svt_hip_ctx *ctx, int32_t scratch_bytes);
/* 1 when two parameter sets may share one launch of svt_hip_me_batch_layers_device: equal in every field but num_ref_lists,
 * temporal_layer_index, hierarchical_levels and same_ref_poc (compared field by field: the record has padding) */
int32_t svt_hip_me_params_same_launch(const svt_me_params *a, const svt_me_params *b);

/* ------------------------------------------------------------------------------------------------ */
/* context                                                                                            */
/* ------------------------------------------------------------------------------------------------ */
int32_t svt_hip_ctx_create(svt_hip_ctx **ctx, int32_t device_ordinal);
/* Same, but all work is enqueued on a caller-provided hipStream_t (passed as void*). */
int32_t svt_hip_ctx_create_on_stream(svt_hip_ctx **ctx, int32_t device_ordinal, void *hip_stream);
/* A context whose own stream is restricted to a set of compute units (hipExtStreamCreateWithCUMask; bit i of the mask
 * words = CU i in the driver's enumeration).  Stages of a pipeline that run concurrently can be given disjoint CU sets
 * so that each CU executes one kernel (its LDS, instruction cache and issue slots are not shared between stages). */
int32_t svt_hip_ctx_create_cu_mask(svt_hip_ctx **ctx, int32_t device, const uint32_t *cu_mask, int32_t mask_words);
/* the context's HIP stream (hipStream_t), e.g. to record events on it or to make other streams wait for it */
void *svt_hip_ctx_stream(svt_hip_ctx *ctx);
void    svt_hip_ctx_destroy(svt_hip_ctx *ctx);
int32_t svt_hip_ctx_synchronize(svt_hip_ctx *ctx);
const char *svt_hip_last_error(void);
/* Timing of the kernels launched by the most recent *_device call on this context, measured with
 * hipEvents recorded on the context's stream (ms).  Valid after svt_hip_ctx_synchronize(). */
float   svt_hip_last_kernel_ms(svt_hip_ctx *ctx);

/* Device memory for C hosts (the *_device entry points take HBM pointers): plain allocations on the context's device, and
 * copies ordered on the context's stream.  svt_hip_mem_upload_2d returns after the host rows have been consumed (the caller
 * may reuse them), svt_hip_mem_download after the data has arrived. */
int32_t svt_hip_mem_alloc(svt_hip_ctx *ctx, size_t bytes, void **d_ptr);
void    svt_hip_mem_free(svt_hip_ctx *ctx, void *d_ptr);
int32_t svt_hip_mem_upload_2d(svt_hip_ctx *ctx, void *d_dst, size_t dst_stride, const void *src, size_t src_stride, size_t width_bytes,
                              size_t rows);
int32_t svt_hip_mem_download(svt_hip_ctx *ctx, void *dst, const void *d_src, size_t bytes);
/* Asynchronous form of svt_hip_mem_upload_2d for a host that must not wait for the device: the rows are copied into a pinned
 * staging buffer owned by the context before the call returns (= the copy eb_vp9_svt_enc_send_picture makes of the caller's
 * picture, Codec/EbEncHandle.c:2743-2796: the caller may reuse its buffer at once), the host-to-device copy is enqueued on the
 * context's stream.  The call blocks only when all staging buffers (4) still hold copies the device has not consumed. */
int32_t svt_hip_mem_upload_2d_async(svt_hip_ctx *ctx, void *d_dst, size_t dst_stride, const void *src, size_t src_stride, size_t width_bytes,
                                    size_t rows);
/* Up to 4 planes of one picture through ONE staging slot (same contract as svt_hip_mem_upload_2d_async for each plane): destinations
 * that lie back to back on the device, tight (dst_stride == width_bytes, d_dst[i + 1] == the end of plane i: Y | Cb | Cr in one buffer),
 * travel as one host-to-device copy -- a third of the stream operations of three separate uploads (copy_frame_buffer copies the three
 * planes of a picture in one call too, Codec/EbEncHandle.c:2743-2796). */
int32_t svt_hip_mem_upload_planes_async(svt_hip_ctx *ctx, int32_t n_planes, void *const *d_dst, const size_t *dst_stride, const void *const *src,
                                        const size_t *src_stride, const size_t *width_bytes, const size_t *rows);
/* The same upload WITHOUT the staging copy, for a host whose rows lie in memory that stays allocated while the library is in use: a
 * range of host memory is page-locked (hipHostRegister) the first time it is seen, so a host that sends from a fixed pool of buffers
 * pays for that once and is read by the DMA engines directly from then on (57 GB/s on the MI355X box against ~27 GB/s through the
 * staging copy); ranges that cannot be registered, and more than 1024 distinct ranges, go through the staging path.  The copy is
 * asynchronous: the rows must stay valid until svt_hip_mem_upload_wait(ctx) has returned (it waits for every direct upload enqueued
 * on ctx -- not for the rest of the stream).  svt_hip_host_unregister_all unlocks everything (no upload may be in flight).  Locked
 * ranges must not be freed, nor passed in part to other host <-> device copies of the process, before they are unlocked. */
int32_t svt_hip_mem_upload_2d_direct(svt_hip_ctx *ctx, void *d_dst, size_t dst_stride, const void *src, size_t src_stride, size_t width_bytes,
                                     size_t rows);
int32_t svt_hip_mem_upload_wait(svt_hip_ctx *ctx);
void    svt_hip_host_unregister_all(void);
/* The registry's life follows its users: a host retains it while it uploads directly and releases it when all its uploads have completed;
 * the LAST release unlocks every range (memory freed afterwards, or re-allocated at the same address, is never read through a stale
 * registration).  A range whose registration failed is not remembered: the next upload from it tries again.  The encoder library
 * (libSvtVp9Enc.so, SVT_HIP_REGISTER_INPUT=1) retains in eb_vp9_init_encoder and releases in eb_vp9_deinit_encoder. */
void    svt_hip_host_registry_retain(void);
void    svt_hip_host_registry_release(void);
/* Completion markers: svt_hip_ctx_marker_record notes "everything enqueued on the context's stream so far" and returns a marker;
 * svt_hip_ctx_marker_query returns 1 when that work has completed, 0 while it is pending (never blocks), negative on error;
 * svt_hip_ctx_marker_wait blocks until it has.  This is what lets eb_vp9_svt_get_packet poll without blocking and block only when
 * the application says it has sent its last picture (Codec/EbEncHandle.c:2880-2915). */
int32_t svt_hip_ctx_marker_record(svt_hip_ctx *ctx, uint64_t *marker);
int32_t svt_hip_ctx_marker_query(svt_hip_ctx *ctx, uint64_t marker);
int32_t svt_hip_ctx_marker_wait(svt_hip_ctx *ctx, uint64_t marker);
int32_t svt_hip_mem_set(svt_hip_ctx *ctx, void *d_dst, int32_t value, size_t bytes);

/* ------------------------------------------------------------------------------------------------ */
/* ME entry points                                                                                    */
/* ------------------------------------------------------------------------------------------------ */

/* Device-resident form (the one that is benchmarked): every svt_plane.buf in cur/ref0/ref1 is a
 * device pointer, d_results is a device array [n_sb][85].  ref1 may be NULL when num_ref_lists==1.
 * d_rcme_distortion (uint32 per SB) may be NULL.  Asynchronous on the context's stream. */
int32_t svt_hip_me_picture_device(svt_hip_ctx *ctx, const svt_pa_picture *cur, const svt_pa_picture *ref0,
                                  const svt_pa_picture *ref1, const svt_me_params *params,
                                  svt_me_pu_result *d_results, uint32_t *d_rcme_distortion);

/* Batched device-resident form: ME of n_pics independent pictures in ONE launch (ME reads source
 * pictures only -- Codec/EbMotionEstimation.c:4638-4642 -- so all pictures of a mini-GOP are
 * independent).  Arrays of n_pics descriptors (host memory); d_results[i] / d_rcme[i] device arrays. */
int32_t svt_hip_me_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_pa_picture *cur,
                                const svt_pa_picture *ref0, const svt_pa_picture *ref1,
                                const svt_me_params *params, svt_me_pu_result *const *d_results,
                                uint32_t *const *d_rcme_distortion);
/* The same with one parameter set PER PICTURE (params[i] for picture i): the pictures of a mini-GOP differ in
 * num_ref_lists, temporal_layer_index, hierarchical_levels and same_ref_poc only (everything else follows from the
 * configuration: Codec/EbMotionEstimationProcess.c:541-720), so one launch serves all its temporal layers -- no launch
 * tails between the layers.  Returns SVT_HIP_ERR_BAD_PARAMETER when the sets differ in any other field. */
int32_t svt_hip_me_batch_layers_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_pa_picture *cur,
                                       const svt_pa_picture *ref0, const svt_pa_picture *ref1,
                                       const svt_me_params *params, svt_me_pu_result *const *d_results,
                                       uint32_t *const *d_rcme_distortion);

/* Host-pointer convenience form (what the reference's ME thread would call): uploads the planes,
 * runs svt_hip_me_picture_device, downloads results[n_sb][85], synchronous. */
int32_t svt_hip_me_picture(svt_hip_ctx *ctx, const svt_pa_picture *cur, const svt_pa_picture *ref0,
                           const svt_pa_picture *ref1, const svt_me_params *params, svt_me_pu_result *results,
                           uint32_t *rcme_distortion);

/* Stand-alone HME level-0 search = eb_vp9_sad_loop_kernel (C_DEFAULT/EbComputeSAD_C.c:132-169)
 * batched over n independent (block, window) problems; device pointers. Exposed for unit parity tests.
 * Each problem: block w x h (rows already at src_stride), window search_w x search_h; ref row step
 * for the block rows = ref_stride, for successive search rows = ref_stride_raw. */
typedef struct svt_sad_loop_job {
    uint64_t src_off;   /* byte offset into d_src */
    uint64_t ref_off;   /* byte offset into d_ref */
    int32_t  src_stride, ref_stride, ref_stride_raw;
    int32_t  width, height;       /* block */
    int32_t  search_w, search_h;  /* window */
} svt_sad_loop_job;
typedef struct svt_sad_loop_result {
    uint32_t best_sad;
    int16_t  x, y;
} svt_sad_loop_result;
int32_t svt_hip_sad_loop_batch_device(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_ref,
                                      const svt_sad_loop_job *d_jobs, int32_t n_jobs,
                                      svt_sad_loop_result *d_out);

/* Per-SB side outputs of the ME stage (row M12 of the scope table).
 *
 * svt_hip_me_zz_sad_device = compute_zz_sad (Codec/EbMotionEstimationProcess.c:431-534): for every complete SB the
 * 16x16 SAD between the current picture's 1/16 plane and the 4x4 point-decimated collocated SB of the PREVIOUS
 * picture's input (eb_vp9_decimation_2d, Codec/EbPictureAnalysisProcess.c:102-122); incomplete SBs get 0xffffffff.
 * d_non_moving_index[sb] = NON_MOVING_SCORE_{0,1,2,3} = 0/10/20/30 from the thresholds 2,4,8 x (16*16) >>
 * non_moving_th_shift[input_resolution] (:353; input_resolution 0..3 = <=576p, 720p, 1080p, 2160p) -- the value the
 * reference stores into the previous picture's non_moving_index_array.  Planes are device resident. */
int32_t svt_hip_me_zz_sad_device(svt_hip_ctx *ctx, const svt_plane *cur_sixteenth, const svt_plane *prev_input,
                                 int32_t input_resolution, uint32_t *d_zz_sad, uint8_t *d_non_moving_index);

/* Host-side: eb_vp9_derive_similar_collocated_flag (Codec/EbMotionEstimationProcess.c:747-783) for n SBs: compares the
 * 64x64 mean / variance of each SB (picture analysis outputs) with the list-0 reference's.  similar[sb] is only set
 * when the picture is used as a reference, similar_all_layers[sb] always. */
void svt_hip_me_similar_collocated(const uint8_t *cur_mean, const uint16_t *cur_var, const uint8_t *ref_mean,
                                   const uint16_t *ref_var, int32_t n_sb, int32_t is_i_slice,
                                   int32_t is_used_as_reference, uint8_t *similar, uint8_t *similar_all_layers);

/* The rest of the ME kernel process's per-SB bookkeeping (scope row M12), on the device so that neither the 6.9 MB result
 * array nor the picture-analysis statistics have to come back to the host for it:
 *   stationary_edge_over_update_over_time_sb_part1 / _part2 (Codec/EbMotionEstimationProcess.c:785-869): the logo /
 *       stationary-edge flags of every SB from the 64x64 list-0 MV and distortion of its best ME candidate (d_results[sb][0])
 *       and the variance of its four 32x32 blocks (d_var[sb * 85 + 1..4], svt_hip_pa_mean_variance_device's layout);
 *       which SBs can hold a logo is eb_vp9_sb_params_init's potential_logo_sb rule (Codec/EbSequenceControlSet.c:332-413);
 *   the rate-control SAD-interval indices and histograms (:1103-1237): inter index from rcme_distortion[sb] (the ME entry
 *       points' d_rcme_distortion), intra index from the 64x64 variance, one count per complete SB in each histogram.
 * part2 only runs when run_part2 != 0 (= !end_of_sequence_flag && look_ahead_distance != 0); without it check2 /
 * low_dist_logo are written as 0.  The histograms and the full-SB count are ADDED to (the reference zeroes them per picture). */
typedef struct svt_me_sb_stats_params {
    int32_t pic_width, pic_height;
    int32_t input_resolution;      /* svt_hip_input_resolution() */
    int32_t temporal_layer_index;
    int32_t slice_type;            /* 0 B_SLICE, 1 P_SLICE, 2 I_SLICE (Codec/EbDefinitions.h EB_SLICE) */
    int32_t run_part2;
    int32_t rate_control_mode;     /* 0: no indices / histograms (static_config.rate_control_mode) */
} svt_me_sb_stats_params;
typedef struct svt_me_sb_stats {
    uint8_t  check1_for_logo_stationary_edge_over_time_flag;
    uint8_t  pm_check1_for_logo_stationary_edge_over_time_flag;
    uint8_t  check2_for_logo_stationary_edge_over_time_flag;
    uint8_t  low_dist_logo;
    uint16_t inter_sad_interval_index;
    uint16_t intra_sad_interval_index;
} svt_me_sb_stats;                 /* 8 bytes */
#define SVT_SAD_INTERVALS 128      /* NUMBER_OF_SAD_INTERVALS, Codec/EbRateControlTables.h:19 */
/* d_results may be NULL for an I picture, d_rcme_distortion when rate_control_mode == 0 or for an I picture.
 * d_hist: [0..127] me_distortion_histogram, [128..255] ois_distortion_histogram; d_full_sb_count: one uint32. */
int32_t svt_hip_me_sb_stats_device(svt_hip_ctx *ctx, const svt_me_sb_stats_params *params, const svt_me_pu_result *d_results,
                                   const uint16_t *d_var, const uint32_t *d_rcme_distortion, svt_me_sb_stats *d_stats,
                                   uint32_t *d_hist, uint32_t *d_full_sb_count);

/* ------------------------------------------------------------------------------------------------ */
/* Picture-analysis pre-ME stage ("next" row f-1 of the scope table)                                  */
/* ------------------------------------------------------------------------------------------------ */

/* Builds the three planes of an EbPaReferenceObject from a picture's W x H luma, all on the device:
 *   full      = copy + edge replication by origin_x/origin_y samples (eb_vp9_generate_padding, Codec/EbMcp.c:17-58,
 *               called by pad_picture_to_multiple_of_sb_dimensions, Codec/EbPictureAnalysisProcess.c:5010-5020)
 *   quarter   = 2x2 point decimation (eb_vp9_decimation_2d, :102-122, step 2) + edge replication, only if make_quarter
 *   sixteenth = 4x4 point decimation (step 4) + edge replication       (decimate_input_picture, :5025-5088)
 * `out[i]` describes the destination planes of picture i (device buffers; buf, stride, origin, width, height as the
 * ME entry points expect them: quarter = W/2 x H/2, sixteenth = W/4 x H/4).  W and H must be multiples of 8. */
int32_t svt_hip_pa_prepare_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const uint8_t *const *d_luma,
                                        const int32_t *luma_stride, const svt_pa_picture *out, int32_t make_quarter);

/* 8x8 .. 64x64 block mean and variance of every SB of a padded luma plane = compute_block_mean_compute_variance
 * (Codec/EbPictureAnalysisProcess.c:2115-3356; 8x8 sums on rows 0,2,4,6 with the SSE2 kernels the reference calls at
 * `-asm 0`, ASM_SSE2/EbComputeMean_Intrinsic_SSE2.c:10-53; larger blocks are >>2 averages of their four children).
 * d_mean[sb*85 + pu] = (uint8_t)(mean >> 8), d_var[sb*85 + pu] = (uint16_t)((mean_of_squares - mean^2) >> 16), pu in
 * raster order per size: 0 = 64x64, 1-4 = 32x32, 5-20 = 16x16, 21-84 = 8x8 (ME_TIER_ZERO_PU_*,
 * Codec/EbMotionEstimationContext.h:45-131).  SBs at the right/bottom border read the replicated padding. */
int32_t svt_hip_pa_mean_variance_device(svt_hip_ctx *ctx, const svt_plane *full, uint8_t *d_mean, uint16_t *d_var);

/* Noise detection = picture_pre_processing_operations (Codec/EbPictureAnalysisProcess.c:4191-4232) without the denoiser, which the
 * reference never reaches (enable_denoise_src_flag is false for tune 1, 2 and compiled out for tune 0 by TURN_OFF_PRE_PROCESSING). */
#define SVT_PA_NOISE_FULL 0    /* detect_input_picture_noise (:3512-3619) on the full picture, 64x64 variance per complete SB */
#define SVT_PA_NOISE_HALF 1    /* sub_sample_detect_noise (:3930-4055) on the 1/16 picture, 16x16 variance per SB */
#define SVT_PA_NOISE_QUARTER 2 /* quarter_sample_detect_noise (:3809-3928) on the 1/4 picture, 32x32 variance per SB */

typedef struct svt_pa_noise_params {
    int32_t method;             /* SVT_PA_NOISE_* (not the reference's NOISE_DETECT_* numbering) */
    int32_t noise_detection_th; /* picture_control_set_ptr->noise_detection_th, 0 or 1 */
    int32_t luma_height;        /* sequence_control_set_ptr->luma_height: selects the class ladder's offset */
} svt_pa_noise_params;

typedef struct svt_pa_noise_result {
    uint32_t pic_noise_class;        /* PIC_NOISE_CLASS_1, 2, 3, 3_1 = 1, 2, 3, 4 (Codec/EbDefinitions.h:860-871) */
    uint32_t sb_count;               /* tot_sb_count: the SBs the loop visited */
    uint64_t pic_noise_variance_sum; /* sum of (noiseBlkVar >> 16); pic_noise_variance_float = sum / (double)sb_count */
} svt_pa_noise_result;

/* The noise fields of eb_vp9_signal_derivation_pre_analysis_sq / _oq / _vmaf (Codec/EbResourceCoordinationProcess.c:291-440) for
 * tune 0 / 1 / 2, enc_mode 0..12 and the picture size (through the input-resolution class of the helper above). */
int32_t svt_hip_pa_noise_params_derive(svt_pa_noise_params *p, int32_t tune, int32_t enc_mode, int32_t pic_width, int32_t pic_height);

/* For each picture of the batch: the weak luma filter (N + W + 4C + E + S) / 8 (get_filtered_types type 0, :1403-1412, as
 * eb_vp9_noise_extract_luma_weak applies it, :1653-1706: picture-border samples are copied and their noise is 0), the difference
 * clip(in - filtered), and the block variances of both, on pics[i].full / .sixteenth / .quarter by params->method.  Written:
 *   d_sb_flat_noise[i][sb] (ceil(W/64) * ceil(H/64) bytes of the full picture, every one of them: 0 for SBs the reference's loop
 *   does not visit) and d_result[i].  The decimated forms visit only the whole 64x64 blocks of the decimated picture and take the
 *   noise variance of all SB rows of such a block from its first SB row, as the reference does.
 * d_denoised / d_noise are both NULL, or both arrays of n_pics dense planes of the analysed picture (stride = its width): they
 * receive the filtered and the noise samples of the area the reference's loop filters (all of the picture for the full form, the
 * whole 64x64 blocks for the others) and exist so that a test can compare with the reference's own filter.  When they are NULL
 * those samples never leave the registers.  The pointer arrays are host memory, what they point to is device memory. */
int32_t svt_hip_pa_noise_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_pa_picture *pics, const svt_pa_noise_params *params,
                                      uint8_t *const *d_sb_flat_noise, svt_pa_noise_result *d_result, uint8_t *const *d_denoised,
                                      uint8_t *const *d_noise);

/* Intensity histograms and averages = sub_sample_luma_generate_pixel_intensity_histogram_bins (:4237-4312) on pics[i].sixteenth,
 * its chroma twin (:4314-4432) on cb[i] / cr[i] (the source chroma planes, (W/2) x (H/2) of pics[i].full's W x H, every 4th row
 * and column; their sample (0,0) is the one under luma (0,0)) and calculate_input_average_intensity (:4839-4886).
 *   d_hist[i]       uint32 [regions_w][regions_h][3][256]  (1 + count) << 4
 *   d_avg_region[i] uint8  [regions_w][regions_h][3]
 *   d_avg[i]        uint8  [3]; with scd_mode 0 only [0] is written, from the 8x8 sub-sampled means of the W x H bytes at
 *                   pics[i].full.buf (the reference indexes buffer_y without the origin there, :4857-4860)
 * The last region in each direction takes the remainder of the division. */
int32_t svt_hip_pa_histogram_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_pa_picture *pics, const svt_plane *cb,
                                          const svt_plane *cr, int32_t regions_w, int32_t regions_h, int32_t scd_mode,
                                          uint32_t *const *d_hist, uint8_t *const *d_avg_region, uint8_t *const *d_avg);

/* cb_mean / cr_mean [sb][21] = compute_chroma_block_mean (:1828-2109) for complete SBs of a width x height luma picture, zero for
 * the others (zero_out_chroma_block_mean): index 0 = 64x64, 1-4 = 32x32, 5-20 = 16x16 luma blocks in raster order, from
 * eb_vp9_compute_sub_mean8x8_sse2_intrin sums of the 8x8 chroma blocks.  The 64x64 entry is (m32[0] + m32[1] + 2 * m32[3]) >> 2,
 * as the reference writes it (:2010-2015). */
int32_t svt_hip_pa_chroma_mean_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_plane *cb, const svt_plane *cr, int32_t width,
                                            int32_t height, uint8_t *const *d_cb_mean, uint8_t *const *d_cr_mean);

/* ------------------------------------------------------------------------------------------------ */
/* Transform / quantisation                                                                           */
/* ------------------------------------------------------------------------------------------------ */

/* TX sizes / types follow VPX/vp9_enums.h (TX_4X4..TX_32X32; DCT_DCT, ADST_DCT, DCT_ADST, ADST_ADST). */
#define SVT_TX_4X4 0
#define SVT_TX_8X8 1
#define SVT_TX_16X16 2
#define SVT_TX_32X32 3
#define SVT_DCT_DCT 0
#define SVT_ADST_DCT 1
#define SVT_DCT_ADST 2
#define SVT_ADST_ADST 3

/* Quantiser tables of one (qindex, plane): the [0]=DC,[1]=AC pairs eb_vp9_init_quantizer produces
 * (VPX/vp9_quantize.c:206-265); passed to eb_vp9_quantize_b[_32x32] (VPX/quantize.c:112-254). */
typedef struct svt_quant_tables {
    int16_t zbin[2], round[2], quant[2], quant_shift[2], dequant[2];
} svt_quant_tables;

/* Host-side: the tables of one (q index, plane) as eb_vp9_init_quantizer derives them (sharpness 0): q_index 0..255;
 * y_dc_step = eb_vp9_dc_quant(q_index, 0) (it selects the zero-bin factor, get_qzbin_factor :192-204); dc_step / ac_step =
 * eb_vp9_dc_quant / eb_vp9_ac_quant with the plane's deltas (VPX/vp9_quant_common.c). */
int32_t svt_hip_quant_tables_init(int32_t q_index, int32_t y_dc_step, int32_t dc_step, int32_t ac_step, svt_quant_tables *out);

/* One transform block of perform_coding_loop (Codec/EbEncDecProcess.c:365-587). */
typedef struct svt_tq_block {
    uint32_t src_off;    /* byte offset of the block's top-left in the source plane  */
    uint32_t pred_off;   /* byte offset in the prediction plane                       */
    uint32_t recon_off;  /* byte offset in the recon plane (written when do_recon)    */
    uint32_t coeff_off;  /* element offset into qcoeff / dqcoeff (n*n contiguous); multiple of 8 */
    uint32_t iscan_off;  /* element offset of this block's iscan table inside the iscan array */
    uint16_t src_stride, pred_stride, recon_stride;
    uint8_t  tx_size;    /* SVT_TX_* */
    uint8_t  tx_type;    /* SVT_DCT_DCT.. (ADST only for <=16x16) */
    uint8_t  qtab;       /* index into the quant-table array */
    uint8_t  do_recon;   /* run inverse transform + add into recon */
    uint8_t  partial32;  /* 32x32 only: use eb_vpx_partial_fdct32x32 (low 16x16 kept, rest zero) */
    uint8_t  pad_[1];    /* svt_hip_tq_rd_batch_device only: SVT_TQ_RATE_INFO(ctx, plane_type, is_inter), the block's rate inputs */
} svt_tq_block;          /* 32 bytes */
/* rate inputs of a block for the fused distortion + rate entry: ctx = combine_entropy_contexts(left, above) 0..2
 * (Codec/EbEncDecProcess.c:734), plane_type = get_plane_type (0 luma, 1 chroma), is_inter = is_inter_block(mi) */
#define SVT_TQ_RATE_INFO(ctx, plane_type, is_inter) ((uint8_t)(((ctx) & 3) | (((plane_type) & 1) << 2) | (((is_inter) & 1) << 3)))

/* Scan tables: the caller passes the reference's own iscan tables (scan_order->iscan of
 * eb_vp9_scan_orders[tx_size][tx_type] / eb_vp9_default_scan_orders[TX_32X32], VPX/vp9_scan.c) concatenated
 * in one int16 array; every block names its table by element offset (iscan_off).  iscan[rc] = position of
 * raster coefficient rc in scan order, which is all the quantiser needs to produce eob.
 *
 * residual = src - pred (eb_vp9_residual_kernel, C_DEFAULT/EbPictureOperators_C.c:204-223)
 * -> forward DCT/ADST (VPX/fwd_txfm.c, VPX/vp9_dct.c) -> eb_vp9_quantize_b[_32x32]
 * -> if do_recon: recon = pred; inverse transform of dqcoeff added into recon
 *    (eb_vp9_idct*_add / eb_vp9_iht*_add, VPX/vp9_idct.c:111-189).
 * Outputs: qcoeff, dqcoeff (int16, raster within block), eob per block.  Device pointers.
 * d_blocks must be GROUPED by transform size in the order 4x4, 8x8, 16x16, 32x32 with size_count[s] blocks of
 * size s (size_count is a host array), and do_recon must be uniform within a size group (the encode pass
 * reconstructs every block, mode decision none).  d_qcoeff / d_dqcoeff are 16-byte aligned and every coeff_off is a
 * multiple of 8 (rows are stored as 16-byte vectors; the reference's per-SB coefficient buffers advance by whole
 * blocks of >= 16 coefficients, so its offsets always are). */
int32_t svt_hip_tq_batch_device(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *d_recon,
                                const svt_tq_block *d_blocks, const int32_t size_count[4],
                                const svt_quant_tables *d_qtabs, const int16_t *d_iscan, int16_t *d_qcoeff,
                                int16_t *d_dqcoeff, uint16_t *d_eob);

/* Host-pointer convenience form. plane_bytes = size of each of src/pred/recon; coeff_count = total coeffs. */
/* Same, additionally producing the coefficient-domain distortion pair of every block as the reference's
 * full_distortion_kernel32bit does right after the transform/quantisation in mode decision
 * (C_DEFAULT/EbPictureOperators_C.c:288-311; function table Codec/EbPictureOperators.h:240):
 * d_dist[2*b] = sum (coeff - dqcoeff)^2, d_dist[2*b+1] = sum coeff^2 over the NxN block, with the reference's
 * int16/uint32 wrap-around.  (The _intra and _eob_zero variants of the reference return one of the two values twice.) */
int32_t svt_hip_tq_batch_dist_device(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *d_recon,
                                     const svt_tq_block *d_blocks, const int32_t size_count[4],
                                     const svt_quant_tables *d_qtabs, const int16_t *d_iscan, int16_t *d_qcoeff,
                                     int16_t *d_dqcoeff, uint16_t *d_eob, uint64_t *d_dist);

/* Forward declaration (defined with the coefficient rate section below). */
struct svt_rate_tables;

/* perform_dist_rate_calc in one pass (Codec/EbEncDecProcess.c:700-745): svt_hip_tq_batch_dist_device plus, per block,
 * d_bits[b] = coeff_rate_estimate(...) (Codec/EbRateDistortionCost.c:55-172, use_fast_coef_costing = 0) of the coefficients the
 * quantiser has just produced -- computed from registers / LDS behind the quantiser, no second pass over d_qcoeff.  The
 * block's rate inputs travel in svt_tq_block.pad_[0] (SVT_TQ_RATE_INFO).  d_tables / d_scan as for
 * svt_hip_coeff_rate_batch_device, with d_scan in the CANONICAL layout: for tx_size 0..3, for tx_type 0..3 the table
 * {scan[n], neighbors[2 (n + 1)]} of eb_vp9_scan_orders[tx_size][tx_type] (for 32x32 the four slots all hold the
 * default order); a block's table is found from its tx_size / tx_type.  4x4 blocks are walked with the three VP9 4x4 scan
 * orders compiled into the kernel (svt_hip_rate_scan4x4_table returns them; d_scan must hold the same, normative, ones). */
int32_t svt_hip_tq_rd_batch_device(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *d_recon,
                                   const svt_tq_block *d_blocks, const int32_t size_count[4],
                                   const svt_quant_tables *d_qtabs, const int16_t *d_iscan, int16_t *d_qcoeff,
                                   int16_t *d_dqcoeff, uint16_t *d_eob, uint64_t *d_dist,
                                   const struct svt_rate_tables *d_tables, const int16_t *d_scan, int32_t *d_bits);
/* The same for a batch whose blocks reconstruct into up to 8 different buffers: block b writes into recon_set[i] + recon_off with
 * i = bits 4-6 of pad_[0] (SVT_TQ_RECON_SET(i), OR-ed with the rate info).  recon_set is a HOST array of n_set device pointers; a
 * block whose i >= n_set is transformed and quantised like any other but its reconstruction is written nowhere.
 * In the reference every picture reconstructs into its own reference-picture buffer (Codec/EbEncDecProcess.c:5658-5674); a step of
 * a picture-level pipeline codes pictures of several mini-GOPs whose buffers need not lie within one 32-bit offset of each other:
 * this entry serves them with one launch per transform size.  d_bits == NULL: no rate (then d_tables / d_scan are ignored). */
#define SVT_TQ_RECON_SET(i) ((uint8_t)(((i) & 7) << 4))
int32_t svt_hip_tq_rd_batch_multi_device(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *const *recon_set, int32_t n_set,
                                         const svt_tq_block *d_blocks, const int32_t size_count[4], const svt_quant_tables *d_qtabs,
                                         const int16_t *d_iscan, int16_t *d_qcoeff, int16_t *d_dqcoeff, uint16_t *d_eob, uint64_t *d_dist,
                                         const struct svt_rate_tables *d_tables, const int16_t *d_scan, int32_t *d_bits);
/* host: the 4x4 scan order (16 entries) and neighbour pairs (32 entries) the fused rate pass uses for tx_type 0..3 */
int32_t svt_hip_rate_scan4x4_table(int32_t tx_type, int16_t out[48]);

int32_t svt_hip_tq_batch(svt_hip_ctx *ctx, const uint8_t *src, const uint8_t *pred, uint8_t *recon,
                         size_t plane_bytes, const svt_tq_block *blocks, int32_t n_blocks,
                         const svt_quant_tables *qtabs, int32_t n_qtabs, const int16_t *iscan, size_t iscan_count,
                         int16_t *qcoeff, int16_t *dqcoeff, size_t coeff_count, uint16_t *eob);

/* The decoder's half of the transform stage: quantised coefficients -> dequantise (DC dequant[0], AC dequant[1], the product kept in 16
 * bits as the encode pass and a non-high-bit-depth decoder keep it; 32x32: product / 2 towards zero) -> inverse DCT / ADST with the
 * eob shortcuts of VPX/vp9_idct.c:111-189 -> recon = clip(pred + residual); a block with eob 0 copies the prediction.
 * d_blocks / size_count: svt_hip_tq_batch_device's lists (grouped by size); of a descriptor pred_off / pred_stride, recon_off /
 * recon_stride, coeff_off, tx_type (ADST up to 16x16) and qtab are used, src_*, iscan_off, partial32 and do_recon are ignored (every
 * block is reconstructed).  d_qcoeff (16-byte aligned) and d_eob (per list entry) are INPUTS -- what svt_hip_tq_batch_device wrote, or
 * what a frame reader returned.  For such input d_recon receives exactly the bytes svt_hip_tq_batch_device's do_recon writes.
 * d_overflow (may be NULL): set to the number of coefficients, over the blocks with eob != 0, whose dequantised value (after the
 * division for 32x32) does not fit in 16 signed bits -- a conformant stream has none; the wrapped value is what gets used.
 * Asynchronous on the context's stream. */
int32_t svt_hip_recon_batch_device(svt_hip_ctx *ctx, const uint8_t *d_pred, uint8_t *d_recon, const svt_tq_block *d_blocks,
                                   const int32_t size_count[4], const svt_quant_tables *d_qtabs, const int16_t *d_qcoeff,
                                   const uint16_t *d_eob, uint32_t *d_overflow);

/* ------------------------------------------------------------------------------------------------ */
/* In-loop deblocking                                                                                 */
/* ------------------------------------------------------------------------------------------------ */

/* Bit-for-bit the reference's LOOP_FILTER_MASK (VPX/vp9_loopfilter.h; 160 bytes):
 * built on the host by eb_vp9_build_mask_frame (VPX/vp9_loopfilter.c:1548) and uploaded as is. */
typedef struct svt_lf_mask {
    uint64_t left_y[4];   /* per TX size */
    uint64_t above_y[4];
    uint64_t int_4x4_y;
    uint16_t left_uv[4];
    uint16_t above_uv[4];
    uint16_t int_4x4_uv;
    uint8_t  lfl_y[64];
} svt_lf_mask;

/* Per-level thresholds = loop_filter_info_n.lfthr[] (VPX/vp9_loopfilter.h: mblim/lim/hev_thr, each
 * SIMD_WIDTH=16 replicated bytes); only byte 0 of each is meaningful to the C kernels. */
typedef struct svt_lf_thresh {
    uint8_t mblim[64];
    uint8_t lim[64];
    uint8_t hev_thr[64];
} svt_lf_thresh;

/* Compute the thresholds exactly as eb_vp9_loop_filter_init/update_sharpness
 * (VPX/vp9_loopfilter.c:221-262) for a given sharpness level. */
void svt_hip_lf_thresh_init(svt_lf_thresh *t, int32_t sharpness_level);
/* eb_vp9_pick_filter_level's level-from-q rule (VPX/vp9_picklpf.c:37-89), 8-bit. */
int32_t svt_hip_lf_level_from_q(int32_t ac_q, int32_t is_key_frame);

/* The fields of ModeInfo (VPX/vp9_blockd.h) that the mask builder reads, one record per 8x8 unit of the picture
 * (mi_rows x mi_stride grid).  Every 8x8 unit covered by a prediction block carries that block's values, exactly as
 * every entry of cm->mi_grid_visible[] points at the block's ModeInfo in the reference. */
typedef struct svt_lf_mode_info {
    uint8_t sb_type;      /* BLOCK_SIZE: 0 4x4, 1 4x8, 2 8x4, 3 8x8, 4 8x16, 5 16x8, 6 16x16, 7 16x32, 8 32x16, 9 32x32,
                             10 32x64, 11 64x32, 12 64x64 (VPX/vp9_enums.h) */
    uint8_t tx_size;      /* TX_4X4 .. TX_32X32 */
    uint8_t skip;         /* no coefficients coded */
    uint8_t is_inter;     /* ref_frame[0] > INTRA_FRAME */
    uint8_t filter_level; /* get_filter_level(): lf_info.lvl[segment_id][ref_frame[0]][mode_lf_lut[mode]] */
    uint8_t pad_[3];
} svt_lf_mode_info;

/* Host-side: builds the LOOP_FILTER_MASK of every SB from the mode-info grid = eb_vp9_build_mask_frame
 * (VPX/vp9_loopfilter.c:1548-1571 -> eb_vp9_setup_mask :901-1040 / per block eb_vp9_build_mask :1587-1689).
 * lfm[(mi_row >> 3) * lfm_stride + (mi_col >> 3)] is written for every SB (zeroed first, like eb_vp9_setup_mask).
 * The result is the input of svt_hip_lf_frame (eb_vp9_adjust_mask is applied inside the filter, as in the reference). */
int32_t svt_hip_lf_build_masks(const svt_lf_mode_info *mi, int32_t mi_stride, int32_t mi_rows, int32_t mi_cols,
                               svt_lf_mask *lfm, int32_t lfm_stride);

/* 4:2:0 recon picture, planes filtered in place.  For the svt_hip_lf_* entry points: y, u, v, y_stride and uv_stride must be multiples
 * of 4 (u, v and uv_stride are not looked at when y_only is set), otherwise the call returns SVT_HIP_ERR_BAD_PARAMETER and launches
 * nothing.  No further alignment is needed: a stride may be larger than the width and sample (0, 0) may lie anywhere inside a padded
 * picture; only the width x height luma and width/2 x height/2 chroma samples are read or written.  Addresses, strides and widths
 * that are all multiples of 8 get the faster 8-byte copies.  Every size from one 8x8 block up is accepted, pictures one block high
 * or wide included. */
typedef struct svt_yuv_planes {
    uint8_t *y, *u, *v;    /* pointers to picture sample (0,0) of each plane */
    int32_t  y_stride, uv_stride;
    int32_t  width, height; /* luma dimensions (multiples of 8) */
} svt_yuv_planes;

/* Takes the context's per-SB edge-descriptor buffer (1 280 bytes per SB) for launches of up to n_pics pictures now: it grows on demand, but growing
 * waits for the context's stream.  The encoder library calls this when it is initialised. */
int32_t svt_hip_lf_reserve(svt_hip_ctx *ctx, int32_t n_pics, int32_t mi_rows, int32_t mi_cols);

/* = eb_vp9_loop_filter_frame(frame, cm, xd, lfm_base, filter_level, y_only=0, partial=0)
 * (VPX/vp9_loopfilter.c:1521-1546 -> loop_filter_rows :1456).  lfm: one mask per SB in raster order
 * [ceil(mi_rows/8)][lfm_stride].  Device pointers.  mi_rows/mi_cols in 8x8 units; d_recon->width / height must equal mi_cols * 8 /
 * mi_rows * 8, and the planes must meet svt_yuv_planes' alignment rule -- SVT_HIP_ERR_BAD_PARAMETER otherwise. */
int32_t svt_hip_lf_frame_device(svt_hip_ctx *ctx, const svt_yuv_planes *d_recon, const svt_lf_mask *d_lfm,
                                int32_t lfm_stride, const svt_lf_thresh *thr, int32_t mi_rows, int32_t mi_cols,
                                int32_t y_only);
/* Several independent frames in one launch (their SB-row wavefronts interleave and fill the GPU).  Host arrays of
 * n_pics entries; every pointer inside them is a device pointer. */
int32_t svt_hip_lf_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_yuv_planes *d_recon,
                                const svt_lf_mask *const *d_lfm, const int32_t *lfm_stride, const svt_lf_thresh *thr,
                                const int32_t *mi_rows, const int32_t *mi_cols, int32_t y_only);
/* Host-pointer convenience form (planes are tightly described by recon; rows*stride bytes copied). */
int32_t svt_hip_lf_frame(svt_hip_ctx *ctx, const svt_yuv_planes *recon, const svt_lf_mask *lfm, int32_t lfm_stride,
                         const svt_lf_thresh *thr, int32_t mi_rows, int32_t mi_cols, int32_t y_only);

/* ------------------------------------------------------------------------------------------------------------------
 * Inter prediction (8-tap motion compensation) of a whole picture -- SURVEY 8(f) row 2.
 *
 * Replaces the inter branch of prediction_fun_table (Codec/EbEncDecProcess.c:132, called per block and plane at
 * :277 / :3800): inter_prediction (Codec/EbIntraPrediction.c:49-72) -> build_inter_predictors
 * (VPX/vp9_reconinter.c:102-252) -> eb_vp9_clamp_mv_to_umv_border_sb (:72-92) -> inter_predictor
 * (VPX/vp9_reconinter.h:23-28) -> eb_vpx_convolve_copy / eb_vp9_convolve8[_horiz|_vert] and their _avg forms for the
 * second reference of a compound block (VPX/vpx_convolve.c:20-215) with the regular 8-tap kernel
 * (VPX/vp9_filter.c:32-47; the reference hard-wires eb_vp9_filter_kernels[0], vp9_reconinter.c:107-109).
 * Unscaled references only (sf->x_step_q4 == y_step_q4 == 16, the only case the reference's scale setup keeps,
 * VPX/vp9_scale.c:76-84, 126-128).  The prediction written here is the d_pred input of svt_hip_tq_batch_device.
 *
 * The picture is described the way the reference describes it after mode decision: one record per 8x8 unit of the
 * mode-info grid (cm->mi_grid_visible), every unit of a block carrying the block's values.  Blocks are the
 * reference's >= 8x8 partitions (inter_prediction asserts that no sub-8x8 inter block exists, :62-64), aligned to
 * their own size. */
typedef struct svt_mc_mode_info {
    int16_t mv_row[2], mv_col[2]; /* mi->mv[ref].as_mv, 1/8 luma sample (MV_PRECISION_Q3) */
    int8_t  ref_list[2];          /* reference list of ref 0 / ref 1: 0 = REF_LIST_0 (LAST_FRAME), 1 = REF_LIST_1, -1 = none;
                                     ref_list[0] < 0: not an inter block, nothing is written for this unit;
                                     ref_list[1] >= 0: compound (has_second_ref) */
    uint8_t bw8, bh8;             /* block width / height in 8x8 units (1, 2, 4, 8): num_8x8_blocks_wide/high_lookup[sb_type] */
} svt_mc_mode_info;               /* 12 bytes */

/* One picture: d_mi[mi_row * mi_stride + mi_col]; ref[l] = ref_pic_list[l] (planes need the reference's padding of
 * at least 64 + 16 samples around the luma picture and half of it around chroma, Codec/EbEncHandle.c:968-970: a
 * clamped MV reaches bw + 4 samples beyond the edge and the filter 4 more); pred = the prediction picture (sample
 * (0,0) pointers).  use_subpel = context_ptr->use_subpel_flag (0: the MVs are rounded to full samples the way
 * vp9_reconinter.c:175-188 does).  All pointers are device pointers.
 * What is read of a reference plane of W x H samples (luma, or chroma with its halved sizes), for a block of bw x bh samples of
 * that plane: rows -(bh + 7) .. H + bh + 6, and in each of them the bytes -(bw + 10) .. W + bw + 11 relative to the row's sample 0.
 * Rows are fetched as 16 aligned-down bytes around the 11 samples a 4-sample tile needs, so the fetch begins up to 3 bytes before
 * the first of them and ends up to 5 bytes after the last.  With 64x64 blocks that is rows -71 .. H + 70 and bytes -74 .. W + 75 in luma,
 * inside the padding of 80; in chroma (32x32, padding 40) it is rows -39 .. H + 38 but bytes -42 .. W + 43, so the first and last
 * bytes of a fetch can belong to the neighbouring row's padding: the padded plane must be one allocation, rows stride apart, which the
 * reference's buffers are.  No byte before the padded plane's first or after its last is read (tests/test_mc_model.py).
 * MVs are VP9's: MV_LOW .. MV_UPP = -16384 .. 16383.  Beyond that a luma MV wraps the way the reference's does when it is scaled
 * into int16 sixteenths (vp9_reconinter.c:76), e.g. 32767 becomes -2; nothing is read out of bounds for any int16 value. */
typedef struct svt_mc_picture {
    const svt_mc_mode_info *d_mi;
    int32_t        mi_stride, mi_rows, mi_cols;
    svt_yuv_planes ref[2];
    svt_yuv_planes pred;
    int32_t        use_subpel;
} svt_mc_picture;

/* n_pics independent pictures in one launch (host array of descriptors holding device pointers). */
int32_t svt_hip_inter_pred_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_mc_picture *pics);
/* Host-pointer convenience form for one picture: plane buffers are given WITH their padding (buf = first byte of the
 * padded plane, org_x/org_y = padding of the luma plane; chroma planes have half of it); the three prediction planes
 * are tight (width x height, width/2 x height/2) and are read back. */
typedef struct svt_mc_host_ref {
    const uint8_t *y, *u, *v;        /* padded planes */
    int32_t        y_stride, uv_stride;
    int32_t        org_x, org_y;     /* luma padding (even) */
} svt_mc_host_ref;
int32_t svt_hip_inter_pred_frame(svt_hip_ctx *ctx, const svt_mc_mode_info *mi, int32_t mi_stride, int32_t mi_rows,
                                 int32_t mi_cols, const svt_mc_host_ref ref[2], int32_t use_subpel, uint8_t *pred_y,
                                 uint8_t *pred_u, uint8_t *pred_v);

/* ------------------------------------------------------------------------------------------------------------------
 * Deblocked reconstruction -> reference picture: the step that closes the loop of the path.
 *
 * Replaces pad_ref_and_set_flags (Codec/EbEncDecProcess.c:4822-4851, called after the loop filter at :5696 for every picture
 * with is_used_as_reference_flag) -> eb_vp9_generate_padding (Codec/EbMcp.c:17-58) on Y with (pad_x, pad_y) and on Cb / Cr
 * with (pad_x >> 1, pad_y >> 1): the picture's edge samples are replicated into the border of its buffer, in place (in the
 * reference a reference picture's reconstruction buffer IS the reference picture, allocated with 64 + 16 samples of border,
 * Codec/EbEncHandle.c:968-971).  pics[i] gives the sample (0,0) pointers and strides of picture i (device memory; the
 * border of pad_y rows / pad_x columns around each plane must belong to the buffer: stride >= width + 2 pad_x).  The
 * padded planes are what svt_mc_picture.ref[] expects and what svt_hip_ref_handoff_device ships.  Host array of
 * descriptors; asynchronous on the context's stream. */
int32_t svt_hip_ref_pad_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_yuv_planes *pics, int32_t pad_x, int32_t pad_y);

/* ------------------------------------------------------------------------------------------------------------------
 * Coefficient rate estimation -- SURVEY 8(f) row 4 (with T3, svt_hip_tq_batch_dist_device, this completes what
 * perform_dist_rate_calc computes per transform block, Codec/EbEncDecProcess.c:700-745).
 *
 * Replaces coeff_rate_estimate (Codec/EbRateDistortionCost.c:55-172, libvpx's cost_coeffs) with
 * use_fast_coef_costing = 0, the only way the reference calls it (:736-745): the bits (scaled by 2^9, vp9_cost.h) of
 * the tokens of one quantised transform block under the frame's coefficient probabilities.
 * Tables are the reference's own, handed over by the caller the way the scan tables are for TQ:
 *   token_costs   = x->token_costs (VPX/vp9_block.h:140, filled by fill_token_costs, VPX/vp9_rd.c:93-107)
 *   value_cost    = eb_vp9_dct_cat_lt_10_value_cost[v], v = -66 .. 66, stored at index v + 66 (VPX/vp9_tokenize.c:52)
 *   cat6_low_cost = eb_vp9_cat6_low_cost[256], cat6_high_cost = eb_vp9_cat6_high_cost[64] (VPX/vp9_tokenize.c:82, 97)
 * and per (tx_size, tx_type) the scan order's `scan` (n entries) followed by its `neighbors` (2 (n + 1) entries)
 * (VPX/vp9_scan.c), concatenated in one int16 array; a block names its table by element offset (scan_off). */
typedef struct svt_rate_tables {
    uint32_t token_costs[4][2][2][6][2][6][12]; /* [tx_size][plane_type][is_inter][band][prev token == 0][ctx][token] */
    int32_t  value_cost[133];
    uint16_t cat6_low_cost[256];
    uint16_t cat6_high_cost[64];
    uint16_t pad_[2];
} svt_rate_tables;                            /* 56472 bytes */

typedef struct svt_rate_block {
    uint32_t coeff_off;  /* element offset of the block's n*n quantised coefficients (raster) in d_qcoeff; multiple of 8
                            (the TQ batch's coeff_off) */
    uint32_t scan_off;   /* element offset of {scan[n], neighbors[2 (n + 1)]} of the block's scan order */
    uint16_t eob;
    uint8_t  tx_size;    /* SVT_TX_* */
    uint8_t  plane_type; /* 0 luma, 1 chroma (get_plane_type) */
    uint8_t  is_inter;   /* is_inter_block(mi) */
    uint8_t  ctx;        /* combine_entropy_contexts(left, above): 0..2 (EbEncDecProcess.c:734) */
    uint8_t  pad_[2];
} svt_rate_block;        /* 16 bytes */

/* d_bits[b] = coeff_rate_estimate(...) of block b.  Device pointers; blocks in any order.
 * d_scan must be 4-byte aligned and hold at least SVT_RATE_SCAN_MIN_ENTRIES int16 entries (the size of the four 4x4 and
 * four 8x8 tables): every workgroup stages that prefix in LDS before it looks at a block (with the canonical layout --
 * the 4x4 tables of tx_type 0..3 first, then the 8x8 ones -- those blocks read their scan from LDS; any other layout
 * is still correct, the entries are then read in place).  The host-pointer form pads a shorter array itself. */
#define SVT_RATE_SCAN_MIN_ENTRIES 976
int32_t svt_hip_coeff_rate_batch_device(svt_hip_ctx *ctx, const int16_t *d_qcoeff, const svt_rate_block *d_blocks,
                                        int32_t n_blocks, const svt_rate_tables *d_tables, const int16_t *d_scan,
                                        int32_t *d_bits);
/* Host-pointer convenience form. */
int32_t svt_hip_coeff_rate_batch(svt_hip_ctx *ctx, const int16_t *qcoeff, size_t coeff_count, const svt_rate_block *blocks,
                                 int32_t n_blocks, const svt_rate_tables *tables, const int16_t *scan, size_t scan_count,
                                 int32_t *bits);

/* ------------------------------------------------------------------------------------------------------------------
 * Coefficient tokenisation: the data-parallel half of entropy coding.
 *
 * Replaces eb_vp9_tokenize_sb -> tokenize_b (VPX/vp9_tokenize.c:275-349, 397-430) as eb_vp9_entropy_coding_kernel calls it for
 * every coded block in front of the bool coder (Codec/EbEntropyCodingProcess.c:381-398).  The reference codes with the default
 * probabilities (its count-based update is compiled out, VPX/vp9_tokenize.c:301-304), so a token stream plus the fixed tables is
 * all the arithmetic coder needs (the bool coder and the mode-info stages of key frames and of inter pictures follow below); the
 * two headers and the packets are the frame stage's (further below).
 *
 * One token = one uint32_t record: extra << 16 | prob_row << 4 | token.
 *   token     ZERO 0, ONE..FOUR 1..4, CAT1..CAT6 5..10 (|v| 5-6, 7-10, 11-18, 19-34, 35-66, >= 67), EOB 11 (at scan position eob
 *             when eob < n) -- VPX/vp9_entropy.h:28-52
 *   extra     ((|v| - base of the token) << 1 | (v < 0)) & 0xffff: the reference's int16 EXTRABIT (VPX/vp9_tokenize.h:34, 100-111); 0
 *             for ZERO and EOB
 *   prob_row  (((tx_size * 2 + plane_type) * 2 + is_inter) * 6 + band) * 6 + ctx (< 576): TOKENEXTRA.context_tree =
 *             &coef_probs[0][0][0][0][0][0] + 3 * prob_row
 * counts[SVT_TOK_COUNTS] = td->rd_counts.coef_counts[tx_size][plane_type][is_inter][band][ctx][token] = counts[prob_row * 12 + token]
 * (eob_branch is compiled out in the reference and is not produced here: svt_hip_coef_update_batch_device counts it from the records). */
#define SVT_TOK_EOB 11
#define SVT_TOK_COUNTS 6912   /* 4 * 2 * 2 * 6 * 6 * 12 */
#define SVT_TOK_NONE 0xFFFFFFFFu
#define SVT_TOK_TOKEN(rec) ((uint32_t)(rec) & 15u)
#define SVT_TOK_PROB_ROW(rec) (((uint32_t)(rec) >> 4) & 0xfffu)
#define SVT_TOK_EXTRA(rec) ((uint32_t)(rec) >> 16)
#define SVT_TOK_RECORD(extra, prob_row, token) ((uint32_t)(extra) << 16 | (uint32_t)(prob_row) << 4 | (uint32_t)(token))

/* host: the scan orders the tokeniser (and the rate estimation) walk, in the canonical layout svt_rate_block.scan_off addresses:
 * for tx_size 0..3, for tx_type 0..3 {scan[n], neighbors[2 (n + 1)]} = eb_vp9_scan_orders[tx_size][tx_type].scan / .neighbors
 * (VPX/vp9_scan.c); offsets16[tx_size * 4 + tx_type] = element offset of a table.  Built at first use from the committed inverse
 * scans (svt_hip_vp9_iscan_tables) and the neighbour rule of csrc/tokenize_core.h. */
const int16_t *svt_hip_vp9_scan_tables(const uint32_t **offsets16, int32_t *entries);

/* Block-level form = tokenize_b per block (VPX/vp9_tokenize.c:275-349): the blocks are the records the rate estimation takes, their
 * scan_off in the canonical layout (it names the transform type).  d_tok_off[n_blocks + 1] is WRITTEN: block b's tokens are
 * d_tokens[d_tok_off[b] .. d_tok_off[b + 1]), eob + (eob < n) of them, in scan order; the last entry is the total.  Nothing is
 * written at or beyond d_tokens + capacity (a total above capacity tells the caller; the contents are then unspecified).  d_counts
 * (SVT_TOK_COUNTS, may be NULL) is overwritten.  Asynchronous on the context's stream. */
int32_t svt_hip_tokenize_blocks_device(svt_hip_ctx *ctx, const int16_t *d_qcoeff, const svt_rate_block *d_blocks, int32_t n_blocks,
                                       uint32_t *d_tokens, uint32_t capacity, uint32_t *d_tok_off, uint32_t *d_counts);
/* Host-pointer convenience form. */
int32_t svt_hip_tokenize_blocks(svt_hip_ctx *ctx, const int16_t *qcoeff, size_t coeff_count, const svt_rate_block *blocks, int32_t n_blocks,
                                uint32_t *tokens, uint32_t capacity, uint32_t *tok_off, uint32_t *counts);

/* host form of the block-level tokeniser (the same text, csrc/tokenize_core.h), pure CPU, host pointers; validates the blocks */
int32_t svt_hip_tokenize_blocks_host(const int16_t *qcoeff, size_t coeff_count, const svt_rate_block *blocks, int32_t n_blocks, uint32_t *tokens,
                                     uint32_t capacity, uint32_t *tok_off, uint32_t *counts);

/* Picture-level form = eb_vp9_tokenize_sb over every coded block of a picture (VPX/vp9_tokenize.c:397-430 as
 * Codec/EbEntropyCodingProcess.c:381-398 calls it, above / left entropy contexts cleared as :88-105 clears them for the one tile),
 * from what svt_hip_encdec_batch_device / svt_hip_encdec_intra_device leave on the device: the grid with its skip flags, the
 * position-addressed coefficients, the eob map.  A skipped block emits nothing and its contexts are 0; every transform block of a
 * coded block emits eob + (eob < n) tokens.  Token order = coefficient order: SBs raster; inside an SB Y, Cb, Cr; inside a plane area
 * transform blocks in z-order of their origin unit; inside a block scan order.
 *   d_tok_off  shape of the eob map: at the origin unit of every transform block of a coded block the offset of its first token,
 *              SVT_TOK_NONE everywhere else
 *   d_sb_off   n_sb + 1 entries: first token of every SB; the last entry is the picture's total, written ALWAYS.  When it exceeds
 *              capacity nothing is written at or beyond d_tokens + capacity and the contents are unspecified
 *   d_counts   SVT_TOK_COUNTS entries, overwritten; may be NULL */
typedef struct svt_tok_picture {
    const svt_lf_mode_info *d_lf_mi;
    const int16_t          *d_qcoeff;   /* n_sb * SVT_SB_COEFFS, 16-byte aligned */
    const uint16_t         *d_eob_map;
    uint32_t               *d_tokens;
    uint32_t                capacity;   /* records d_tokens can hold */
    uint32_t                pad_;
    uint32_t               *d_tok_off;
    uint32_t               *d_sb_off;
    uint32_t               *d_counts;
} svt_tok_picture;
/* n_pics (<= 32) pictures of one geometry in one call (host array of descriptors holding device pointers).  Asynchronous on the
 * context's stream: behind svt_hip_encdec_batch_device / svt_hip_encdec_intra_device on the same context it needs no host round trip. */
int32_t svt_hip_tokenize_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_tok_picture *pics, int32_t width, int32_t height, int32_t mi_stride);
/* host form of the same text (csrc/tokenize_core.h), pure CPU; the svt_tok_picture fields are host pointers */
int32_t svt_hip_tokenize_picture(const svt_tok_picture *pic, int32_t width, int32_t height, int32_t mi_stride);
/* records a picture emits at most: every coefficient a token (W*H*3/2), plus room for an EOB token per 4x4 block (W*H*3/32) */
uint32_t svt_hip_tokenize_capacity(int32_t width, int32_t height);

/* ------------------------------------------------------------------------------------------------------------------
 * Bool coder: token streams (and raw bools) -> VP9 arithmetic-coded bytes.
 *
 * Replaces pack_mb_tokens over vpx_write (VPX/vp9_bitstream.c:98-162, VPX/bitwriter.h:34-84) between eb_vp9_start_encode and
 * eb_vp9_stop_encode (VPX/bitwriter.c): the bytes of one tile.  A stream is coded as (128, 0), its bools, 32 x (128, 0), plus one zero
 * byte when the last byte looks like a superframe marker ((last & 0xe0) == 0xc0).
 *
 *   bool record   uint16_t, bit << 8 | prob, prob in 1 .. 255
 *   token record  the tokeniser's uint32_t (above); its bools are node 0 (bit = token != EOB; left out when the record's band is not
 *                 0 and the record in front of it in the segment is ZERO), node 1, node 2, the eb_vp9_coef_con_tree walk over
 *                 pareto[probs[2] - 1], the category bits MSB first, the sign at probability 128 -- 22 bools at most
 *   segment       {first, count, kind}: kind 0 = `count` token records from d_tokens + first, kind 1 = `count` bool records from
 *                 d_bools + first.  Segments are coded in list order; a transform block never straddles two segments.
 * The tables are the caller's data (the frame's coefficient probabilities and the two constant tables of VPX/vp9_entropy.c),
 * uploaded once per context.  The raw bools and the segment list of a tile come from the mode-info stages below (key frames:
 * svt_hip_modes_kf_batch_device, inter pictures: svt_hip_modes_inter_batch_device behind svt_hip_md_inter_modes_batch_device); the
 * uncompressed and compressed headers and the packet around the tile are the frame stage's (svt_hip_frame_header_host,
 * svt_hip_frame_batch_device); delivery through libSvtVp9Enc.so is not here yet. */
typedef struct svt_bool_tables {
    uint8_t coef_probs[576 * 3]; /* [prob_row][node]: cm->fc->coef_probs flattened */
    uint8_t pareto[255][8];      /* eb_vp9_pareto8_full */
    uint8_t cat_probs[6][14];    /* eb_vp9_extra_bits[CATEGORY1_TOKEN + i].prob (8-bit depth), unused entries 0 */
} svt_bool_tables;
typedef struct svt_bool_segment {
    uint32_t first, count, kind;
} svt_bool_segment;
#define SVT_BOOL_RECORD(bit, prob) ((uint16_t)((bit) << 8 | (prob)))
#define SVT_BOOL_MAX_PER_TOKEN 22
#define SVT_BOOL_SIZE_OVERFLOW 0xFFFFFFFFu
/* one stream of a batch; every pointer is a device pointer.
 *   d_segments  NULL: the stream is the token records d_tokens[0 .. n_tokens) (or *d_n_tokens of them when d_n_tokens is set, e.g.
 *               the last entry of the tokeniser's d_sb_off: a count only the device knows)
 *   max_bools   what the context's scratch is sized for (its kernels' grids as well): an upper bound of the stream's bools, e.g.
 *               svt_hip_boolcode_bools_capacity(tokens).  A stream with more bools is not coded: *d_size = SVT_BOOL_SIZE_OVERFLOW;
 *               the same answer for a stream with a non-empty segment of an unknown kind or of a kind whose buffer pointer is NULL
 *               (the list lives on the device: the entry point cannot look at it)
 *   d_size      WRITTEN always: the stream's size in bytes, also when it exceeds capacity -- nothing is then written at or beyond
 *               d_bytes + capacity and the contents are unspecified */
typedef struct svt_bool_stream {
    const uint32_t         *d_tokens;
    const uint16_t         *d_bools;
    const svt_bool_segment *d_segments;
    const uint32_t         *d_n_tokens;
    uint32_t                n_segments, n_tokens, max_bools, capacity;
    uint8_t                *d_bytes;
    uint32_t               *d_size;
} svt_bool_stream;
#define SVT_BOOL_MAX_STREAMS 32

int32_t svt_hip_boolcode_set_tables(svt_hip_ctx *ctx, const svt_bool_tables *tables);
/* n_streams (<= SVT_BOOL_MAX_STREAMS) streams in one call (host array of descriptors holding device pointers).  Asynchronous on the
 * context's stream: behind svt_hip_tokenize_batch_device on the same context it needs no host round trip.  Bit positions are 32-bit:
 * a stream with 7 * (max_bools + 33) >= 2^32 is refused. */
int32_t svt_hip_boolcode_batch_device(svt_hip_ctx *ctx, int32_t n_streams, const svt_bool_stream *streams);
/* host-pointer convenience form of one stream (segments NULL: all n_tokens records); *size as d_size above */
int32_t svt_hip_boolcode(svt_hip_ctx *ctx, const uint32_t *tokens, uint32_t n_tokens, const uint16_t *bools, uint32_t n_bools,
                         const svt_bool_segment *segments, uint32_t n_segments, uint8_t *bytes, uint32_t capacity, uint32_t *size);
/* the same rules (csrc/boolcode_core.h) in front of the plain serial writer, pure CPU, host pointers */
int32_t svt_hip_boolcode_host(const svt_bool_tables *tables, const uint32_t *tokens, uint32_t n_tokens, const uint16_t *bools, uint32_t n_bools,
                              const svt_bool_segment *segments, uint32_t n_segments, uint8_t *bytes, uint32_t capacity, uint32_t *size);
/* bytes n_bools bools occupy at most (7 bits a bool, the 33 framing bools, the marker byte); bools n_tokens records expand to at most */
uint32_t svt_hip_boolcode_capacity(uint32_t n_bools);
uint32_t svt_hip_boolcode_bools_capacity(uint32_t n_tokens);
/* the kernels' constants: bools per chunk (K) and chunks per tile of the chain kernel */
void svt_hip_boolcode_geometry(int32_t *bools_per_chunk, int32_t *chunks_per_tile);
/* svt_hip_boolcode_batch_device with coefficient probabilities per stream: d_coef_probs is a HOST array of n_streams DEVICE pointers to
 * 1 728 bytes each ([prob_row][node], e.g. svt_cu_picture.d_probs); a NULL entry (or d_coef_probs NULL) means the context's table.  pareto
 * and cat_probs are the context's for every stream.  The same kernels; the expand kernel alone reads the table and is instantiated twice,
 * so the entry above runs the code it ran before this one existed. */
int32_t svt_hip_boolcode_batch_tables_device(svt_hip_ctx *ctx, int32_t n_streams, const svt_bool_stream *streams, const uint8_t *const *d_coef_probs);

/* ------------------------------------------------------------------------------------------------------------------
 * Forward coefficient-probability update: a picture's token stream and coef_counts -> the coefficient section of its compressed header
 * (as bool records, between the records in front of and behind it) and the probabilities its tile is then coded with.
 *
 * Replaces update_coef_probs (VPX/vp9_bitstream.c:669-687).  The reference leaves FRAME_COUNTS zeroed and so writes one "no update" bit
 * per transform size; its update code is alive and is what this stage restates (rules: csrc/coef_update_core.h): build_tree_distribution
 * with eob_branch counted from the token stream, the TWO_LOOP decision per transform size, the savings searches and the
 * sub-exponential code of VPX/vp9_subexp.c with coeff_prob_appx_step 1.  All sums are 64-bit: equal to the reference wherever its 32-bit
 * sums do not wrap (a branch count of about 2^31 / 4096), true beyond.
 *
 *   d_tokens       the picture's token records in stream order (svt_hip_tokenize_batch_device's d_tokens), scanned as ONE run
 *   d_n_tokens     device count of them (the last entry of the tokeniser's d_sb_off), or NULL: n_tokens.  max_tokens sizes the count
 *                  kernel's grid and bounds the scan: records at or beyond it are not read
 *   d_counts       SVT_TOK_COUNTS coef_counts (the tokeniser's d_counts)
 *   d_old_probs    1 728 bytes the update is measured against and coded relative to; NULL: the coef_probs of the context's
 *                  svt_hip_boolcode_set_tables table.  Callers that code every picture from the default probabilities and send
 *                  refresh_frame_context = 0 (all of today's) leave it NULL: the pictures of a batch are then independent.  Chaining
 *                  pictures (refresh_frame_context = 1) is a later change and needs only this pointer.  Entries are 1 .. 255; a 0 is read as 1
 *   d_eob_branch   576 counts, overwritten: records of prob_row r that code node 0
 *   d_probs        1 728 bytes, overwritten: the probabilities after the update (the old ones where nothing is sent)
 *   d_hdr_bools    the compressed header's complete record list prefix || coefficient section || suffix, svt_hip_coef_update_bools_capacity()
 *                  records; *d_n_hdr_bools = their number; *d_segment = {0, n, 1}: svt_hip_boolcode_batch_device codes the header as a
 *                  bool-only stream (d_bools = d_hdr_bools, d_segments = d_segment, n_segments = 1)
 *   prefix, suffix the records in front of and behind the section (svt_hip_frame_header_parts_host); they travel inside the descriptor
 *   d_result       svt_cu_result: per transform size the entries that update (counted also when the size is not sent), whether the size
 *                  is sent, its summed savings in 1/512 bit as the decision saw them (0 for a size with tx_total <= 20); the header's bools
 * sizeof(svt_cu_picture) = 528, sizeof(svt_cu_result) = 72. */
#define SVT_CU_ROWS 576
#define SVT_CU_PROBS 1728
#define SVT_CU_ENTRIES 396          /* per transform size: 132 rows that exist x 3 nodes */
#define SVT_CU_MAX_PER_ENTRY 12     /* the flag, 3 bits of the range, 7 + 1 bits of encode_uniform */
#define SVT_CU_SECTION_MAX (4 * (1 + SVT_CU_ENTRIES * SVT_CU_MAX_PER_ENTRY))
#define SVT_CU_PREFIX_MAX 8
#define SVT_CU_SUFFIX_MAX 208
#define SVT_CU_MAX_PICS 32
typedef struct svt_cu_result {
    uint32_t updated[4];
    uint32_t sent[4];
    uint32_t hdr_bools;
    uint32_t tokens;       /* records scanned */
    int64_t  savings[4];
} svt_cu_result;
typedef struct svt_cu_picture {
    const uint32_t   *d_tokens;
    const uint32_t   *d_n_tokens;
    const uint32_t   *d_counts;
    const uint8_t    *d_old_probs;
    uint32_t         *d_eob_branch;
    uint8_t          *d_probs;
    uint16_t         *d_hdr_bools;
    uint32_t         *d_n_hdr_bools;
    svt_bool_segment *d_segment;
    svt_cu_result    *d_result;
    uint32_t          n_tokens, max_tokens;
    uint16_t          n_prefix, n_suffix;
    uint16_t          prefix[SVT_CU_PREFIX_MAX];
    uint16_t          suffix[SVT_CU_SUFFIX_MAX];
    uint32_t          pad_;
} svt_cu_picture;
/* n_pics (<= SVT_CU_MAX_PICS) pictures in one call (host array of descriptors holding device pointers): the count kernel (an LDS
 * histogram per workgroup, partial histograms in a context buffer, no global atomics), the decide kernel (one workgroup per picture and
 * transform size) and the kernel that joins the sections.  Asynchronous on the context's stream: behind svt_hip_tokenize_batch_device
 * and in front of svt_hip_boolcode_batch_tables_device it needs no host round trip.  Refused, with nothing launched: a null pointer
 * (d_n_tokens and d_old_probs may be NULL; d_tokens may be NULL when max_tokens is 0), n_pics out of range, n_prefix / n_suffix beyond
 * their arrays, svt_hip_boolcode_set_tables not called. */
int32_t svt_hip_coef_update_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_cu_picture *pics);
/* host form of the same text (csrc/coef_update_core.h), pure CPU; the svt_cu_picture fields are host pointers; d_old_probs NULL:
 * tables->coef_probs */
int32_t svt_hip_coef_update_picture(const svt_cu_picture *pic, const svt_bool_tables *tables);
/* records d_hdr_bools must hold: SVT_CU_PREFIX_MAX + SVT_CU_SECTION_MAX + SVT_CU_SUFFIX_MAX */
uint32_t svt_hip_coef_update_bools_capacity(void);
/* the count kernel's constants: records per workgroup and pass, workgroups of a picture at most */
void svt_hip_coef_update_geometry(int32_t *records_per_pass, int32_t *max_workgroups);
/* the tables behind the rules, for tests: the 256 probability costs (eb_vp9_prob_cost); remap[(newp - 1) * 255 + oldp - 1] for all 255 x 255
 * pairs (0 on the diagonal) and bits[] likewise, the bools the update of that pair writes */
const uint16_t *svt_hip_coef_update_cost_table(void);
void svt_hip_coef_update_remap_tables(uint8_t *remap, uint8_t *bits);

/* ------------------------------------------------------------------------------------------------------------------
 * Key-frame mode-info syntax: the grid of an intra-only picture -> the raw bools and the segment list that, with the tokeniser's
 * records, make the bool coder write the complete compressed tile data of the picture.
 *
 * Replaces, for intra-only pictures, what eb_vp9_entropy_coding_kernel codes per block in front of its tokens
 * (Codec/EbEntropyCodingProcess.c:110-442): write_partition (VPX/vp9_bitstream.c:399-417) at every node of an SB's quad-tree that
 * reaches into the picture and write_mb_modes_kf (:323-358) at every leaf -- skip, luma mode(s), chroma mode; no transform size
 * (tx_mode is ALLOW_32X32) and no segment id.  Every context is read from the grid (csrc/modeinfo_core.h says why that is the serial
 * walk's value).  Chain: intra encode pass -> tokeniser -> this -> bool coder, all on one context's stream, no host round trip; the
 * result is what the reference writes between eb_vp9_start_encode and eb_vp9_stop_encode.
 *
 * The tables are the caller's data (VPX/vp9_entropymode.c: eb_vp9_kf_y_mode_prob, eb_vp9_kf_uv_mode_prob, eb_vp9_kf_partition_probs;
 * the frame's skip probabilities), uploaded once per context. */
typedef struct svt_modes_tables {
    uint8_t kf_y_mode_prob[10][10][9]; /* [above][left][node] */
    uint8_t kf_uv_mode_prob[10][9];    /* [luma mode][node] */
    uint8_t kf_partition_probs[16][3]; /* [4 * level (8x8 .. 64x64) + 2 * left + above][node] */
    uint8_t skip_probs[3];             /* [above skip + left skip] */
} svt_modes_tables;
#define SVT_MODES_BAD_GRID 0xFFFFFFFFu
/* one picture of a batch; every pointer is a device pointer (host pointers in the host form).
 *   d_lf_mi     the grid as svt_hip_encdec_intra_device takes it (sb_type 0 / 3 / 6 / 9, modes in pad_[1], pad_[2] and the nibbles of
 *               pad_[0]; `skip` as the encode pass wrote it), and also sb_type 12 with tx_size 3
 *   d_eob_map, d_tok_off   the tokeniser's input and output: first token and token count of every leaf's Y, Cb and Cr runs
 *   d_bools     WRITTEN: the picture's bool records in coding order; nothing is written at or beyond d_bools + capacity
 *               (svt_hip_modes_bools_capacity always suffices).  4-byte aligned
 *   d_segments  WRITTEN, every one of the svt_hip_modes_segments records: four per 8x8 unit, SBs raster, units in z-order --
 *               {kind 1: the bools that start at the unit}, {kind 0: Y tokens}, {Cb}, {Cr}; count 0 where the unit is no leaf's origin,
 *               lies outside the picture, or the leaf is skipped.  Handed to the bool coder with the tokeniser's d_tokens and d_bools
 *               the list codes the tile.  16-byte aligned
 *   d_n_bools   WRITTEN always: the picture's bools, also when they exceed capacity; SVT_MODES_BAD_GRID for a grid this entry does not
 *               take (a rectangular sb_type, is_inter != 0, a mode above 9, a block that crosses the picture edge or overlaps another, a
 *               tx_size other than the block's largest up to 32x32): every segment is then empty */
typedef struct svt_modes_picture {
    const svt_lf_mode_info *d_lf_mi;
    const uint16_t         *d_eob_map;
    const uint32_t         *d_tok_off;
    uint16_t               *d_bools;
    svt_bool_segment       *d_segments;
    uint32_t               *d_n_bools;
    uint32_t                capacity;   /* records d_bools can hold */
    uint32_t                pad_;
} svt_modes_picture;
int32_t svt_hip_modes_set_tables(svt_hip_ctx *ctx, const svt_modes_tables *tables);
/* n_pics (<= 32) pictures of one geometry in one call (host array of descriptors holding device pointers).  Asynchronous on the
 * context's stream: behind svt_hip_tokenize_batch_device and in front of svt_hip_boolcode_batch_device it needs no host round trip. */
int32_t svt_hip_modes_kf_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_modes_picture *pics, int32_t width, int32_t height, int32_t mi_stride);
/* host form of the same text (csrc/modeinfo_core.h), pure CPU, host pointers; also checks the per-unit bound of the capacity */
int32_t svt_hip_modes_kf_picture(const svt_modes_tables *tables, const svt_modes_picture *pic, int32_t width, int32_t height, int32_t mi_stride);
/* records of a picture's segment list (a host value: svt_bool_stream.n_segments); bools a picture emits at most: its 8x8 units times
 * 48 = 4 partition symbols of 3 bools + skip + (4 luma modes + the chroma mode) of 7 bools */
uint32_t svt_hip_modes_segments(int32_t width, int32_t height);
uint32_t svt_hip_modes_bools_capacity(int32_t width, int32_t height);

/* ------------------------------------------------------------------------------------------------------------------
 * Inter mode-info syntax: the grid of an inter picture -> the raw bools and the segment list of its tile, the counterpart of the
 * key-frame entry above for every other picture.
 *
 * Replaces what eb_vp9_entropy_coding_kernel codes per block in front of its tokens in a picture that is not intra-only
 * (Codec/EbEntropyCodingProcess.c:60-449): write_partition (VPX/vp9_bitstream.c:399-417) under the frame's partition probabilities
 * and pack_inter_mode_mvs (:206-321) at every leaf -- skip, intra/inter, then for an intra block its luma mode(s) and chroma mode, for
 * an inter block the reference frames (write_ref_frames, :170-204), the inter mode and, for NEWMV, one motion-vector difference per
 * reference (eb_vp9_encode_mv, VPX/vp9_encodemv.c:33-66, 201-220).  No transform size (tx_mode is ALLOW_32X32), no segment id, no
 * interpolation filter (fixed); no inter block below 8x8.  Every context reads the leaves above and left of the leaf's origin
 * (VPX/vp9_pred_common.c) and is taken from the grid (csrc/modeinfo_inter_core.h).  Chain: encode pass -> tokeniser -> this -> bool
 * coder on one context's stream, no host round trip.  mbmi_ext's values -- the MV references and the mode context that
 * eb_vp9_find_mv_refs derives -- are inputs here exactly as they are inputs of pack_inter_mode_mvs; svt_hip_mvrefs_batch_device below
 * derives them on the device, and svt_hip_md_inter_modes_batch_device produces the whole records from the encode pass's grids.  The two headers and the packet around the tile are the frame stage's (svt_hip_frame_header_host,
 * svt_hip_frame_batch_device); delivery through libSvtVp9Enc.so is not here yet.
 *
 * The tables are the caller's data (the frame context cm->fc), uploaded once per context. */
typedef struct svt_modes_mv_comp {       /* nmv_component (VPX/vp9_entropymv.h) */
    uint8_t sign, classes[10], class0[1], bits[10], class0_fp[2][3], fp[3], class0_hp, hp;
} svt_modes_mv_comp;                     /* 33 bytes */
typedef struct svt_modes_inter_tables {
    uint8_t partition_prob[16][3];       /* [4 * level (8x8 .. 64x64) + 2 * left + above][node], as kf_partition_probs */
    uint8_t skip_probs[3];               /* [above skip + left skip] */
    uint8_t intra_inter_prob[4];
    uint8_t comp_inter_prob[5];
    uint8_t single_ref_prob[5][2];
    uint8_t comp_ref_prob[5];
    uint8_t y_mode_prob[4][9];           /* [size group: 4x4 blocks, 8x8, 16x16, 32x32 and 64x64][node] */
    uint8_t uv_mode_prob[10][9];         /* [luma mode][node] */
    uint8_t inter_mode_probs[7][3];      /* [mode context][node] */
    uint8_t mv_joints[3];
    svt_modes_mv_comp mv_comps[2];       /* 0: vertical (row), 1: horizontal (column) */
} svt_modes_inter_tables;                /* 291 bytes */
/* what the grid records lack, one record per 8x8 unit (the grid's mi_stride).  ref_frame is read from every unit (neighbours read
 * it), the other fields at the origin of a leaf only. */
typedef struct svt_mi_inter_ext {
    int16_t ref_mv_row[2], ref_mv_col[2]; /* mbmi_ext->ref_mvs[ref_frame[ref]][0] of ref 0 / ref 1, 1/8 sample */
    uint8_t ref_frame[2];                 /* 0 intra, 1 LAST, 2 GOLDEN, 3 ALTREF; ref_frame[1] == 0: no second reference */
    uint8_t mode;                         /* inter block: 10 NEARESTMV, 11 NEARMV, 12 ZEROMV, 13 NEWMV */
    uint8_t mode_context;                 /* mbmi_ext->mode_context[ref_frame[0]], 0 .. 6 */
} svt_mi_inter_ext;                       /* 12 bytes */
#define SVT_MODES_SINGLE_REFERENCE 0
#define SVT_MODES_COMPOUND_REFERENCE 1
#define SVT_MODES_REFERENCE_SELECT 2
/* one picture of a batch; the first eight fields are svt_modes_picture's and mean the same (an intra block keeps its modes in pad_[1],
 * pad_[2] and the nibbles of pad_[0]).
 *   d_mc_mi     the grid the encode pass holds: the motion vectors are read from it (mv_row / mv_col of ref 0 / 1)
 *   d_ext       the extension records
 *   reference_mode .. ref_frame_sign_bias   cm->reference_mode, cm->allow_high_precision_mv, and what
 *               eb_vp9_setup_compound_reference_mode leaves in cm->comp_fixed_ref / comp_var_ref from cm->ref_frame_sign_bias
 *   d_n_bools   SVT_MODES_BAD_GRID also for: an inter block below 8x8; is_inter, d_mc_mi's ref_list and ref_frame disagreeing about
 *               inter or compound; a reference frame above 3; a compound block under SINGLE_REFERENCE (a single one under
 *               COMPOUND_REFERENCE) or one whose references are not comp_fixed_ref plus one of comp_var_ref; an inter mode outside
 *               10 .. 13; mode_context above 6; a motion-vector difference of a NEWMV block beyond +-16383 in a component */
typedef struct svt_modes_inter_picture {
    const svt_lf_mode_info *d_lf_mi;
    const uint16_t         *d_eob_map;
    const uint32_t         *d_tok_off;
    uint16_t               *d_bools;
    svt_bool_segment       *d_segments;
    uint32_t               *d_n_bools;
    uint32_t                capacity;   /* records d_bools can hold */
    uint32_t                pad_;
    const svt_mc_mode_info *d_mc_mi;
    const svt_mi_inter_ext *d_ext;
    uint8_t                 reference_mode, allow_hp, comp_fixed_ref, comp_var_ref[2], ref_frame_sign_bias[4];
    uint8_t                 pad2_[7];
} svt_modes_inter_picture;              /* 88 bytes */
int32_t svt_hip_modes_inter_set_tables(svt_hip_ctx *ctx, const svt_modes_inter_tables *tables);
/* n_pics (<= 32) pictures of one geometry in one call; their frame parameters may differ.  Asynchronous on the context's stream:
 * behind svt_hip_tokenize_batch_device and in front of svt_hip_boolcode_batch_device it needs no host round trip.  The segment list
 * has the key-frame entry's format and length (svt_hip_modes_segments). */
int32_t svt_hip_modes_inter_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_modes_inter_picture *pics, int32_t width, int32_t height,
                                         int32_t mi_stride);
/* host form of the same text (csrc/modeinfo_inter_core.h), pure CPU, host pointers; also checks the per-unit bound of the capacity */
int32_t svt_hip_modes_inter_picture(const svt_modes_inter_tables *tables, const svt_modes_inter_picture *pic, int32_t width, int32_t height,
                                    int32_t mi_stride);
/* bools a picture emits at most: its 8x8 units times 111 (derived in csrc/modeinfo_inter_core.h) */
uint32_t svt_hip_modes_inter_bools_capacity(int32_t width, int32_t height);

/* ------------------------------------------------------------------------------------------------------------------
 * MV-reference derivation: the grid of an inter picture -> the MV references and mode contexts the inter mode-info entry above takes
 * as inputs, and the NEARESTMV / NEARMV candidates of every block.
 *
 * Replaces eb_vp9_find_mv_refs (VPX/vp9_mvref_common.c:20-197 with the tables and macros of vp9_mvref_common.h) as
 * prepare_fast_loop_candidates calls it per block of 8x8 or larger and per reference frame of a picture that is not intra-only
 * (Codec/EbModeDecision.c:638-672), and with it the filling of mbmi_ext->ref_mvs[..][0] and mbmi_ext->mode_context[..]: the eight
 * positions of the block's size (mv_ref_blocks), the counter of the two nearest (mode_2_counter, counter_to_context), same-reference
 * candidates first, then -- unless cm->use_prev_frame_mvs restricts the derivation -- other references' MVs with the sign inversion
 * of scale_mv, and clamp_mv_ref.  Spatial candidates only, as in the reference; one tile.  Every position lies above or left of the
 * block, so the derivation is a function of the grid (csrc/mvrefs_core.h) and runs per leaf in parallel.  Chain: encode pass ->
 * tokeniser -> this -> inter mode info -> bool coder on one context's stream, no host round trip: d_ext_out is the d_ext of
 * svt_hip_modes_inter_batch_device. */
typedef struct svt_mvref_cand {             /* 32 bytes */
    int16_t mv_row[3][2], mv_col[3][2];     /* [ref_frame - 1][candidate], clamped as the reference clamps them */
    uint8_t count[3];                       /* eb_vp9_find_mv_refs' return value 0 / 1 / 2; 0xFF: not asked for in ref_mask */
    uint8_t mode_context;
    uint8_t pad_[4];
} svt_mvref_cand;
/* one picture of a batch; every pointer is a device pointer (host pointers in the host form); the grids share one mi_stride.
 *   d_lf_mi, d_mc_mi   sb_type and is_inter; mv_row / mv_col of ref 0 / 1 (every unit of a block carries them; not read for an intra unit)
 *   d_ext       ref_frame of every unit, mode at leaf origins; the other fields are not read
 *   d_ext_out   WRITTEN (unless NULL), one complete record per unit of the picture: ref_frame as in d_ext; at a leaf's origin its mode;
 *               at an inter leaf's origin ref_mv_row / ref_mv_col[k] = the first candidate of ref_frame[k] and mode_context; every
 *               other field 0.  Must not alias d_ext
 *   d_cand      WRITTEN (unless NULL), one record per unit: at the origin of a leaf of 8x8 or larger, intra leaves included as in the
 *               reference, both candidates and the return value of every reference frame of ref_mask (an entry the reference does
 *               not find is 0) and the mode context; at every other unit 0 with the three counts 0xFF
 *   d_status    WRITTEN always: {inter leaves whose coded MVs contradict their mode -- NEARESTMV with an MV that is not the first
 *               candidate of its reference, NEARMV not the second, ZEROMV not zero --, inter leaves}; both SVT_MODES_BAD_GRID for a grid
 *               this entry does not take: a rectangular sb_type, a block that crosses the picture edge or overlaps another, a
 *               reference frame above 3, is_inter, d_mc_mi's ref_list and ref_frame disagreeing about inter or compound, an inter block
 *               below 8x8, an inter mode outside 10 .. 13.  d_ext_out and d_cand are then unspecified
 *   ref_mask    bits 1 .. 3: the reference frames of d_cand
 *   restrict_ref_mvs   cm->use_prev_frame_mvs: same-reference candidates only, at most one is returned unless two are found */
typedef struct svt_mvrefs_picture {
    const svt_lf_mode_info *d_lf_mi;
    const svt_mc_mode_info *d_mc_mi;
    const svt_mi_inter_ext *d_ext;
    svt_mi_inter_ext       *d_ext_out;
    svt_mvref_cand         *d_cand;
    uint32_t               *d_status;
    uint8_t                 ref_mask;
    uint8_t                 restrict_ref_mvs;
    uint8_t                 ref_frame_sign_bias[4];
    uint8_t                 pad_[2];
} svt_mvrefs_picture;                       /* 56 bytes */
/* n_pics (<= 32) pictures of one geometry (multiples of 8, 8 .. 8192, mi_stride >= width / 8) in one call; their parameters may
 * differ.  Asynchronous on the context's stream, no synchronisation.  Refused: a null required pointer, n_pics outside 1 .. 32, ref_mask
 * with bit 0 or bits 4 .. 7 set, d_ext_out == d_ext. */
int32_t svt_hip_mvrefs_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_mvrefs_picture *pics, int32_t width, int32_t height, int32_t mi_stride);
/* host form of the same text (csrc/mvrefs_core.h), pure CPU, host pointers */
int32_t svt_hip_mvrefs_picture(const svt_mvrefs_picture *pic, int32_t width, int32_t height, int32_t mi_stride);

/* ------------------------------------------------------------------------------------------------------------------
 * Inter mode labelling: the two grids the encode pass holds -> complete svt_mi_inter_ext records, the producer the two entries above
 * lacked.  ref_frame of every unit follows from the prediction grid's ref_list; the inter mode of every leaf is chosen so that it
 * agrees with the leaf's MVs -- NEARESTMV if every reference's MV is the first candidate eb_vp9_find_mv_refs derives (and one was
 * found), else NEARMV if it is the second (and two were found), else ZEROMV if every MV is zero, else NEWMV -- in that fixed order,
 * not by rate (csrc/md_inter_core.h says why); mode_context and ref_mv_* are then derived from the labelled grid exactly as
 * svt_hip_mvrefs_batch_device derives them, which by construction counts no contradiction in these records.  Chain: encode pass ->
 * tokeniser -> this -> inter mode info -> bool coder -> frame on one context's stream, no host round trip: d_ext_out is the d_ext of
 * svt_hip_modes_inter_batch_device.
 *
 * one picture of a batch; every pointer is a device pointer (host pointers in the host form); the grids share one mi_stride.
 *   d_lf_mi, d_mc_mi   sb_type and is_inter; ref_list and mv_row / mv_col of ref 0 / 1 (not read for an intra unit)
 *   d_ext_out   WRITTEN, one complete record per unit of the picture, in svt_hip_mvrefs_batch_device's format: ref_frame at every unit
 *               ({0, 0} at an intra one); at an inter leaf's origin mode, ref_mv_row / ref_mv_col[k] and mode_context; every other
 *               field 0
 *   d_cand      WRITTEN (unless NULL) as svt_hip_mvrefs_batch_device writes it, for the reference frames of ref_mask
 *   d_status    WRITTEN always, four words: {inter leaves, leaves labelled NEWMV, NEWMV leaves pack_inter_mode_mvs cannot code
 *               faithfully -- a difference to ref_mv[k] beyond +-16383 in a component, or an odd one where the high-precision bit is
 *               not coded (!(allow_hp && use_mv_hp(ref_mv[k]))): counted, not altered; a picture with a non-zero count must not be
 *               shipped --, 0}; all four SVT_MODES_BAD_GRID for a grid this entry does not take: whatever svt_hip_mvrefs_batch_device
 *               refuses, a ref_list above 1, list_ref_frame outside 1 .. 3, a compound leaf under SINGLE_REFERENCE (a single one
 *               under COMPOUND_REFERENCE) or one whose references are not comp_fixed_ref plus one of comp_var_ref.  d_ext_out and
 *               d_cand are then unspecified
 *   list_ref_frame     the reference frame (1 .. 3) REF_LIST_0 / REF_LIST_1 stand for in this picture
 *   the other parameters mean what they mean in svt_mvrefs_picture and svt_modes_inter_picture */
typedef struct svt_md_inter_picture {
    const svt_lf_mode_info *d_lf_mi;
    const svt_mc_mode_info *d_mc_mi;
    svt_mi_inter_ext       *d_ext_out;
    svt_mvref_cand         *d_cand;
    uint32_t               *d_status;
    uint8_t                 list_ref_frame[2];
    uint8_t                 ref_frame_sign_bias[4];
    uint8_t                 restrict_ref_mvs, allow_hp, reference_mode, comp_fixed_ref, comp_var_ref[2];
    uint8_t                 ref_mask;
    uint8_t                 pad_[3];
} svt_md_inter_picture;                     /* 56 bytes */
/* n_pics (<= 32) pictures of one geometry (multiples of 8, 8 .. 8192, mi_stride >= width / 8) in one call; their parameters may
 * differ.  Asynchronous on the context's stream, no synchronisation; scratch (12 bytes per unit of the batch) is taken from the context
 * at the first call of a geometry.  Refused, nothing launched: a null required pointer, n_pics outside 1 .. 32, ref_mask with bit 0 or
 * bits 4 .. 7 set, reference_mode above 2 or -- unless it is SINGLE_REFERENCE -- a compound reference outside 1 .. 3. */
int32_t svt_hip_md_inter_modes_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_md_inter_picture *pics, int32_t width, int32_t height,
                                            int32_t mi_stride);
/* host form of the same text (csrc/md_inter_core.h), pure CPU, host pointers */
int32_t svt_hip_md_inter_modes_picture(const svt_md_inter_picture *pic, int32_t width, int32_t height, int32_t mi_stride);

/* ------------------------------------------------------------------------------------------------------------------
 * Picture-level EncDec: everything the encode pass does with mode decision's output, whole pictures at a time, device resident.
 *
 * Replaces, per batch of mutually independent pictures (e.g. the pictures of one temporal layer of a mini-GOP), the data path of
 * eb_vp9_enc_dec_kernel behind mode decision (Codec/EbEncDecProcess.c:5306): encode_pass_sb (:3627-4241) = inter prediction
 * (:3787-3802) -> perform_coding_loop per transform block (:3830, 3890, 3940) -> skip flags (:4069-4098) -> and, once per picture,
 * eb_vp9_build_mask_frame + eb_vp9_loop_filter_frame (:5651-5686) -> pad_ref_and_set_flags (:5694-5697).  The input is the mode-info
 * grid (what mode decision leaves in picture_control_set_ptr->mode_info_array), not block lists: the transform-block descriptors,
 * the skip flags and the LOOP_FILTER_MASKs are derived ON THE DEVICE (svt_tq_count / _emit, svt_tq_skip, svt_lf_mask kernels --
 * the same rules as svt_hip_tq_blocks_from_grid and svt_hip_lf_build_masks, one text: csrc/encdec_core.h), so no per-picture
 * descriptor data crosses PCIe and nothing waits for the host between the stages.
 * ------------------------------------------------------------------------------------------------------------------ */

/* Where the planes of one picture of a batch live relative to the batch's base pointers, and where its outputs go.  Offsets are
 * bytes from the batch's source / prediction base pointer (one 32-bit offset space each) and from the picture's own
 * reconstruction buffer; plane order Y, Cb, Cr. */
typedef struct svt_tq_pic_geom {
    uint32_t src_off[3], pred_off[3], recon_off[3];
    uint16_t src_stride[2], pred_stride[2], recon_stride[2]; /* luma, chroma */
    uint32_t coeff_base;    /* element offset of the picture's coefficient area (n_sb * SVT_SB_COEFFS elements) in the batch's arrays */
    int32_t  width, height; /* luma samples (multiples of 8) */
    uint8_t  recon_set;     /* which reconstruction base pointer of the batch (0..7): recon_off is relative to it */
    uint8_t  do_recon;
    uint8_t  pic;           /* index of the picture in its batch (0..63): goes into the position code */
    uint8_t  pad_[1];
} svt_tq_pic_geom;
/* Coefficient layout of the driver: per SB 64*64 luma + 2 x 32*32 chroma coefficients (Y at +0, Cb at +4096, Cr at +5120), every
 * block's N*N coefficients contiguous (raster inside the block) as in the reference's per-SB quantized_coeff_buffer
 * (Codec/EbEncDecProcess.c:4100-4108), but addressed by POSITION: inside a plane area the 4x4 units are in z-order, so the block at
 * sample (x, y) of its plane starts at zorder((x % S) / 4, (y % S) / 4) * 16 with S = 64 (luma) / 32 (chroma). */
#define SVT_SB_COEFFS 6144

/* host: the transform blocks of n_pics pictures (one geometry) from their mode-info grids, grouped by transform size and inside a
 * size ordered picture, SB (raster), 8x8 unit of the SB (raster), and per unit luma, Cb, Cr -- exactly the lists the driver builds
 * on the device.  The luma transform type of a block travels in svt_lf_mode_info.pad_[0] (0 = DCT_DCT).  pos[i] = picture-in-batch
 * << 24 | plane << 22 | (y / 4) << 11 | (x / 4) of block i, x / y in samples of its plane.  Returns the number of blocks or a negative error. */
int32_t svt_hip_tq_blocks_from_grid(int32_t n_pics, const svt_lf_mode_info *const *lf_mi, int32_t mi_stride, const svt_tq_pic_geom *geom,
                                    svt_tq_block *blocks, uint32_t *pos, int32_t capacity, int32_t size_count[4]);

/* host: the normative VP9 tables the transform stage needs (generated from the reference's own objects, tools/gen_vp9_tables.py):
 * the inverse scan orders eb_vp9_scan_orders[tx_size][tx_type].iscan (VPX/vp9_scan.c) concatenated, offsets16[tx_size * 4 +
 * tx_type] = element offset of a table; the quantiser steps eb_vp9_dc_quant / eb_vp9_ac_quant(q_index, 0, 8 bit)
 * (VPX/vp9_quant_common.c); eb_vp9_quantizer_to_qindex (VPX/vp9_quantize.c:329). */
const int16_t *svt_hip_vp9_iscan_tables(const uint32_t **offsets16, int32_t *entries);
int32_t svt_hip_vp9_qindex_from_qp(int32_t qp);
/* The q index a picture is coded at in fixed-QP mode: the sequence QP scaled by the picture's temporal layer -- QP_SCALING_MODE_0 of
 * eb_vp9_rate_control_kernel (Codec/EbRateControlProcess.c:4680-4722: eb_vp9_compute_qdelta with delta_rate_oq / _sq / _vmaf).  tune:
 * 0 SQ, 1 OQ, 2 VMAF; hierarchical_levels 3 or 4.  is_key: the sequence q index itself (key frames take the reference's adaptive
 * QP_SCALING_MODE_1, which is rate control proper and not part of this path). */
int32_t svt_hip_vp9_layer_qindex(int32_t qp, int32_t tune, int32_t hierarchical_levels, int32_t temporal_layer_index, int32_t is_key);
int32_t svt_hip_vp9_dc_step(int32_t q_index);
int32_t svt_hip_vp9_ac_step(int32_t q_index);
/* out[0] luma, out[1] chroma tables of a q index with zero deltas (the sequence-level eb_vp9_init_quantizer) */
int32_t svt_hip_quant_tables_for_qindex(int32_t q_index, svt_quant_tables out[2]);

/* Which stages the reference runs behind mode decision for a picture: the flags eb_vp9_signal_derivation_enc_dec_kernel_{sq,oq,
 * vmaf} derive (limit_intra, Codec/EbEncDecProcess.c:4989-4997 / 5127-5136 / 5257-5263; allow_enc_dec_mismatch, :4954-4959 /
 * 5084-5089 / 5201) and what encode_pass_sb (:3653-3657) and the picture's last SB (:5633-5697) do with them. */
typedef struct svt_encdec_flags_config {
    int32_t enc_mode, tune;
    int32_t temporal_layer_index;
    int32_t is_used_as_reference;
    int32_t recon_file;            /* static_config.recon_file */
    int32_t loop_filter;           /* static_config.loop_filter */
} svt_encdec_flags_config;
typedef struct svt_encdec_flags {
    int32_t limit_intra, allow_enc_dec_mismatch;
    int32_t do_recon;              /* inter SBs are reconstructed (inverse transform + add) */
    int32_t apply_loop_filter;     /* lf_application_enable_flag */
    int32_t pad_reference;         /* pad_ref_and_set_flags runs */
} svt_encdec_flags;
int32_t svt_hip_encdec_flags_derive(const svt_encdec_flags_config *cfg, svt_encdec_flags *flags);

/* One picture of a batch.  Every pointer is a device pointer.  The grids are [mi_rows][mi_stride] records per 8x8 unit. */
typedef struct svt_encdec_picture {
    const svt_mc_mode_info *d_mc_mi;   /* inter part of the mode info (prediction) */
    svt_lf_mode_info       *d_lf_mi;   /* sb_type, tx_size, is_inter, filter_level (+ luma tx_type in pad_[0]); `skip` is WRITTEN */
    svt_yuv_planes          src;       /* source picture, sample (0,0) pointers */
    svt_yuv_planes          ref[2];    /* padded reference pictures (as svt_mc_picture.ref) */
    svt_yuv_planes          pred;      /* prediction picture (written by the inter prediction, read by the transform stage) */
    svt_yuv_planes          recon;     /* the picture's reconstruction = reference buffer (sample (0,0) pointers into padded planes) */
    int16_t                *d_qcoeff, *d_dqcoeff; /* n_sb * SVT_SB_COEFFS each, 16-byte aligned, position-addressed (above).  d_dqcoeff may be
                                                      NULL (for every picture of a call or for none): the encode pass consumes the dequantised
                                                      coefficients in the lane that produced them (inverse transform) and nothing downstream
                                                      reads them -- they then never travel to memory (3 bytes per sample less traffic) */
    uint16_t               *d_eob_map; /* eob of every transform block at its 4x4 unit: [Y: (H/4) x (W/4)] [Cb: (H/8) x (W/8)] [Cr] */
    svt_lf_mask            *d_lfm;     /* [sb_rows][sb_cols] masks (written; read by the loop filter) */
    uint8_t                *d_nz;      /* scratch, mi_rows * mi_stride bytes */
    int32_t                 use_subpel; /* svt_mc_picture.use_subpel */
    int32_t                 no_pad;    /* 1: this picture is not padded although the batch's flags say pad_reference (a picture that is not
                                          used as a reference riding in a batch of reference pictures) */
    int32_t                 has_intra; /* 1: the grid holds intra blocks (is_inter = 0; sizes / modes as for svt_hip_encdec_intra_device): they are
                                          coded by the intra pass behind the batch's transform stage, from their neighbours' reconstruction
                                          (needs the flags' do_recon).  0: every block is inter; an intra block would be left uncoded */
    int32_t                 pad_;
} svt_encdec_picture;

/* workspace of a batch: descriptor lists, per-list eob, counters (device memory owned by the object); sized for max_pics pictures
 * of width x height.  Calls that share a workspace must be issued on the same context (stream order protects it). */
typedef struct svt_encdec_work svt_encdec_work;
int32_t svt_hip_encdec_work_create(svt_hip_ctx *ctx, int32_t max_pics, int32_t width, int32_t height, svt_encdec_work **work);
void    svt_hip_encdec_work_destroy(svt_hip_ctx *ctx, svt_encdec_work *work);

/* n_pics (<= 32, <= the workspace's max_pics) pictures of one geometry and one set of flags (the pictures of a temporal layer, or
 * of several layers of different mini-GOPs that share their flags; the reconstruction buffers of a batch must fall into at most 8
 * regions of 4 GB -- e.g. be carved out of a few slabs):
 * inter prediction -> transform blocks from the grids -> residual / transform / quantisation (/ reconstruction when
 * flags->do_recon) with the tables of q_index -> skip flags + eob map -> (flags->apply_loop_filter: masks + deblocking with
 * filter_level's thresholds) -> (flags->pad_reference: border of pad_x / pad_y samples).  Source and prediction planes of the
 * batch must each lie within 4 GB of the lowest of them (32-bit block offsets).  Asynchronous on the context's stream.
 * A malformed grid (block crossing the picture edge, transform larger than its block ...) is reported by
 * svt_hip_encdec_work_status after the work has completed; its blocks are left out. */
int32_t svt_hip_encdec_batch_device(svt_hip_ctx *ctx, svt_encdec_work *work, int32_t n_pics, const svt_encdec_picture *pics, int32_t width,
                                    int32_t height, int32_t mi_stride, int32_t q_index, const svt_encdec_flags *flags,
                                    const svt_lf_thresh *thr, int32_t pad_x, int32_t pad_y);
/* The decode pass: n_pics INTER pictures rebuilt from their coefficients and mode info -- what a decoder does with a parsed frame, on
 * the workspace and picture records of svt_hip_encdec_batch_device.  Of a picture, src and d_dqcoeff are ignored; d_mc_mi, d_lf_mi
 * (with `skip`), d_qcoeff (zero wherever nothing was coded) and d_eob_map are INPUTS; pred, recon, d_lfm and the grid's `skip` are
 * written (d_nz is scratch).  Stages, asynchronous on the context's stream with no host round trip: inter prediction -> transform
 * blocks from the grids -> svt_hip_recon_batch_device's arithmetic over them, each block's eob read from the eob map -> skip flags
 * as a decoder derives them for the loop filter (an inter leaf of 8x8 or larger whose eobs are all zero is skipped) -> thr != NULL
 * (the header's filter level is not 0): masks + deblocking -> border of pad_x / pad_y samples for every picture without no_pad.
 * For the grids, coefficients and eob maps an encode pass left (do_recon, and apply_loop_filter / pad_reference as here) the planes, the
 * masks and the skip flags equal that pass's byte for byte.
 * d_status (device, required): d_status[0] = the number of coefficients whose dequantised value overflowed 16 bits (0 for a
 * conformant stream).  A picture with has_intra is refused (SVT_HIP_ERR_UNSUPPORTED) before anything is launched -- this entry is the
 * pass for batches known to hold inter leaves only; svt_hip_decode_mixed_batch_device below takes the others.  A grid that holds an
 * is_inter = 0 leaf all the same, or is malformed, is reported by svt_hip_encdec_work_status, its blocks left out. */
int32_t svt_hip_decode_batch_device(svt_hip_ctx *ctx, svt_encdec_work *work, int32_t n_pics, const svt_encdec_picture *pics, int32_t width,
                                    int32_t height, int32_t mi_stride, int32_t q_index, const svt_lf_thresh *thr, int32_t pad_x, int32_t pad_y,
                                    int32_t *d_status);
/* The same pass for batches whose pictures may carry has_intra (inter pictures with intra leaves): same arguments, stages and outputs.
 * Behind the reconstruction of the inter leaves and in front of the skip flags, the intra leaves of every picture with has_intra are
 * predicted and reconstructed from their coefficients by the wavefront kernel of svt_hip_decode_intra_device, one picture after the other
 * -- the place and order of svt_hip_encdec_batch_device's intra step.  Planes and strides of a picture with has_intra must be 4-byte
 * aligned.  An is_inter = 0 leaf in a picture whose has_intra is 0 is still reported by svt_hip_encdec_work_status; d_status[0] counts
 * the overflowed coefficients of inter and intra blocks together. */
int32_t svt_hip_decode_mixed_batch_device(svt_hip_ctx *ctx, svt_encdec_work *work, int32_t n_pics, const svt_encdec_picture *pics, int32_t width,
                                          int32_t height, int32_t mi_stride, int32_t q_index, const svt_lf_thresh *thr, int32_t pad_x, int32_t pad_y,
                                          int32_t *d_status);
/* The decode pass of an INTRA picture (key frames, intra-refresh pictures): the decode twin of svt_hip_encdec_intra_device below, on the
 * same grid format.  INPUTS: pic->d_lf_mi, d_qcoeff (zero wherever nothing was coded), d_eob_map; src, d_dqcoeff, d_mc_mi and ref are not
 * looked at.  WRITTEN: pred (may be all NULL: the prediction is then not stored), recon, the grid's `skip`, d_nz, d_lfm.  Stages,
 * asynchronous on the context's stream: d_status[0] cleared -> reference samples + predictor + dequantisation / inverse transform /
 * reconstruction of every block in the encode pass's dependency order (each block's eob read from the eob map; eob 0: the prediction is the
 * reconstruction) -> skip flags (a block with no coefficient in any of its transform blocks is skipped) -> thr != NULL: masks +
 * deblocking -> border of pad_x / pad_y samples unless pic->no_pad.  For the grid, coefficients and eob map an encode pass left, the planes,
 * masks and skip flags equal that pass's byte for byte.  The above-right rule is the encode pass's (none for blocks >= 8x8).
 * d_status (device, required): d_status[0] = coefficients whose dequantised value overflowed 16 bits.  A malformed grid (a 64x64 or
 * rectangular block, an inter leaf ...) is reported by svt_hip_encdec_work_status; the pass terminates whatever the grid and the
 * coefficient arrays hold.  d_qcoeff 16-byte aligned; planes and strides 4-byte aligned. */
int32_t svt_hip_decode_intra_device(svt_hip_ctx *ctx, svt_encdec_work *work, const svt_encdec_picture *pic, int32_t width, int32_t height,
                                    int32_t mi_stride, int32_t q_index, const svt_lf_thresh *thr, int32_t pad_x, int32_t pad_y, int32_t *d_status);
/* The encode pass of an INTRA picture (key frames, intra-refresh pictures): reference samples + the ten VP9 intra predictors +
 * transform / quantisation / reconstruction of every block in coding-dependency order (encode_pass_sb with intra blocks,
 * Codec/EbEncDecProcess.c:3680-4160: generate_intra_reference_samples :1128, intra_prediction Codec/EbIntraPrediction.c:16 ->
 * VPX/vp9_reconintra.c:249-408 / VPX/intrapred.c, perform_coding_loop :365), then the tail of svt_hip_encdec_batch_device: skip flags,
 * loop-filter masks, deblocking, border.  The grid (pic->d_lf_mi) describes intra blocks of 8x8, 16x16 or 32x32 (sb_type 3 / 6 / 9)
 * with the transform of their own size, is_inter = 0, pad_[1] = luma mode, pad_[2] = chroma mode (PREDICTION_MODE: 0 DC, 1 V, 2 H,
 * 3 D45, 4 D135, 5 D117, 6 D153, 7 D207, 8 D63, 9 TM); the luma transform type follows the mode
 * (eb_vp9_intra_mode_to_tx_type_lookup).  sb_type 0 = an 8x8 unit of four 4x4 luma blocks (+ one 4x4 chroma block per plane): tx_size 0,
 * the luma modes of blocks 0..3 in the nibbles of pad_[1] (blocks 0, 1) and pad_[0] (blocks 2, 3), pad_[2] the chroma mode.  The 64x64
 * block and rectangular blocks are outside this entry (reported as malformed through svt_hip_encdec_work_status).  pic->ref / d_mc_mi are ignored; pic->pred may be all NULL (the prediction is then not stored).
 * flags->do_recon must be set.  Planes and strides 4-byte aligned.  Asynchronous on the context's stream. */
int32_t svt_hip_encdec_intra_device(svt_hip_ctx *ctx, svt_encdec_work *work, const svt_encdec_picture *pic, int32_t width, int32_t height,
                                    int32_t mi_stride, int32_t q_index, const svt_encdec_flags *flags, const svt_lf_thresh *thr, int32_t pad_x,
                                    int32_t pad_y);
/* Stand-in decision for an intra picture (NOT the reference's): 16x16 blocks with DC prediction, 8x8 where a 16x16 block would
 * cross the picture edge. */
int32_t svt_hip_md_intra_default_device(svt_hip_ctx *ctx, int32_t width, int32_t height, int32_t filter_level, svt_lf_mode_info *d_lf_mi, int32_t mi_stride);
/* Open-loop intra search (OIS): the per-block, per-mode cost of every VP9 intra predictor, computed from the SOURCE samples (no
 * reconstruction, so no dependency chain: the whole picture runs in parallel).  NOT the reference's mode decision; like the ME
 * results, the records are the kind of input a host's mode decision consumes.
 * For every square block of N in {4, 8, 16, 32} that lies wholly inside the picture and each of the ten modes, the prediction is
 * built from the source with the rules of the intra encode pass (svt_hip_encdec_intra_device): left column 129 at x = 0, above row
 * 127 at y = 0, corner 129 with an above row but no left column (127 at y = 0), no above-right samples for N >= 8 (the above row is
 * replicated), a 4x4 block in the left half of its 8x8 unit reads the four true above-right samples.  sad = luma SAD of the best mode,
 * ties to the lowest mode index.  For N >= 8 the chroma block (N / 2, both planes) is searched the same way: uv_mode = argmin of
 * SAD_Cb + SAD_Cr, uv_sad = that sum.  Blocks that cross the right or bottom edge (and the parts of an incomplete SB outside the
 * picture) get sad = uv_sad = UINT32_MAX, mode = uv_mode = 0xFF. */
typedef struct svt_ois_block {   /* 12 bytes */
    uint32_t sad;      /* luma SAD of the best mode; UINT32_MAX: block not inside the picture */
    uint32_t uv_sad;   /* Cb SAD + Cr SAD of the best chroma mode (blocks >= 8x8; UINT32_MAX for 4x4 records) */
    uint8_t  mode, uv_mode;  /* PREDICTION_MODE 0 DC .. 9 TM; 0xFF where the SAD is UINT32_MAX */
    uint8_t  pad_[2];
} svt_ois_block;
#define SVT_OIS_PER_SB 340  /* 4 x 32x32, 16 x 16x16, 64 x 8x8, 256 x 4x4, each group in z-order inside the SB */
/* d_out: n_sb * SVT_OIS_PER_SB records, SB raster order (device memory).  src: device planes (luma stride >= width, chroma stride >=
 * width / 2).  Width and height multiples of 8.  Asynchronous on the context's stream. */
int32_t svt_hip_intra_search_device(svt_hip_ctx *ctx, const svt_yuv_planes *src, int32_t width, int32_t height, svt_ois_block *d_out);
/* The same for n_pics pictures of one geometry in one launch (srcs, d_out: host arrays of n_pics entries holding device pointers).  With
 * with_4x4 = 1 every picture's records equal svt_hip_intra_search_device's.  with_4x4 = 0 leaves the 256 luma 4x4 blocks of an SB out:
 * records 0 .. 83 are the same, records 84 .. 339 are written as "none" (sad = uv_sad = UINT32_MAX, mode = uv_mode = 0xFF).  A null plane
 * or output, a stride below the width, a misaligned output or with_4x4 outside {0, 1}: SVT_HIP_ERR_BAD_PARAMETER, nothing launched. */
int32_t svt_hip_intra_search_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_yuv_planes *srcs, int32_t width, int32_t height, int32_t with_4x4,
                                          svt_ois_block *const *d_out);
/* Stand-in intra decision from the OIS records (NOT the reference's mode decision): cost of a coded block J = D + lambda, D = sad +
 * uv_sad for blocks >= 8x8, and for a unit of four 4x4 blocks (sb_type 0) the sum of the four 4x4 sad + the 8x8 record's uv_sad.
 * Bottom-up: 8x8 against its four 4x4 blocks, 16x16 against its four best 8x8 subtrees, 32x32 against its four best 16x16 subtrees;
 * a parent replaces its children when J_parent <= sum J_children (ties to the larger block), never when its record is UINT32_MAX or
 * it crosses the picture edge; compared in 64 bits.  No 64x64 (the intra pass does not take it).  Writes the grid of
 * svt_hip_encdec_intra_device: sb_type 0 / 3 / 6 / 9, tx_size of the block's size, is_inter = skip = 0, luma modes in pad_[1]
 * (nibbles of pad_[1] / pad_[0] for sb_type 0), chroma mode in pad_[2], filter_level as given.  d_ois: the records of
 * svt_hip_intra_search_device.  svt_hip_md_intra_search_picture is the host form (same text, csrc/encdec_core.h). */
int32_t svt_hip_md_intra_search_device(svt_hip_ctx *ctx, const svt_ois_block *d_ois, int32_t width, int32_t height, uint32_t lambda,
                                       int32_t filter_level, svt_lf_mode_info *d_lf_mi, int32_t mi_stride);
int32_t svt_hip_md_intra_search_picture(const svt_ois_block *ois, int32_t width, int32_t height, uint32_t lambda, int32_t filter_level,
                                        svt_lf_mode_info *lf_mi, int32_t mi_stride);
/* Profiling aid: `hook` is called on the enqueueing thread at every stage boundary of svt_hip_encdec_batch_device (before the
 * stage named is enqueued; SVT_ENCDEC_STAGE_END after the last), so that a host can record events of its own on the context's stream
 * and attribute the chain's time to its stages.  NULL removes it. */
#define SVT_ENCDEC_STAGE_MC 0
#define SVT_ENCDEC_STAGE_LISTS 1
#define SVT_ENCDEC_STAGE_TQ 2
#define SVT_ENCDEC_STAGE_SKIP 3
#define SVT_ENCDEC_STAGE_LF 4
#define SVT_ENCDEC_STAGE_PAD 5
#define SVT_ENCDEC_STAGE_END 6
typedef void (*svt_encdec_stage_hook)(void *user, int32_t stage);
void svt_hip_encdec_work_set_stage_hook(svt_encdec_work *work, svt_encdec_stage_hook hook, void *user);
/* synchronises the context; 0 = every grid the workspace has seen was well-formed, else SVT_HIP_ERR_BAD_PARAMETER (and the flag is
 * cleared).  counts[8] (optional) = offset and number of blocks per transform size of the most recent batch. */
int32_t svt_hip_encdec_work_status(svt_hip_ctx *ctx, svt_encdec_work *work, int32_t counts[8]);
/* most recent batch: copies the descriptor list, the position codes and the per-list eob to the host (capacity in blocks);
 * returns the number of blocks.  For tests and for hosts that walk the coefficients in list order. */
int32_t svt_hip_encdec_work_download(svt_hip_ctx *ctx, svt_encdec_work *work, svt_tq_block *blocks, uint32_t *pos, uint16_t *eob, int32_t capacity);

/* Stand-in for mode decision (NOT the reference's: mode decision is host control logic outside this path).  Turns the ME results
 * of n_pics pictures into well-formed mode-info grids so that the stages behind mode decision can run without a host-supplied
 * decision: bottom-up merge over the PU tree (16x16 -> 32x32 -> 64x64: a parent replaces its four children when
 * distortion(parent) <= sum distortion(children) + 3 lambda), blocks split at the picture edge down to 8x8, every block inter with
 * the direction / vectors of its own PU's best ME candidate and the transform of its own size (32x32 for 64x64).  d_results[i],
 * d_mc_mi[i], d_lf_mi[i] device arrays of picture i.  svt_hip_md_default_picture is the host form (same text). */
int32_t svt_hip_md_default_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_me_pu_result *const *d_results, int32_t width, int32_t height,
                                        uint32_t lambda, int32_t filter_level, svt_mc_mode_info *const *d_mc_mi, svt_lf_mode_info *const *d_lf_mi,
                                        int32_t mi_stride);
int32_t svt_hip_md_default_picture(const svt_me_pu_result *results, int32_t pic_width, int32_t pic_height, uint32_t lambda, int32_t filter_level,
                                   svt_mc_mode_info *mc_mi, svt_lf_mode_info *lf_mi, int32_t mi_stride);

/* Mixed stand-in for mode decision of an inter picture (NOT the reference's either; deterministic, no claim of coding efficiency): the
 * partition of svt_hip_md_default_batch_device with an intra alternative per PU, from the ME records and the records of the open-loop
 * intra search of the same picture.  PU p of an SB: 0 the 64x64, 1..4 the 32x32, 5..20 the 16x16, 21..84 the 8x8 blocks, each group in
 * z-order -- the order of the OIS groups too, so the OIS record of PU p >= 1 is record p - 1 of the SB.
 *      inter(p) = results[p].distortion_direction[0].distortion
 *      intra(p) = ois[p - 1].sad + intra_penalty (64 bits); none where the record's sad is UINT32_MAX, and for the 64x64 PU
 *      cost(p)  = min(inter(p), intra(p))
 * Only luma SADs are compared (ME's distortion is luma only; uv_sad takes no part).  The bottom-up merge is the default stand-in's with
 * cost(p) in place of the ME distortion (parent when cost(parent) <= sum cost(children) + 3 lambda; split at the picture edge down to
 * 8x8).  A leaf is intra iff intra(p) < inter(p): ties go to inter.  No unit of four 4x4 blocks is produced; records 84 .. 339 of an SB are
 * not read, so the batched search may leave its 4x4 phase out.  An inter leaf is written as the default stand-in writes it.  An intra
 * leaf: sb_type 3 / 6 / 9, tx_size 1 / 2 / 3, is_inter = skip = 0, pad_[0] = 0, pad_[1] / pad_[2] = the record's mode / uv_mode; in the
 * prediction grid bw8 = bh8 = its size, ref_list = {-1, -1}, vectors 0.  With intra_penalty >= 1 << 24 (a 64x64 SAD is at most
 * 64 * 64 * 255) no leaf of real ME records is intra and both grids equal the default stand-in's byte for byte.
 * d_intra_units[i] (n_pics counters in device memory) = number of 8x8 units of picture i written with is_inter = 0; the entry zeroes them
 * on the stream first.  A caller derives svt_encdec_picture.has_intra from it.  Pictures are host records of device pointers; d_results
 * and d_ois 4-byte aligned.  A null field, a misaligned pointer or a bad size: SVT_HIP_ERR_BAD_PARAMETER, nothing launched or written.
 * svt_hip_md_mixed_picture is the host form (same text, csrc/encdec_core.h); *intra_units receives the count. */
typedef struct svt_md_mixed_picture {
    const svt_me_pu_result *d_results;  /* n_sb * 85 */
    const svt_ois_block    *d_ois;      /* n_sb * SVT_OIS_PER_SB */
    svt_mc_mode_info       *d_mc_mi;
    svt_lf_mode_info       *d_lf_mi;
} svt_md_mixed_picture;
int32_t svt_hip_md_mixed_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_md_mixed_picture *pics, int32_t width, int32_t height, uint32_t lambda,
                                      uint32_t intra_penalty, int32_t filter_level, int32_t mi_stride, int32_t *d_intra_units);
int32_t svt_hip_md_mixed_picture(const svt_me_pu_result *results, const svt_ois_block *ois, int32_t pic_width, int32_t pic_height, uint32_t lambda,
                                 uint32_t intra_penalty, int32_t filter_level, svt_mc_mode_info *mc_mi, svt_lf_mode_info *lf_mi, int32_t mi_stride,
                                 int32_t *intra_units);

/* device form of svt_hip_lf_build_masks (same text): masks of n_pics pictures from device-resident grids */
int32_t svt_hip_lf_build_masks_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_lf_mode_info *const *d_lf_mi, int32_t mi_stride, int32_t mi_rows,
                                      int32_t mi_cols, svt_lf_mask *const *d_lfm);

/* Makes everything enqueued LATER on `ctx` wait for marker `marker` of `other` (both on the same device or not): the
 * stream-to-stream dependency a pipeline of contexts needs (ME one mini-GOP ahead of EncDec) without a host wait. */
int32_t svt_hip_ctx_wait_marker(svt_hip_ctx *ctx, svt_hip_ctx *other, uint64_t marker);
/* asynchronous device-to-host copy into PINNED host memory (svt_hip_host_alloc), ordered on the context's stream; completion is
 * observed through a marker recorded after it */
int32_t svt_hip_host_alloc(svt_hip_ctx *ctx, size_t bytes, void **ptr);
void    svt_hip_host_free(svt_hip_ctx *ctx, void *ptr);
int32_t svt_hip_mem_download_2d_async(svt_hip_ctx *ctx, void *pinned_dst, size_t dst_stride, const void *d_src, size_t src_stride, size_t width_bytes,
                                      size_t rows);
/* device-to-device rectangle copy on the context's stream */
int32_t svt_hip_mem_copy_2d_device(svt_hip_ctx *ctx, void *d_dst, size_t dst_stride, const void *d_src, size_t src_stride, size_t width_bytes,
                                   size_t rows);

/* ------------------------------------------------------------------------------------------------ */
/* Multi-GPU: GOP sharding and the inter-segment reference hand-off (scope row e)                      */
/* ------------------------------------------------------------------------------------------------ */
/* Closed GOPs are independent units of the reference (every intra refresh is a key frame, Codec/EbPictureDecisionProcess.c:952,
 * 1596-1603): GOP g is encoded by device g % n_devices and the data path needs no exchange.  svt_hip_gop_assign writes the
 * GOPs of device `index` (ascending) into gops[] (capacity max) and returns how many there are; svt_hip_gop_owner is g % n. */
int32_t svt_hip_gop_owner(int64_t gop, int32_t n_devices);
int32_t svt_hip_gop_assign(int64_t n_gops, int32_t n_devices, int32_t index, int64_t *gops, int32_t max);
/* Split-GOP (low-latency) mode: consecutive mini-GOPs of ONE GOP go to consecutive devices; mini-GOP m is encoded by device
 * m % n_devices and needs the reconstructed, deblocked, padded base-layer picture of mini-GOP m - 1 from device (m - 1) %
 * n_devices first -- the one exchange step of the path (a point-to-point copy over one xGMI link, ~13.9 MB at 4K).
 * Returns the device that produces the reference mini-GOP m needs, or -1 for m = 0 (it starts from the key frame). */
int32_t svt_hip_minigop_reference_source(int64_t minigop, int32_t n_devices);

/* How the reference cuts the pictures waiting in its pre-assignment buffer when they are released short of a full mini-GOP (end of
 * stream, or an intra refresh arrived) into the units it assigns prediction structures to: eb_vp9_generate_picture_window_split +
 * eb_vp9_handle_incomplete_picture_window_map as the picture-decision kernel drives them (Codec/EbPictureDecisionProcess.c:387-476,
 * 1662-1680; mini-GOP table Codec/EbUtility.c:167-185).  A full group (n_pictures == 1 << hierarchical_levels) is one part.
 * cut_by_intra != 0: the group was released by an intra refresh and n_pictures INCLUDES that intra picture as its last element, as
 * the reference's pre_assignment_buffer_count does (:1641-1646).  A part whose length equals the period of its own levels (8
 * pictures at 3 levels) keeps the random-access hierarchy; any other part is coded with the low-delay P structure (:1711-1727), and
 * so is the LAST part of a group cut by an intra refresh -- the one that ends with the intra picture (mini_gop_idr_count is set for
 * the last part only, :419-424, 463-472): earlier whole-period parts of such a group stay random access.
 * Returns the number of parts (<= 4) or a negative error. */
typedef struct svt_minigop_part {
    int32_t start, length;          /* pictures [start, start + length) of the group */
    int32_t hierarchical_levels;    /* of the part (mini_gop_hierarchical_levels) */
    int32_t random_access;          /* 1: hierarchical B pictures; 0: low-delay P */
} svt_minigop_part;
int32_t svt_hip_minigop_split(int32_t n_pictures, int32_t hierarchical_levels, int32_t cut_by_intra, svt_minigop_part parts[4]);

/* A set of contexts, one per device of a node, for a host that drives several GPUs from one process (one host thread per
 * device is the intended use: a context is not shared between threads).  Devices are HIP ordinals. */
typedef struct svt_hip_device_set svt_hip_device_set;
int32_t      svt_hip_device_set_create(svt_hip_device_set **set, const int32_t *device_ordinals, int32_t n_devices);
int32_t      svt_hip_device_set_size(const svt_hip_device_set *set);
svt_hip_ctx *svt_hip_device_set_ctx(svt_hip_device_set *set, int32_t index);
void         svt_hip_device_set_destroy(svt_hip_device_set *set);
/* The hand-off itself: `bytes` of device memory (a padded picture buffer) from d_src on src's device to d_dst on dst's
 * device, ordered after everything enqueued on src's stream and before everything enqueued later on dst's stream; src's
 * stream also waits for the copy, so the producer may overwrite d_src afterwards.  Peer access is enabled on first use;
 * the copy travels device to device (xGMI) when the devices are peers.  src == dst degenerates to a device-local copy. */
int32_t svt_hip_ref_handoff_device(svt_hip_ctx *src, const void *d_src, svt_hip_ctx *dst, void *d_dst, size_t bytes);

/* ------------------------------------------------------------------------------------------------------------------
 * Frame packets: the two VP9 headers (host) and the dense assembly of header || tile || trailer of a batch (device).
 *
 * Replaces eb_vp9_pack_bitstream (VPX/vp9_bitstream.c:1369-1412): write_uncompressed_header (:1186-1290), the 16-bit first_part_size,
 * write_compressed_header (:1292-1367) and the copy of the entropy coder's tile bytes behind them; and the four one-byte
 * show-existing frames Codec/EbPacketizationProcess.c:374-453 appends to a packet flagged EB_BUFFERFLAG_SHOW_EXT (svt_ivf_packetize
 * below splits such a packet again).
 *
 * The no-update rule.  The reference keeps FRAME_COUNTS at zero: the increments of eb_vp9_tokenize_sb are compiled out
 * (VPX/vp9_tokenize.c:405-425, "count-based probability update not yet supported"), tx_totals is never incremented, and
 * Codec/EbResourceCoordinationProcess.c:666 clears the counts.  With zero counts update_coef_probs writes one 0 bit per transform size
 * (tx_totals <= 20, VPX/vp9_bitstream.c:679-681), eb_vp9_cond_prob_diff_update finds no savings (VPX/vp9_subexp.c:173-185) and
 * update_mv no gain (VPX/vp9_encodemv.c:144-155): every one of them writes a 0 at probability 252.  The compressed header is therefore
 * a function of: intra-only or not, reference_mode, allow_comp_inter_inter, allow_hp -- and nothing in either header depends on device
 * data, so the host writes both, first_part_size included, before the tile has been coded.
 *
 * Fixed, as in the reference: profile 0 (8 bit, 4:2:0), segmentation off, one tile (log2_tile_cols = log2_tile_rows = 0), tx_mode
 * ALLOW_32X32, interpolation filter literal 0 (write_interp_filter(0, ..)), found = 0 in write_frame_size_with_refs. */
typedef struct svt_frame_params {
    /* frame state */
    uint8_t frame_type;                 /* 0 KEY_FRAME, 1 INTER_FRAME */
    uint8_t show_frame, error_resilient_mode, intra_only;
    uint8_t reset_frame_context;        /* 0 .. 3 */
    uint8_t refresh_frame_context, frame_parallel_decoding_mode;
    uint8_t frame_context_idx;          /* 0 .. 3 */
    /* references */
    uint8_t refresh_frame_mask;         /* ref_signal.refresh_frame_mask */
    uint8_t ref_dpb_index[3];           /* ref_signal.ref_dpb_index: LAST, GOLDEN, ALTREF; 0 .. 7 */
    uint8_t ref_frame_sign_bias[4];     /* cm->ref_frame_sign_bias; [0] (INTRA_FRAME) is not coded */
    uint8_t allow_hp;                   /* cm->allow_high_precision_mv */
    uint8_t reference_mode;             /* SVT_MODES_SINGLE_REFERENCE .. SVT_MODES_REFERENCE_SELECT */
    uint8_t allow_comp_inter_inter;     /* cpi->allow_comp_inter_inter */
    /* colour and size */
    uint8_t color_space;                /* 0 .. 6 (7, SRGB, needs profile 1) */
    uint8_t color_range;
    uint8_t pad0_[3];
    int32_t width, height;              /* 1 .. 4096 (one tile column is not codable beyond), 1 .. 65536 */
    int32_t render_width, render_height; /* 1 .. 65536 */
    /* loop filter; the last_* fields are the stream's state in front of this frame: INPUTS (encode_loopfilter updates them in
       place where a delta is sent; here the caller does, the struct is const) */
    uint8_t filter_level;               /* 0 .. 63 */
    uint8_t sharpness_level;            /* 0 .. 7 */
    uint8_t mode_ref_delta_enabled, mode_ref_delta_update;
    int8_t  ref_deltas[4], mode_deltas[2];            /* -63 .. 63 */
    int8_t  last_ref_deltas[4], last_mode_deltas[2];
    /* quantiser */
    uint8_t base_qindex;
    int8_t  y_dc_delta_q, uv_dc_delta_q, uv_ac_delta_q; /* -15 .. 15 */
    uint8_t pad1_[4];
} svt_frame_params;                     /* 64 bytes */
/* bytes of the two headers together at most; derived from the syntax in csrc/frame_core.h */
#define SVT_FRAME_HEADER_MAX 56
/* out: uncompressed header (first_part_size filled in) || compressed header; the two lengths are reported.  The compressed header is
 * built as raw bool records and coded by svt_hip_boolcode_host (framing and marker byte of eb_vp9_stop_encode included).
 * SVT_HIP_ERR_BAD_PARAMETER, and nothing written, for: a null pointer; a width of 0 or above 4096 (eb_vp9_get_tile_n_bits then gives
 * min_log2_tile_cols > 0); a height or a render size of 0 or above 65536; color_space 7; a delta q outside +-15; a loop-filter delta
 * (last_* included) outside +-63; a flag above 1; frame_type, reset_frame_context, frame_context_idx, ref_dpb_index, reference_mode,
 * filter_level or sharpness_level out of its bit width; intra_only together with show_frame on a non-key frame (the bit is not coded
 * then); a capacity below the bytes needed (SVT_FRAME_HEADER_MAX always suffices). */
int32_t svt_hip_frame_header_host(const svt_frame_params *p, uint8_t *out, uint32_t capacity, uint32_t *uncompressed_bytes, uint32_t *compressed_bytes);
/* The same two headers around a coefficient section that updates (svt_hip_coef_update_batch_device / svt_hip_coef_update_picture).
 * svt_hip_frame_header_parts_host yields the bool records of the compressed header in front of the section (at most SVT_CU_PREFIX_MAX)
 * and behind it (at most SVT_CU_SUFFIX_MAX), from the text svt_hip_frame_header_host writes them with.  svt_hip_frame_header_coef_host
 * writes the uncompressed header as above and codes the compressed header from the complete record list hdr_bools (prefix || section ||
 * suffix) with svt_hip_boolcode_host; first_part_size is the coder's answer.  With a section of four "no update" bits the bytes are
 * svt_hip_frame_header_host's.  Refused as above; a capacity below the bytes needed writes nothing the caller may use. */
int32_t svt_hip_frame_header_parts_host(const svt_frame_params *p, uint16_t *prefix, uint32_t *n_prefix, uint16_t *suffix, uint32_t *n_suffix);
int32_t svt_hip_frame_header_coef_host(const svt_frame_params *p, const uint16_t *hdr_bools, uint32_t n_hdr_bools, uint8_t *out, uint32_t capacity,
                                       uint32_t *uncompressed_bytes, uint32_t *compressed_bytes);
/* The uncompressed header alone, from the text svt_hip_frame_header_host writes it with: *bytes of it (at most
 * SVT_FRAME_UNCOMPRESSED_MAX), the 16 bits of first_part_size left 0, *size_bit their bit position (bit 0 = the most significant bit of
 * out[0]).  For callers whose compressed header is coded on the device (svt_hip_frame_parts_batch_device fills the field in).
 * Refused as above. */
#define SVT_FRAME_UNCOMPRESSED_MAX 27
int32_t svt_hip_frame_header_uncompressed_host(const svt_frame_params *p, uint8_t *out, uint32_t capacity, uint32_t *bytes, uint32_t *size_bit);
/* the one-byte frame that shows DPB slot dpb_slot (0 .. 7): eb_vp9_pack_bitstream with show_existing_frame set */
int32_t svt_hip_frame_show_existing_host(int32_t dpb_slot, uint8_t *out);

/* The header half of the frame reader (host/frame_read.c): the two headers parsed the way a decoder reads them (VP9 specification 6.2,
 * 6.3), so that what the writers above produce is proven readable and not only equal to the reference's bytes.
 * info->params: every coded field.  last_ref_deltas / last_mode_deltas are INPUTS (the stream's state in front of the frame), copied into
 * params.last_*; a delta that is not sent keeps that value.  A field the frame does not code reads 0, except what a decoder infers:
 * refresh_frame_mask 0xFF on a key frame; refresh_frame_context 0 and frame_parallel_decoding_mode 1 under error_resilient_mode; the
 * render size = the frame size when none is sent; allow_comp_inter_inter = "the sign bias of GOLDEN or ALTREF differs from LAST's" (the
 * decoder's condition for reading the reference-mode bits -- a writer that sends them under any other condition is misread);
 * reference_mode from those bits, SINGLE without them.
 * interp_filter is the filter AFTER the decoder's literal table {smooth, regular, sharp, bilinear}; tx_mode 0 ONLY_4X4 .. 3 ALLOW_32X32;
 * needs_backward_adaptation = !error_resilient_mode && !frame_parallel_decoding_mode (a decoder then adapts its probabilities after the
 * frame and leaves the fixed tables the entropy stages code with); lossless = q index 0 with all three delta qs 0.
 * uncompressed_bytes / compressed_bytes (= first_part_size): the tile starts at their sum.  A show-existing frame sets
 * show_existing_frame and show_existing_slot and nothing else (uncompressed_bytes 1).
 * SVT_HIP_ERR_UNSUPPORTED with a message in svt_hip_last_error, for syntax the writers never produce: profile above 0, found_ref,
 * a switchable filter is REPORTED (interp_filter) and not refused here, segmentation, more than one tile, TX_MODE_SELECT, any probability
 * update flag of the compressed header.  `lossless` is REPORTED too: a decoder then reads no tx_mode and runs the Walsh-Hadamard transform, the
 * writers send tx_mode all the same, so the bytes are parsed as written and a caller must not read a tile under that flag.
 * SVT_HIP_ERR_BAD_PARAMETER for bytes that are no VP9 frame: wrong marker or sync code, a header that ends early, first_part_size 0 or
 * beyond the frame, a set marker bit, a compressed header that ends inside a symbol.  Never reads at or beyond frame + size. */
#define SVT_READ_FILTER_REGULAR 0     /* EIGHTTAP: the 8-tap kernel svt_mc_kernel implements */
#define SVT_READ_FILTER_SMOOTH 1
#define SVT_READ_FILTER_SHARP 2
#define SVT_READ_FILTER_BILINEAR 3
#define SVT_READ_FILTER_SWITCHABLE 4
typedef struct svt_frame_read_info {
    svt_frame_params params;
    uint32_t uncompressed_bytes, compressed_bytes;
    uint8_t  show_existing_frame, show_existing_slot;
    uint8_t  interp_filter;             /* SVT_READ_FILTER_* */
    uint8_t  tx_mode;
    uint8_t  needs_backward_adaptation;
    uint8_t  lossless;
    uint8_t  pad_[2];
} svt_frame_read_info;                  /* 80 bytes */
int32_t svt_hip_frame_read_header_host(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2],
                                       svt_frame_read_info *info);
/* the same reader for frames whose compressed header updates coefficient probabilities: the updates are read (the inverse of the remap
 * and of the sub-exponential code, csrc/coef_update_core.h) and applied to tables_inout->coef_probs, which enters as the table the
 * update was coded against and leaves as the table the tile is coded with (svt_hip_tile_read_host takes it).  Every other update flag is
 * refused as above; the two readers above and svt_hip_frame_read_host keep refusing a coefficient update too. */
int32_t svt_hip_frame_read_header_coef_host(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2],
                                            svt_frame_read_info *info, svt_bool_tables *tables_inout);

/* The tile of a KEY FRAME read back (host/frame_read.c): the inverse of svt_hip_modes_kf_picture, svt_hip_tokenize_picture and the bool
 * coder, block by block in coding order -- partition walk, skip flag, intra modes, tokens (the Pareto tail, category bits MSB first,
 * the sign) -- with every context taken from the grid and eob map filled so far by the writers' own functions.  Outputs, host arrays the
 * caller sizes, in the formats the stages exchange: lf_mi [mi_rows][mi_stride] as svt_hip_encdec_intra_device takes it (sb_type 0 / 3 / 6 /
 * 9 / 12, tx_size by the ALLOW_32X32 rule, skip as coded, is_inter 0, modes in pad_[1] / pad_[2] and the nibbles for sb_type 0,
 * filter_level as given: the header's level after the decoder's delta rule); qcoeff n_sb * SVT_SB_COEFFS position-addressed, zero
 * wherever nothing was coded; the eob map in the encode pass's layout.  result: leaves, skipped leaves, tokens read (EOB tokens
 * included), the tile bytes consumed (vpx_reader_find_end) and whether the bool decoder consumed bits beyond the end.
 * SVT_HIP_ERR_UNSUPPORTED for a rectangular partition.  Never reads at or beyond tile + size, never writes outside the three arrays,
 * whatever the bytes are: garbage yields an error or a well-formed but meaningless picture. */
typedef struct svt_tile_read_result {
    uint32_t leaves, inter_leaves, skipped_leaves, tokens, tile_bytes, past_end;
    uint32_t odd_candidates; /* inter leaves whose NEARESTMV / NEARMV candidate or NEWMV reference is odd where no high-precision bit applies: a
                                decoder lowers such a candidate to even (find_best_ref_mvs) and would predict from another MV than the grid's */
    uint32_t pad_;
} svt_tile_read_result;                 /* 32 bytes */
int32_t svt_hip_tile_read_kf_host(const uint8_t *tile, uint32_t size, int32_t width, int32_t height, int32_t mi_stride, int32_t filter_level,
                                  const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables, svt_lf_mode_info *lf_mi, int16_t *qcoeff,
                                  uint16_t *eob_map, svt_tile_read_result *result);

/* The tile of ANY picture the writers produce, and header plus tile in one call.  An inter picture's tile is the inverse of
 * svt_hip_modes_inter_picture (csrc/modeinfo_inter_core.h: skip, is_inter, reference frames under the writers' own context functions, the
 * inter mode under the mode context, MV differences: joint, sign, class, integer bits LSB first, fraction, high-precision bit where
 * svt_mii_use_mv_hp allows one) with the candidates of every leaf derived by svt_mvr_derive (csrc/mvrefs_core.h) on the grids filled so far.
 * Outputs beside svt_hip_tile_read_kf_host's: lf_mi with is_inter, luma tx_type 0 in pad_[0] of an inter block (DCT, as the encode pass codes
 * them), filter_level by the decoder's rule from the header's level and deltas; mc_mi (MVs, ref_list through the inverse of list_ref_frame,
 * bw8 / bh8; ref_list -1 for an intra unit); ext in svt_hip_mvrefs_batch_device's output format (ref_frame at every unit; mode, ref_mv_*,
 * mode_context at leaf origins).  NEARESTMV / NEARMV take the candidate as derived, NEWMV adds the difference to slot 0 (a bit that is not coded
 * reads as set) -- the project's model of section 5.13; result->odd_candidates counts the leaves where a conformant decoder would first lower
 * the candidate's precision and so end at another MV.
 * SVT_HIP_ERR_UNSUPPORTED beside the key-frame entry's: lossless, a filter other than the regular one (switchable included), inter blocks
 * below 8x8, a reference frame with no list in list_ref_frame, a picture size that is no multiple of 8 (frame entry).  Reference scaling
 * (found_ref, or a size that differs from the reference's) is the header entry's found_ref refusal; reference sizes are not known here.
 * The same memory-safety contract: nothing at or beyond the input's end is read, nothing outside the arrays written, whatever the bytes. */
typedef struct svt_tile_read_params {
    int32_t width, height, mi_stride;
    uint8_t intra_only;             /* a key frame or an intra-only picture: the key-frame syntax, mc_mi / ext / inter_tables are not touched */
    uint8_t reference_mode, allow_hp, restrict_ref_mvs;
    uint8_t interp_filter, lossless; /* as svt_frame_read_info reports them */
    uint8_t filter_level, mode_ref_delta_enabled;
    int8_t  ref_deltas[4], mode_deltas[2];
    uint8_t ref_frame_sign_bias[4];
    uint8_t list_ref_frame[2];      /* the VP9 reference frame (1 .. 3) REF_LIST_0 / REF_LIST_1 stand for */
} svt_tile_read_params;             /* 32 bytes */
int32_t svt_hip_tile_read_host(const uint8_t *tile, uint32_t size, const svt_tile_read_params *params, const svt_bool_tables *bool_tables,
                               const svt_modes_tables *modes_tables, const svt_modes_inter_tables *inter_tables, svt_lf_mode_info *lf_mi,
                               svt_mc_mode_info *mc_mi, svt_mi_inter_ext *ext, int16_t *qcoeff, uint16_t *eob_map, svt_tile_read_result *result);
int32_t svt_hip_frame_read_host(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2], int32_t mi_stride,
                                int32_t restrict_ref_mvs, const uint8_t list_ref_frame[2], const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables,
                                const svt_modes_inter_tables *inter_tables, svt_frame_read_info *info, svt_lf_mode_info *lf_mi, svt_mc_mode_info *mc_mi,
                                svt_mi_inter_ext *ext, int16_t *qcoeff, uint16_t *eob_map, svt_tile_read_result *result);
/* header and tile in one call for frames whose compressed header updates coefficient probabilities (the entropy pass's coefficient-update
 * mode): svt_hip_frame_read_header_coef_host on a COPY of bool_tables -- the table the update was coded against -- then
 * svt_hip_tile_read_host under the copy.  tables_out (may be NULL) receives the copy, the table the tile was coded with; the caller's
 * tables are not written.  The reader above keeps refusing a coefficient update. */
int32_t svt_hip_frame_read_coef_host(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2], int32_t mi_stride,
                                     int32_t restrict_ref_mvs, const uint8_t list_ref_frame[2], const svt_bool_tables *bool_tables,
                                     const svt_modes_tables *modes_tables, const svt_modes_inter_tables *inter_tables, svt_frame_read_info *info,
                                     svt_lf_mode_info *lf_mi, svt_mc_mode_info *mc_mi, svt_mi_inter_ext *ext, int16_t *qcoeff, uint16_t *eob_map,
                                     svt_tile_read_result *result, svt_bool_tables *tables_out);

/* one picture of a batch.  header / trailer are HOST bytes (the two headers; up to four show-existing bytes): they travel to the device
 * inside the descriptor upload of the call.  d_tile / d_tile_size are the bool coder's d_bytes / d_size; d_tile may have ANY alignment. */
typedef struct svt_frame_packet {
    const uint8_t  *d_tile;
    const uint32_t *d_tile_size;
    uint32_t        tile_capacity;      /* as handed to the bool coder */
    uint8_t         header_len;         /* <= SVT_FRAME_HEADER_MAX */
    uint8_t         trailer_len;        /* <= 4 */
    uint8_t         header[SVT_FRAME_HEADER_MAX], trailer[4];
    uint8_t         pad_[6];
} svt_frame_packet;                     /* 88 bytes */
typedef struct svt_frame_entry {
    uint32_t offset, size;
} svt_frame_entry;
#define SVT_FRAME_SIZE_NONE 0xFFFFFFFFu
#define SVT_FRAME_MAX_PICS 32
/* Packet i = header || tile[0 .. *d_tile_size) || trailer at d_arena + d_table[i].offset, d_table[i].size bytes; offset = the sum of
 * the sizes in front of it: dense, no padding.  d_table[n_pics] = {total bytes, pictures without a packet}, WRITTEN always, like every
 * entry.  A picture whose *d_tile_size is SVT_BOOL_SIZE_OVERFLOW or above tile_capacity gets size = SVT_FRAME_SIZE_NONE, contributes
 * nothing, and its offset is where it would have started.  When the total exceeds arena_capacity nothing is written at or beyond
 * d_arena + arena_capacity and the contents are unspecified (offsets and the total saturate at 0xFFFFFFFF).
 * Asynchronous on the context's stream, no synchronisation, one descriptor upload: behind svt_hip_boolcode_batch_device on the same
 * context it needs no host round trip; afterwards one read of the table and one copy of `total` bytes deliver the batch.  d_arena may
 * be device memory or pinned host memory from svt_hip_host_alloc (then no copy is needed); d_table is n_pics + 1 entries of device
 * memory (or pinned host memory).  Refused, nothing launched: n_pics outside 1 .. SVT_FRAME_MAX_PICS, a null pointer (d_arena may
 * be null when arena_capacity is 0, d_tile when tile_capacity is 0), header_len above SVT_FRAME_HEADER_MAX, trailer_len above 4. */
int32_t svt_hip_frame_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_frame_packet *packets, uint8_t *d_arena, uint32_t arena_capacity,
                                   svt_frame_entry *d_table);
/* host form of the same text (csrc/frame_core.h), pure CPU; every pointer a host pointer */
int32_t svt_hip_frame_assemble_host(int32_t n_pics, const svt_frame_packet *packets, uint8_t *arena, uint32_t arena_capacity, svt_frame_entry *table);
/* the assembly kernel's constants: workgroups per picture and bytes they move in one pass of the grid-stride loop */
void svt_hip_frame_geometry(int32_t *workgroups_per_picture, int32_t *bytes_per_pass);

/* The same assembly for a picture whose compressed header is coded on the device too (a header with coefficient-probability updates,
 * svt_hip_coef_update_batch_device): packet i = uncompressed header || compressed[0 .. *d_compressed_size) || tile[0 .. *d_tile_size) ||
 * trailer.  header holds the HOST bytes of the uncompressed header (svt_hip_frame_header_uncompressed_host); its bits
 * [size_bit, size_bit + 16) are first_part_size and leave as *d_compressed_size, most significant bit first, whatever the host put there
 * (replaced, not OR-ed into).  d_compressed / d_compressed_size / compressed_capacity and d_tile / d_tile_size / tile_capacity are the
 * bool coder's d_bytes / d_size / capacity of the two streams; both buffers may have ANY alignment. */
typedef struct svt_frame_parts_packet {
    const uint8_t  *d_compressed;
    const uint32_t *d_compressed_size;
    const uint8_t  *d_tile;
    const uint32_t *d_tile_size;
    uint32_t        compressed_capacity, tile_capacity; /* as handed to the bool coder */
    uint16_t        size_bit;           /* size_bit + 16 <= 8 * header_len */
    uint8_t         header_len;         /* <= SVT_FRAME_UNCOMPRESSED_MAX */
    uint8_t         trailer_len;        /* <= 4 */
    uint8_t         header[SVT_FRAME_UNCOMPRESSED_MAX], trailer[4];
    uint8_t         pad_[5];
} svt_frame_parts_packet;               /* 80 bytes */
/* Table, offsets, density, d_table[n_pics], the saturation of sums and the arena-capacity contract are svt_hip_frame_batch_device's.  A
 * picture gets SVT_FRAME_SIZE_NONE when its tile size is SVT_BOOL_SIZE_OVERFLOW or above tile_capacity, or when its compressed size is
 * SVT_BOOL_SIZE_OVERFLOW, 0, above compressed_capacity or above 0xFFFF (what first_part_size can say).  Asynchronous on the context's
 * stream, one descriptor upload, one launch, no read-modify-write of the arena.  Refused, nothing launched: n_pics outside
 * 1 .. SVT_FRAME_MAX_PICS, a null pointer (d_arena may be null when arena_capacity is 0, d_tile / d_compressed when their capacity is
 * 0), header_len above SVT_FRAME_UNCOMPRESSED_MAX, size_bit + 16 beyond the header's bits, trailer_len above 4. */
int32_t svt_hip_frame_parts_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_frame_parts_packet *packets, uint8_t *d_arena, uint32_t arena_capacity,
                                         svt_frame_entry *d_table);
/* host form of the same text (csrc/frame_core.h), pure CPU; every pointer a host pointer */
int32_t svt_hip_frame_assemble_parts_host(int32_t n_pics, const svt_frame_parts_packet *packets, uint8_t *arena, uint32_t arena_capacity, svt_frame_entry *table);

/* ------------------------------------------------------------------------------------------------ */
/* IVF container (host only): what the reference's sample application wraps the encoder's packets in   */
/* ------------------------------------------------------------------------------------------------ */
#define SVT_IVF_STREAM_HEADER_BYTES 32
/* replaces write_ivf_stream_header (App/EbAppProcessCmd.c:515-540); frame_rate_q16 is used when numerator or
 * denominator is 0, exactly as there */
int32_t svt_ivf_stream_header(uint8_t out[SVT_IVF_STREAM_HEADER_BYTES], uint32_t width, uint32_t height, uint32_t frame_rate_q16,
                              uint32_t rate_numerator, uint32_t rate_denominator);
/* replaces the stream-writing branch of process_output_stream_buffer (App/EbAppProcessCmd.c:617-650): one encoder packet
 * -> one IVF frame, or five when the packet is flagged EB_BUFFERFLAG_SHOW_EXT (the coded frame, then the four trailing
 * one-byte show-existing-frame headers with pts - 2, - 1, + 0, + 1).  Returns bytes written or a negative error. */
int64_t svt_ivf_packetize(const uint8_t *packet, uint32_t len, uint64_t pts, int32_t show_ext, uint8_t *out, size_t capacity);

/* ------------------------------------------------------------------------------------------------------------------
 * Entropy pass: what the encode pass leaves on the device -> VP9 packets, one entry for a batch of pictures.
 *
 * The counterpart of svt_hip_encdec_batch_device for everything behind it (csrc/entropy.hip): headers (host, into the packet
 * descriptors) -> tokeniser -> inter mode labelling (inter pictures) -> mode info (svt_hip_modes_kf_batch_device over the intra-only
 * pictures, svt_hip_modes_inter_batch_device over the others) -> gate -> bool coder -> result -> frame assembly, all on the context's
 * stream, no host round trip, in that fixed order.  The stages are the existing entries; a workspace owns every buffer between them, sized
 * by the caller's budgets, and a small kernel in front of the bool coder (the gate, rules in csrc/entropy_core.h) keeps a picture that
 * exceeds a budget from being read past its buffers: its segment list is emptied, it gets no packet, and the result record says why.
 * The probability tables are the caller's: svt_hip_boolcode_set_tables, svt_hip_modes_set_tables (when a batch holds an intra-only
 * picture) and svt_hip_modes_inter_set_tables (when it holds any other) must have been called on the context.  The pass writes what it is
 * told: svt_hip_entropy_deliverable says whether a decoder will read it. */
typedef struct svt_entropy_limits {
    uint32_t max_pics;       /* pictures a call may hold, 1 .. 32 */
    uint32_t max_tokens;     /* PER PICTURE: token records */
    uint32_t max_bools;      /* bools of the tile's stream, the mode-info stage's and the tokens' together (svt_bool_stream.max_bools: the
                                context's bool-coder scratch grows with it) */
    uint32_t max_tile_bytes; /* bytes of the coded tile */
} svt_entropy_limits;
/* limits no picture of the geometry exceeds: svt_hip_tokenize_capacity; svt_hip_boolcode_bools_capacity of it plus
 * svt_hip_modes_inter_bools_capacity; svt_hip_boolcode_capacity of that.  All 0 for a geometry the stages do not take */
void svt_hip_entropy_limits_worst(int32_t width, int32_t height, int32_t max_pics, svt_entropy_limits *out);
/* device bytes svt_hip_entropy_work_create takes under these limits (0: it would refuse them).  Per picture, each part rounded up to 16:
 * 4 * (W/4 * H/4 * 3/2) tok_off + 4 * (SBs + 1) sb_off + 4 * max_tokens + 12 * (H/8 * mi_stride) extension records
 * + 2 * svt_hip_modes_inter_bools_capacity + 12 * svt_hip_modes_segments + max_tile_bytes + 64; times max_pics.
 * The bool coder's scratch (about 11 bytes per bool of max_bools and picture) is the context's and is not counted here */
uint64_t svt_hip_entropy_work_bytes(int32_t width, int32_t height, int32_t mi_stride, const svt_entropy_limits *limits);
typedef struct svt_entropy_work svt_entropy_work; /* opaque */
/* Refused: a null pointer, a geometry svt_hip_tokenize_batch_device refuses, max_pics outside 1 .. 32, max_bools beyond the bool coder's
 * 32-bit bit positions (7 * (max_bools + 33) >= 2^32).  One workspace serves calls of that geometry on that context, one at a time:
 * a call may be enqueued behind another (the stream orders them), the packets of the first are in the caller's arena by then */
int32_t svt_hip_entropy_work_create(svt_hip_ctx *ctx, int32_t width, int32_t height, int32_t mi_stride, const svt_entropy_limits *limits, svt_entropy_work **work);
void    svt_hip_entropy_work_destroy(svt_hip_ctx *ctx, svt_entropy_work *work);

/* one picture of a batch; every pointer is a device pointer (host pointers in the host form); the grids have the workspace's mi_stride.
 *   d_lf_mi, d_qcoeff, d_eob_map   what svt_hip_encdec_batch_device / svt_hip_encdec_intra_device leave (svt_tok_picture's inputs)
 *   d_mc_mi     the prediction grid; NULL exactly when the picture is a key frame or intra_only
 *   d_counts    the tokeniser's coef_counts (SVT_TOK_COUNTS, overwritten); may be NULL
 *   frame       the two headers are written from it by svt_hip_frame_header_host; width and height are the workspace's; reference_mode,
 *               allow_hp and ref_frame_sign_bias are also the mode stages' parameters
 *   list_ref_frame, restrict_ref_mvs   as in svt_md_inter_picture (inter pictures)
 *   trailer     up to four show-existing bytes behind the tile */
typedef struct svt_entropy_picture {
    const svt_lf_mode_info *d_lf_mi;
    const svt_mc_mode_info *d_mc_mi;
    const int16_t          *d_qcoeff;   /* 16-byte aligned */
    const uint16_t         *d_eob_map;
    uint32_t               *d_counts;
    svt_frame_params        frame;
    uint8_t                 list_ref_frame[2], restrict_ref_mvs, trailer_len, trailer[4];
} svt_entropy_picture;                  /* 112 bytes */

#define SVT_ENT_BAD_GRID 1u        /* a stage answered SVT_MODES_BAD_GRID */
#define SVT_ENT_TOKENS_OVER 2u     /* the tokeniser's total > max_tokens */
#define SVT_ENT_MODE_BOOLS_OVER 4u /* the mode-info stage's bools > its buffer (never under the stage's own capacity, which the workspace uses) */
#define SVT_ENT_UNFAITHFUL_MV 8u   /* the labelling's d_status[2] != 0: a NEWMV leaf the syntax cannot code faithfully */
#define SVT_ENT_STREAM_OVER 16u    /* the bool coder found more bools than max_bools */
#define SVT_ENT_TILE_OVER 32u      /* the tile has more bytes than max_tile_bytes */
/* flags 0: the picture has a packet.  tokens and mode_bools are the stages' totals as they wrote them (mode_bools SVT_MODES_BAD_GRID for a
 * refused grid); tile_bytes is 0 for a picture without a packet; the leaf counts are the labelling's d_status[0 .. 2], 0 for an intra-only
 * picture or a refused grid */
typedef struct svt_entropy_result {
    uint32_t flags, tokens, mode_bools, tile_bytes, inter_leaves, newmv_leaves, unfaithful_leaves, pad_;
} svt_entropy_result;              /* 32 bytes */

/* n_pics (<= the workspace's max_pics) pictures, key and inter pictures in any mix; packets, table and offsets as svt_hip_frame_batch_device
 * documents them, in the caller's picture order: a picture whose flags are not 0 has size SVT_FRAME_SIZE_NONE, contributes no bytes and
 * is counted in d_table[n_pics].size.  d_table (n_pics + 1 entries) and d_results (n_pics records, 4-byte aligned) may be device or pinned
 * host memory, like d_arena.  Asynchronous on the context's stream, no synchronisation.
 * Refused with SVT_HIP_ERR_BAD_PARAMETER, NOTHING launched: a null pointer (d_arena may be null when arena_capacity is 0); n_pics outside
 * 1 .. max_pics; a workspace of another context; a null d_lf_mi / d_qcoeff / d_eob_map, d_qcoeff not 16-byte aligned; d_mc_mi null on an
 * inter picture or set on a key / intra_only picture; trailer_len above 4; frame parameters svt_hip_frame_header_host refuses; frame.width /
 * frame.height other than the workspace's; on an inter picture list_ref_frame outside 1 .. 3; tables (above) that have not been set */
int32_t svt_hip_entropy_batch_device(svt_hip_ctx *ctx, svt_entropy_work *work, int32_t n_pics, const svt_entropy_picture *pics, uint8_t *d_arena,
                                     uint32_t arena_capacity, svt_frame_entry *d_table, svt_entropy_result *d_results);
/* profiling aid, like svt_hip_encdec_work_set_stage_hook: called on the enqueueing thread in front of every stage and once at the end */
#define SVT_ENT_STAGE_HEADERS 0
#define SVT_ENT_STAGE_TOKENS 1
#define SVT_ENT_STAGE_LABELS 2
#define SVT_ENT_STAGE_MODES 3
#define SVT_ENT_STAGE_GATE 4
#define SVT_ENT_STAGE_BOOLCODE 5
#define SVT_ENT_STAGE_RESULT 6
#define SVT_ENT_STAGE_FRAME 7
#define SVT_ENT_STAGE_END 8
#define SVT_ENT_STAGE_COEF_UPDATE 9 /* between MODES and GATE, in the coefficient-update mode only (below) */
void svt_hip_entropy_work_set_stage_hook(svt_entropy_work *work, void (*hook)(void *user, int32_t stage), void *user);
/* where picture `pic` (0 .. max_pics - 1) of the workspace keeps its intermediates: for inspection and measurement */
typedef struct svt_entropy_buffers {
    uint32_t         *d_tok_off, *d_sb_off, *d_tokens;
    svt_mi_inter_ext *d_ext;
    uint32_t         *d_status;   /* the labelling's four words */
    uint16_t         *d_bools;
    svt_bool_segment *d_segments;
    uint32_t         *d_n_bools;
    uint8_t          *d_tile;
    uint32_t         *d_tile_size, *d_verdict;
    uint32_t          n_segments, n_sb;
} svt_entropy_buffers;
int32_t svt_hip_entropy_work_buffers(const svt_entropy_work *work, int32_t pic, svt_entropy_buffers *out);

/* Forward coefficient-probability updates, an opt-in mode of the pass.  With it on a batch goes from grids, coefficients and eob maps to
 * dense packets whose compressed headers carry the coefficient updates (svt_hip_coef_update_batch_device) and whose tiles are coded under
 * the updated probabilities, on one stream, no host round trip.  The order is then: headers (host: the uncompressed header and
 * svt_hip_frame_header_parts_host) -> tokeniser (with counts) -> labelling -> mode info -> coefficient update (d_n_tokens the tokeniser's
 * total on the device, max_tokens the limits', d_old_probs NULL) -> gate -> bool coder over the tiles under every picture's own table
 * (svt_hip_boolcode_batch_tables_device) -> bool coder over the compressed headers (a second call: 32 pictures make 64 streams, above
 * SVT_BOOL_MAX_STREAMS; one path for every batch size) -> result -> svt_hip_frame_parts_batch_device.  The stage hook reports
 * SVT_ENT_STAGE_COEF_UPDATE between MODES and GATE in this mode only.  With the mode off the pass is what it was.
 * Every picture is coded against the context's table: the pass refuses, with nothing launched, a picture with !error_resilient_mode &&
 * refresh_frame_context in this mode -- a decoder would keep the updated probabilities in its frame context while the next picture is
 * again coded against the defaults.  Chaining pictures is out of scope.
 * A picture the gate withholds (TOKENS_OVER ...) is safe: the update stage's scan is bounded by max_tokens, its header stream is coded and
 * ignored.  The header stream itself cannot overflow (csrc/entropy_core.h), so the result record has no flag for it.
 * svt_hip_entropy_work_set_coef_update: the first enabling allocates a second slab of svt_hip_entropy_coef_update_bytes(limits) bytes
 * (SVT_HIP_ERR_NO_RESOURCES when that fails; the mode then stays off); later calls only switch.  It synchronises nothing: the switch
 * holds for the calls enqueued after it.  Per picture the second slab holds, each part rounded up to 16: 4 * SVT_TOK_COUNTS coefficient
 * counts (used when the picture's d_counts is NULL) + 2 304 eob_branch + 1 728 probabilities + 2 * svt_hip_coef_update_bools_capacity()
 * header records + svt_hip_boolcode_capacity(svt_hip_coef_update_bools_capacity()) header bytes + sizeof(svt_cu_result) + 64 (the record
 * count, the segment, the header's size); times max_pics.  0 for limits a workspace cannot be created under. */
int32_t  svt_hip_entropy_work_set_coef_update(svt_hip_ctx *ctx, svt_entropy_work *work, int32_t on);
uint64_t svt_hip_entropy_coef_update_bytes(const svt_entropy_limits *limits);
typedef struct svt_entropy_coef_buffers {
    uint32_t         *d_counts, *d_eob_branch;
    uint8_t          *d_probs;
    uint16_t         *d_hdr_bools;
    uint8_t          *d_hdr_bytes;
    svt_cu_result    *d_result;
    uint32_t         *d_n_hdr_bools;
    svt_bool_segment *d_segment;
    uint32_t         *d_hdr_size;
    uint32_t          hdr_bools_capacity, hdr_capacity;
} svt_entropy_coef_buffers;
/* refused while the mode has never been enabled on the workspace */
int32_t svt_hip_entropy_work_coef_buffers(const svt_entropy_work *work, int32_t pic, svt_entropy_coef_buffers *out);

/* The same pass on host pointers, one picture (host/entropy_host.c): the stages' host forms in the same order and the same gate text; the
 * model of the device entry.  packet (capacity bytes) receives header || tile || trailer; *packet_size its size, SVT_FRAME_SIZE_NONE for a
 * picture without a packet (nothing is then written).  limits->max_pics is not read.  detail (may be NULL) reports what only the host
 * knows.  Refused as the device entry refuses; also a packet_capacity below the packet's size */
typedef struct svt_entropy_host_detail {
    uint32_t stream_bools; /* bools of the tile's stream: what max_bools is compared with (0 when phase A withheld the picture) */
    uint32_t header_bytes; /* the two headers together */
    uint32_t coded_size;   /* the bool coder's answer: the tile's bytes (the empty stream's when phase A withheld the picture), or SVT_BOOL_SIZE_OVERFLOW */
    uint32_t pad_;
} svt_entropy_host_detail;
int32_t svt_hip_entropy_picture(const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables, const svt_modes_inter_tables *inter_tables,
                                const svt_entropy_picture *pic, int32_t mi_stride, const svt_entropy_limits *limits, uint8_t *packet, uint32_t packet_capacity,
                                uint32_t *packet_size, svt_entropy_result *result, svt_entropy_host_detail *detail);
/* The pass in the coefficient-update mode on host pointers: the arguments of svt_hip_entropy_picture, the stages' host forms in the
 * device entry's order of that mode and the same gate text; packet receives uncompressed header || compressed header || tile || trailer.
 * probs (1 728 bytes, may be NULL) receives the probabilities the tile was coded with, update (may be NULL) the stage's record.  Refused
 * as svt_hip_entropy_picture refuses, and a picture with !error_resilient_mode && refresh_frame_context */
int32_t svt_hip_entropy_picture_coef(const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables, const svt_modes_inter_tables *inter_tables,
                                     const svt_entropy_picture *pic, int32_t mi_stride, const svt_entropy_limits *limits, uint8_t *packet, uint32_t packet_capacity,
                                     uint32_t *packet_size, svt_entropy_result *result, svt_entropy_host_detail *detail, uint8_t *probs, svt_cu_result *update);
/* the gate's two rules and the result record on plain values (csrc/entropy_core.h): status NULL for an intra-only picture.  Returns what
 * the tile's size word becomes */
uint32_t svt_hip_entropy_gate_host(uint32_t tok_total, uint32_t max_tokens, uint32_t n_bools, uint32_t bools_capacity, const uint32_t *status, uint32_t size,
                                   uint32_t max_tile_bytes, uint32_t *verdict_a, svt_entropy_result *result);

/* What a decoder needs beyond well-formed bytes (the findings of the frame reader); reported, not refused: the pass stays a faithful writer */
#define SVT_ENT_NEEDS_BACKWARD_ADAPTATION 1u /* !error_resilient_mode && !frame_parallel_decoding_mode: a decoder adapts its probabilities */
#define SVT_ENT_LOSSLESS 2u                  /* q index 0 and all delta qs 0: a decoder reads no tx_mode and runs the Walsh-Hadamard transform */
#define SVT_ENT_COMP_FLAG_MISMATCH 4u        /* inter picture: allow_comp_inter_inter differs from "GOLDEN's or ALTREF's sign bias differs from LAST's" */
#define SVT_ENT_REFERENCE_MODE_UNREAD 8u     /* inter picture: reference_mode is not SINGLE while that condition is false: a decoder assumes SINGLE */
uint32_t svt_hip_entropy_deliverable(const svt_frame_params *p);
/* comp_fixed_ref / comp_var_ref from cm->ref_frame_sign_bias: the rule of eb_vp9_setup_compound_reference_mode */
void svt_hip_compound_refs_from_sign_bias(const uint8_t sign_bias[4], uint8_t *comp_fixed_ref, uint8_t comp_var_ref[2]);

#ifdef __cplusplus
}
#endif
#endif /* SVTVP9_HIP_H */

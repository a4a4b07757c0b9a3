/* svt_ctx.h -- context object behind the C ABI (include/svtvp9_hip.h) and small launch helpers. */
#ifndef SVT_CTX_H
#define SVT_CTX_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/svtvp9_hip.h"

/* the context's grow-only device buffers (svt_ctx_slot): every buffer has a name here, one line a stage, so that no two stages can pick
 * the same one; a new stage adds a line in front of SVT_CTX_SLOTS.  A family indexed by arithmetic is a base and its extent (_N), and the
 * site that does the arithmetic checks it against the extent at compile time.  Nothing outside csrc sees the numbers. */
enum { SVT_SLOT_ME_PLANES_N = 9, SVT_SLOT_MC_REF_N = 6 };
enum svt_ctx_slot_id {
    SVT_SLOT_ME_PLANES,                                      /* svt_hip_me_picture: + 3 * picture (cur, ref0, ref1) + level (full, 1/4, 1/16) */
    SVT_SLOT_ME_RESULTS = SVT_SLOT_ME_PLANES + SVT_SLOT_ME_PLANES_N, SVT_SLOT_ME_RCME,       /* svt_hip_me_picture's device twins */
    SVT_SLOT_ME_PROF, SVT_SLOT_ME_REDO,                                                      /* me_launch: profile counters, redo flags */
    SVT_SLOT_TQ_SRC, SVT_SLOT_TQ_PRED, SVT_SLOT_TQ_RECON, SVT_SLOT_TQ_BLOCKS, SVT_SLOT_TQ_QTABS, SVT_SLOT_TQ_ISCAN, SVT_SLOT_TQ_QCOEFF,
    SVT_SLOT_TQ_DQCOEFF, SVT_SLOT_TQ_EOB,                                                    /* svt_hip_tq_batch's device twins */
    SVT_SLOT_LF_Y, SVT_SLOT_LF_U, SVT_SLOT_LF_V, SVT_SLOT_LF_MASK,                           /* svt_hip_lf_frame's device twins */
    SVT_SLOT_LF_EDESC,                                                                       /* lf_launch: edge descriptors */
    SVT_SLOT_MC_MI, SVT_SLOT_MC_PRED,                                                        /* svt_hip_inter_pred_frame's device twins, and */
    SVT_SLOT_MC_REF,                                                                         /* + 3 * list (0, 1) + plane (Y, Cb, Cr) */
    SVT_SLOT_RATE_QCOEFF = SVT_SLOT_MC_REF + SVT_SLOT_MC_REF_N, SVT_SLOT_RATE_BLOCKS, SVT_SLOT_RATE_TABLES, SVT_SLOT_RATE_SCAN,
    SVT_SLOT_RATE_BITS,                                                                      /* svt_hip_rate_batch's device twins */
    SVT_SLOT_TOK_SCAN,                                                                       /* tokenize.hip: the canonical scan array */
    SVT_SLOT_TOK_QCOEFF, SVT_SLOT_TOK_BLOCKS, SVT_SLOT_TOK_TOKENS, SVT_SLOT_TOK_OFF, SVT_SLOT_TOK_COUNTS, /* svt_hip_tokenize_blocks' device twins */
    SVT_SLOT_BC_SCRATCH, SVT_SLOT_BC_TABLES, SVT_SLOT_BC_IN, SVT_SLOT_BC_OUT,                /* boolcode.hip */
    SVT_SLOT_MI_SB_OFF, SVT_SLOT_MI_TABLES,                                                  /* modeinfo.hip: per-SB offsets, probabilities */
    SVT_SLOT_MII_SB_OFF, SVT_SLOT_MII_TABLES,                                                /* modeinfo_inter.hip: the same */
    SVT_SLOT_MVR_PART,                                                                       /* mvrefs.hip: per-SB partial sums */
    SVT_SLOT_MDI_PART, SVT_SLOT_MDI_LABEL,                                                   /* md_inter.hip: partial sums, the labelled records */
    SVT_SLOT_CU_SCRATCH,                                                                     /* coef_update.hip: partial histograms, the sizes' sections */
    SVT_CTX_SLOTS
};
#define SVT_CTX_RING 64
#define SVT_CTX_UPLOAD_RING 4   /* pinned staging buffers of svt_hip_mem_upload_2d_async */
#define SVT_CTX_MARKERS 1024    /* completion markers in flight (svt_hip_ctx_marker_*) */

struct svt_hip_ctx {
    int         device;
    hipStream_t stream;
    int         owns_stream;
    hipEvent_t  ev_start, ev_stop;
    int         timed;
    int         cu_count;  /* compute units of the device (queried once at creation) */
    int         me_instance; /* kernel instance of the last ME launch: me_spec.h index, + 100 for me_fast.h's driver, + 200 for the two launches of the compact layout (me_layout.h) */
    int         intra_wgs;   /* svt_hip_ctx_set_intra_workgroups: 64-lane workers of the intra pass launched on this context (0 = default) */
    /* ring of staging slots (pinned host + device twin) for launch descriptors: a slot is reused only after the event
       recorded behind its host-to-device copy has completed (svt_ctx_stage_send), so launches never synchronise the stream */
    void       *ring_host[SVT_CTX_RING];
    void       *ring_dev[SVT_CTX_RING];
    size_t      ring_bytes[SVT_CTX_RING];
    hipEvent_t  ring_ev[SVT_CTX_RING];
    int         ring_used[SVT_CTX_RING];
    int         ring_own[SVT_CTX_RING];   /* 1: the entry outgrew its share of the slabs below and owns its buffers */
    void       *ring_slab_host, *ring_slab_dev; /* SVT_CTX_RING x 64 KB, taken when the context is created (an entry used to take its buffers the
                                                   first time round the ring: 64 pairs of allocations inside the first pictures of a stream) */
    int         ring_pos;
    /* asynchronous uploads: the caller's rows are copied into a pinned buffer of this ring before the call returns, the device
       copy is ordered on the stream; a buffer is reused once the event behind its copy has completed */
    void       *up_host[SVT_CTX_UPLOAD_RING];
    size_t      up_bytes[SVT_CTX_UPLOAD_RING];
    hipEvent_t  up_ev[SVT_CTX_UPLOAD_RING];
    int         up_used[SVT_CTX_UPLOAD_RING];
    int         up_pos;
    double      up_prof[3];     /* SVT_HIP_SHIM_PROFILE: seconds waiting for a staging slot / copying rows / enqueuing, and */
    long        up_prof_n;      /* the number of uploads (svt_hip_mem_upload_planes_async) */
    hipEvent_t  direct_ev;      /* behind the last upload that reads the caller's (page-locked) memory directly */
    int         direct_pending;
    /* completion markers: marker m is event m % SVT_CTX_MARKERS; before an event is recorded again its previous use is waited
       for, so a marker older than SVT_CTX_MARKERS records is complete by construction */
    hipEvent_t  mk_ev[SVT_CTX_MARKERS];
    uint64_t    mk_next;
    /* dedicated events of svt_hip_ref_handoff_device (producer side / consumer side) */
    hipEvent_t  ho_produced, ho_consumed;
    void       *slot[SVT_CTX_SLOTS]; /* grow-only device buffers of the host-pointer convenience entry points */
    size_t      slot_bytes[SVT_CTX_SLOTS];
};

int32_t svt_set_error(int32_t code, const char *msg);
int32_t svt_set_hip_error(hipError_t e, const char *file, int line);
/* A launch descriptor goes to the device in two steps.  svt_ctx_stage takes the next staging slot with at least `bytes` in both twins
 * (0 on success); the caller fills the host twin and may still return: nothing is in flight.  svt_ctx_stage_send copies the first `n`
 * bytes of the host twin to `dst` (null: the slot's device twin) on ctx->stream and commits the slot in the same call; after it the
 * caller owes the ring nothing on any path, and when the copy fails nothing is in flight and the slot is not committed.
 * The commit's event sits right behind the copy, and that is enough: a context has exactly one stream, so every kernel that reads or
 * writes the device twin is enqueued on it behind the copy, and a later use of the slot starts with a copy on that same stream, behind
 * those kernels.  The event only keeps the host from rewriting the host twin while the copy is in flight.
 * svt_ctx_stage_commit (record the slot's event, move on to the next slot) is the primitive behind svt_ctx_stage_send and nothing
 * else calls it; until it has run, svt_ctx_stage answers with the same slot. */
int   svt_ctx_stage(svt_hip_ctx *ctx, size_t bytes, void **host, void **dev);
void  svt_ctx_stage_commit(svt_hip_ctx *ctx);
void *svt_ctx_slot(svt_hip_ctx *ctx, int slot, size_t bytes);
inline hipError_t svt_ctx_stage_send(svt_hip_ctx *ctx, size_t n, void *dst = nullptr) {
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, n, &h, &d)) return (hipError_t)1; /* hipErrorInvalidValue: no slot of n bytes had been taken */
    const hipError_t e = hipMemcpyAsync(dst ? dst : d, h, n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) svt_ctx_stage_commit(ctx);
    return e;
}

/* transform stage over device-built block lists (tq_kernel.hip; used by encdec.hip) */
int32_t svt_tq_launch_device_lists(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *const *recon_set, int n_set,
                                   const svt_tq_block *d_blocks, const int32_t cap[4], const int32_t *d_off_cnt, const svt_quant_tables *d_qtabs,
                                   const int16_t *d_iscan, int16_t *d_qcoeff, int16_t *d_dqcoeff, uint16_t *d_eob, uint64_t *d_dist,
                                   const uint32_t *d_pos, const void *d_geom, int geom_stride, const uint32_t *d_iscan_off, int sb_cols);
/* the (up to 8) reconstruction base pointers of a launch, staged through the descriptor ring: *d_set = the device copy, null beyond n_set
 * (tq_kernel.hip; used by recon_kernel.hip too) */
int32_t tq_stage_recon_set(svt_hip_ctx *ctx, uint8_t *const *recon_set, int n_set, const uint8_t *const **d_set);

/* reconstruction from coefficients over device-built block lists (recon_kernel.hip; used by encdec.hip's decode pass) */
int32_t svt_rc_launch_device_lists(svt_hip_ctx *ctx, const uint8_t *d_pred, uint8_t *const *recon_set, int n_set, const int32_t cap[4], const int32_t *d_off_cnt,
                                   const svt_quant_tables *d_qtabs, const int16_t *d_qcoeff, uint16_t *d_eob_list, const uint32_t *d_pos, const void *d_geom,
                                   const void *d_eob_maps, int geom_stride, const uint32_t *d_iscan_off, int sb_cols, uint32_t *d_overflow);

/* encode pass of an intra picture / the stand-in intra decision (intra_kernel.hip; used by encdec.hip).  d_sync: 2 + 3 * (number of
 * 16x16 luma cells) dwords of scratch */
int32_t svt_intra_launch(svt_hip_ctx *ctx, const svt_encdec_picture *p, int32_t width, int32_t height, int32_t mi_stride, const svt_quant_tables *d_qtabs,
                         const int16_t *d_iscan, const uint32_t iscan_off[16], int32_t *d_sync, int32_t *d_status, int32_t mixed);
/* decode pass of an intra picture's blocks (intra_recon_kernel.hip; used by encdec.hip): the same walk from coefficients and eobs.  d_sync as
 * above; d_status_grid |= 1 for a malformed grid; d_overflow (may be null) += coefficients whose dequantised product left 16 bits */
int32_t svt_intra_rc_launch(svt_hip_ctx *ctx, const svt_encdec_picture *p, int32_t width, int32_t height, int32_t mi_stride, const svt_quant_tables *d_qtabs,
                            const uint32_t iscan_off[16], int32_t *d_sync, int32_t *d_status_grid, uint32_t *d_overflow, int32_t mixed);
int32_t svt_md_intra_default_launch(svt_hip_ctx *ctx, svt_lf_mode_info *d_lf_mi, int32_t mi_stride, int32_t mi_rows, int32_t mi_cols, int32_t filter_level);

#define HIP_TRY(expr)                                                        \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) return svt_set_hip_error(e_, __FILE__, __LINE__); \
    } while (0)

/* the bracket behind svt_hip_last_kernel_ms: begin() records ev_start, end() checks the launches and records ev_stop.  A return in
 * between closes the bracket from the destructor, so ev_start and ev_stop are always a pair of one call; `timed` changes only in end() */
struct svt_ctx_timer {
    svt_hip_ctx *ctx;
    bool         open;
    explicit svt_ctx_timer(svt_hip_ctx *c) : ctx(c), open(false) {}
    svt_ctx_timer(const svt_ctx_timer &) = delete;
    svt_ctx_timer &operator=(const svt_ctx_timer &) = delete;
    ~svt_ctx_timer() { if (open) (void)hipEventRecord(ctx->ev_stop, ctx->stream); }
    hipError_t begin() {
        const hipError_t e = hipEventRecord(ctx->ev_start, ctx->stream);
        open = e == hipSuccess;
        return e;
    }
    hipError_t end() {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(ctx->ev_stop, ctx->stream);
        if (e != hipSuccess) return e; /* (the destructor tries ev_stop once more) */
        open = false;
        ctx->timed = 1;
        return hipSuccess;
    }
};

/* replace the constant tables a stage keeps in a grow-only buffer; `name` is the stage's error prefix */
inline int32_t svt_ctx_set_tables(svt_hip_ctx *ctx, int slot, const void *tables, size_t bytes, const char *name) {
    char msg[64];
    snprintf(msg, sizeof msg, "%s: %s", name, ctx && tables ? "tables" : "null argument");
    if (!ctx || !tables) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, msg);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream)); /* (a call in flight may still read the tables) */
    void *d = svt_ctx_slot(ctx, slot, bytes);
    if (!d) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, msg);
    HIP_TRY(hipMemcpyAsync(d, tables, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SVT_HIP_OK;
}
#endif

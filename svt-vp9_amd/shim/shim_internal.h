/*
 * shim_internal.h -- the state of libSvtVp9Enc.so (enc_shim.c): options, fences, slots, groups, devices.  DESIGN.md section 7.
 */
#ifndef SHIM_INTERNAL_H
#define SHIM_INTERNAL_H
#include <pthread.h>
#include <stdint.h>

#include "../../include/svt_vp9_enc_api.h"
#include "../../include/svtvp9_hip.h"
#include "shim_plan.h"

#define SHIM_MAX_DEV 8
#define SHIM_REF_PAD 80 /* border of a reference picture: 64 + 16 (Codec/EbEncHandle.c:968-971) */
#define SHIM_WAVE_MAX 8 /* pictures per EncDec batch (the deepest temporal layer of a 16-picture mini-GOP) */

/* ---- shim_config.c: the configuration rules of the reference, no device behind them ---- */
void        shim_load_defaults(EbSvtVp9EncConfiguration *c);
/* copy_api_from_app + verify_settings: the library's copy of *in (frame rate, automatic intra period resolved) and its hierarchical levels */
EbErrorType shim_resolve_config(const EbSvtVp9EncConfiguration *in, EbSvtVp9EncConfiguration *out, int *levels);

/* ---- the environment's switches, read ONCE per encoder (read_options; the table is in DESIGN.md section 7) ---- */
typedef struct shim_options {
    int n_dev, ordinal[SHIM_MAX_DEV]; /* SVT_HIP_DEVICES (closed GOPs are dealt round-robin to them), else SVT_HIP_DEVICE, else 0 */
    int intra_search;     /* SVT_HIP_INTRA_DECISION=search: intra pictures no callback decided go through the open-loop intra search */
    int inter_mixed;      /* SVT_HIP_INTER_DECISION=mixed: inter pictures no callback decided get the mixed stand-in */
    int ring_groups;      /* SVT_HIP_RING_GROUPS, 2..8: mini-GOPs a device's picture ring holds */
    int single_stream;    /* SVT_HIP_SINGLE_STREAM=1: everything on the main stream, no feeder */
    int no_upload_stream, deep_stream, no_key_stream;
    int me_stream;        /* SVT_HIP_ME_STREAM: 0 / 1, -1 = unset (on without reconstructed output) */
    int share_streams;    /* a repeated ordinal runs on the streams of its first context (SVT_HIP_SHARE_STREAMS=0: streams of its own) */
    int split_gop;        /* SVT_HIP_SPLIT_GOP=1 with several devices: consecutive mini-GOPs on consecutive devices */
    int register_input;   /* SVT_HIP_REGISTER_INPUT=1: the caller's planes are page-locked and read directly */
    int feeder;           /* SVT_HIP_FEEDER != 0 and not SVT_HIP_NO_FEEDER=1 */
    int profile;          /* SVT_HIP_SHIM_PROFILE: 1 = host time per section at deinit, 2 = + per key frame */
    int warmup;           /* a throw-away encoder runs every kernel once at init (SVT_HIP_WARMUP=0: off) */
} shim_options;

/* ---- a point in a stream: "everything enqueued on ctx up to here" (svt_hip_ctx_marker_*).  A fence knows its own context, so whoever
 * waits for it names only the waiter. ---- */
typedef struct shim_fence { svt_hip_ctx *ctx; uint64_t value; int set; } shim_fence;

static inline int32_t fence_record(svt_hip_ctx *ctx, shim_fence *f) {
    const int32_t r = svt_hip_ctx_marker_record(ctx, &f->value);
    f->ctx = ctx;
    f->set = r == SVT_HIP_OK;
    return r;
}
/* device side: what waiter enqueues from here on runs behind the fence (stream order already says so on the fence's own context) */
static inline int32_t fence_order(svt_hip_ctx *waiter, const shim_fence *f) {
    return (!f->set || f->ctx == waiter) ? SVT_HIP_OK : svt_hip_ctx_wait_marker(waiter, f->ctx, f->value);
}
static inline int32_t fence_wait_host(const shim_fence *f) { return f->set ? svt_hip_ctx_marker_wait(f->ctx, f->value) : SVT_HIP_OK; } /* blocks */
static inline int32_t fence_query(const shim_fence *f) { return f->set ? svt_hip_ctx_marker_query(f->ctx, f->value) : 1; } /* 1 reached, 0 not yet, < 0 error */
static inline void    fence_clear(shim_fence *f) { f->set = 0; }

typedef struct shim_packet {
    EbBufferHeaderType  hdr;
    struct shim_packet *next;
    int                 dev;
    shim_fence          done;   /* the GPU work behind this packet */
    int                 ready;  /* `done` is valid: a packet is queued (in decode order) when its group is planned and completed by the device's
                                   feeder once the group's work has been enqueued (release / acquire: feeder thread -> caller) */
} shim_packet;

typedef struct shim_recon { /* one reconstructed picture on its way to eb_vp9_svt_get_recon: pinned host memory, filled asynchronously */
    struct shim_recon *next;
    uint8_t           *host;
    uint8_t           *d_tight; /* device: the picture's three planes packed tight (Y | Cb | Cr), what ONE device-to-host transfer then carries */
    int                dev;
    shim_fence         done;    /* output context: the copy has arrived */
    int64_t            pts;
    uint32_t           flags;
    int                ready;   /* as shim_packet.ready */
} shim_recon;

typedef struct shim_slot { /* one buffered picture, everything device resident */
    int64_t        number;  /* display order, -1 = empty */
    int64_t        pts;
    svt_pa_picture pa;
    uint8_t       *d_src;   /* Y (W x H) then Cb then Cr, tight: inside the device's source slab */
    uint8_t       *d_pred;  /* prediction picture, same layout: inside the prediction slab */
    uint8_t       *d_rec;   /* reconstruction = reference picture, three padded planes */
    void          *d_results, *d_mean, *d_var, *d_rcme, *d_stats, *d_hist;
    void          *d_mc_mi, *d_lf_mi, *d_eob_map, *d_lfm, *d_nz;
    int16_t       *d_qcoeff, *d_dqcoeff;
    int            processed;   /* its ME (or, for an intra picture, its analysis) has been enqueued */
    int            coded;       /* the stages behind mode decision have been enqueued */
    int            is_copy;     /* split-GOP mode: the base picture of the previous mini-GOP, handed over from the device that coded it
                                   (analysed planes + reference picture only) */
    shim_fence     done;        /* completion of everything enqueued for this picture so far */
    shim_fence     free_main;   /* main context: nothing enqueued so far reads this slot's buffers behind it */
    shim_fence     free_deep;   /* the same for the deep-layer context */
    shim_fence     out;         /* output context: the device-to-host copy of this slot's reconstruction */
    svt_vp9_shim_picture_info info;
} shim_slot;

/* A planned group: everything the enqueuing side needs, fixed by the caller's thread (plan_group) -- the plan (shim_plan.h), the ME
 * parameters of its pictures, the packets (and reconstruction records) already queued in output order, the fences its work follows.
 * run_group enqueues it: on the caller's thread, or on the device's feeder. */
typedef struct shim_group {
    shim_plan     plan;
    svt_me_params me[SHIM_MAX_MINIGOP];
    shim_packet  *pkt[SHIM_MAX_MINIGOP];
    shim_recon   *rec[SHIM_MAX_MINIGOP];
    int           end_of_stream, dev;
    shim_fence    in;   /* input context: the group's last picture uploaded and analysed */
    shim_fence    key;  /* the GOP's intra picture, which the group's waves predict from (set for the GOP's first group only) */
} shim_group;

struct shim_state;
typedef struct shim_dev { /* one device: its contexts (streams; what each is for and when it is the main context: DESIGN.md section 7), ring, feeder */
    svt_hip_ctx     *ctx;            /* main: the group's shallow waves, and whatever has no stream of its own */
    svt_hip_ctx     *ctx_in;         /* picture analysis, behind each picture's upload: mini-GOP k + 1 crosses PCIe while mini-GOP k computes */
    svt_hip_ctx     *ctx_up;         /* the uploads themselves: nothing but host-to-device copies, back to back.  Owned by the caller's thread. */
    svt_hip_ctx     *ctx_out;        /* the reconstructions' device-to-host copies (recon_file), behind the coding streams' fences */
    svt_hip_ctx     *ctx_deep;       /* opt-in: the deep-eligible waves of a group (12 of a mini-GOP's 16 pictures), which nothing of the NEXT group
                                        depends on -- its search and shallow waves run beside them instead of behind them */
    svt_hip_ctx     *ctx_me;         /* motion estimation + statistics of a group: the next group's search runs beside this group's layers */
    svt_hip_ctx     *ctx_key;        /* a key frame's intra encode pass (a dependency wavefront: ~6 ms at 4K on a fraction of the device), beside the
                                        search of the GOP's first group and the previous GOP's tail; the group's first wave waits for it (`key`) */
    svt_encdec_work *work, *work_deep, *work_key;
    shim_fence       in;             /* ctx_in: the latest picture's upload + analysis */
    shim_fence       key;            /* the latest intra picture (caller's thread; a planned group carries its copy) */
    int              ordinal;
    int              n_slots;
    shim_slot       *slot;
    int64_t          accepted;       /* pictures this device has taken: ring position */
    void            *d_src_slab, *d_pred_slab, *d_q_slab, *d_dq_slab;
    void            *d_ois;          /* intra_search: the open-loop intra search records of the key frame being decided (n_sb * SVT_OIS_PER_SB;
                                        written and read on the context of the intra pass, in stream order) */
    /* inter_mixed: the search records of the inter pictures being decided (a buffer per picture of the largest wave; the feeder has waited for a
       wave's counts before the next wave uses them) and the waves' intra-unit counts on the device and in pinned host memory */
    void            *d_ois_mixed[SHIM_WAVE_MAX];
    int              n_ois_mixed;
    void            *d_intra_units;
    int32_t         *h_intra_units;
    shim_recon      *free_recon;     /* pinned buffers ready for re-use */
    /* The device's feeder: a thread that enqueues the planned groups of this device (~2/3 of the stream operations of a picture) while the
       caller's thread goes on copying and uploading the next pictures.  One group per device at a time: the caller joins the previous one
       before it posts the next, and before anything else of its own that touches the device's main contexts or the group's slots. */
    struct shim_state *owner;
    pthread_t        feeder;
    int              has_feeder;
    pthread_mutex_t  mu;
    pthread_cond_t   cv;
    int              job_state;      /* 0 idle, 1 posted, 2 running (under mu) */
    int              stop;
    int              job_result;     /* EbErrorType of the last group (under mu) */
    int              outstanding;    /* caller's side: a group has been posted and not joined yet */
    shim_group       group;
} shim_dev;

typedef struct shim_state {
    EbSvtVp9EncConfiguration cfg;   /* the library's copy, with frame_rate / intra_period resolved (shim_resolve_config) */
    shim_options opt;
    int         configured, initialised, eos;
    int         failed;      /* written by the caller's thread and by the feeders: accessed through FAILED() / SET_FAILED() (relaxed atomics) */
    int         levels, minigop;       /* hierarchical levels, 1 << levels */
    int         intra_period;          /* resolved */
    int         n_dev, cur_dev;
    int         registry_held;         /* register_input: this encoder holds the process-wide page-lock registry until deinit */
    int         use_feeder;            /* per-device feeder threads (opt.feeder; off with a decision callback, one stream, split-GOP mode) */
    double      prof_s[8];
    shim_dev    dev[SHIM_MAX_DEV];
    int64_t     gop;                   /* index of the GOP being sent */
    int64_t     next_number;           /* display number of the next picture sent */
    int64_t     pending_first;         /* first picture of the mini-GOP being collected */
    int         pending;               /* pictures collected */
    int64_t     last_base;             /* display number of the latest base-layer / intra picture of the current GOP (-1: none yet) */
    shim_packet *q_head, *q_tail;
    shim_recon  *r_head, *r_tail;
    uint64_t    me_launches;           /* batched ME launches so far (svt_vp9_shim_get_counters) */
    /* geometry and per-stream constants of the stages behind mode decision */
    int         W, H, mi_rows, mi_cols, n_sb;
    size_t      pw, ph, cpw, cph;      /* a reference picture's padded planes: luma pw x ph, then two chroma planes of cpw x cph */
    size_t      pic_bytes, rec_bytes, coeffs;
    int         q_index, filter_level;
    uint32_t    md_lambda;
    svt_lf_thresh thr;
    svt_vp9_shim_md_callback md_cb;
    void       *md_user;
    void       *h_results, *h_mc, *h_lf;   /* host staging of the callback */
} shim_state;

#endif

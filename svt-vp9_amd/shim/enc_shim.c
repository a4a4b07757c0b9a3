/*
 * enc_shim.c -- libSvtVp9Enc.so: the reference's public encoder ABI (Source/API/EbSvtVp9Enc.h:365-439) in front of the GPU hot
 * path of this repository.  Plain C; the GPU is reached through the C ABI of libsvtvp9_hip.so only.  Beside it: shim_config.c (the
 * configuration rules), shim_plan.c (the structure of a group, pure), shim_internal.h (state, options, fences).
 *
 * What mirrors the reference, with the lines it follows:
 *   eb_vp9_svt_init_handle       handle malloc'd by the library, *config_ptr overwritten with the defaults
 *                                (Codec/EbEncHandle.c:1762-1852: eb_vp9_svt_enc_init_parameter; fields it does not touch stay untouched)
 *   eb_vp9_svt_enc_set_parameter copy + verify_settings' rules (:2052-2200, 2203-2557), hierarchical levels and automatic intra
 *                                period of set_param_based_on_input (:2166-2192)
 *   eb_vp9_svt_enc_send_picture  the picture is COPIED before the call returns (:2743-2796); NULL p_buffer / EOS flag ends the stream
 *   eb_vp9_svt_get_packet        non-blocking poll -> EB_NoErrorEmptyQueue when nothing is ready (:2880-2915); packets are the
 *                                library's until eb_vp9_svt_release_out_buffer (:1752-1757)
 *   eb_vp9_svt_get_recon         with recon_file: one reconstructed picture per call in coding order, pts = picture number, EOS on
 *                                the last (:2837-2865 <- recon_output, Codec/EbEncDecProcess.c:4693-4820); EB_ErrorMax without
 *   stream_header / eos_nal      no-ops returning EB_ErrorNone (:2953-2971)
 *
 * What the library does with the pictures (all of it enqueued asynchronously; send_picture returns after the host copy of the picture into
 * pinned staging; streams, fences, the group planner and the environment's switches: DESIGN.md section 7):
 *   as each picture arrives      three planes to the device (one staging copy, one transfer, on an UPLOAD context), picture analysis (padded /
 *                                decimated luma planes, block mean / variance) on an INPUT context behind it; a picture slot of the ring is
 *                                overwritten behind the fence of its last reader; get_recon's copies run on an OUTPUT context the same way
 *   intra pictures               the intra encode pass (svt_hip_encdec_intra_device) on a KEY context, beside the previous GOP's tail and the
 *                                new GOP's motion estimation; decided by the callback, else 16x16 / DC (or the open-loop intra search)
 *   when a mini-GOP is complete  (or cut short by an intra refresh / the end of the stream) the caller's thread plans the group (shim_plan.c;
 *                                packets queued in decode order) and the device's FEEDER thread enqueues it: ONE batched motion-estimation
 *                                launch for all its pictures + the per-SB ME statistics, then one batch per wave: mode decision (the host's
 *                                callback, the built-in stand-in, or the mixed stand-in that may hold intra leaves) -> inter prediction from
 *                                the reconstructed, padded references -> transform / quantisation / reconstruction -> skip flags ->
 *                                deblocking -> reference padding (svt_hip_encdec_batch_device), with the per-picture stage flags the
 *                                reference derives (svt_hip_encdec_flags_derive)
 *   GOPs                         closed GOPs are independent (Codec/EbPictureDecisionProcess.c:952): with SVT_HIP_DEVICES=0,1,.. GOP g is coded
 *                                on device g mod N, each with its own contexts and picture ring; with SVT_HIP_SPLIT_GOP=1
 *                                consecutive MINI-GOPs go to consecutive devices instead and the padded base-layer reconstruction (+ its
 *                                analysed planes) is handed on device to device (svt_hip_ref_handoff_device): the one exchange step
 * Every picture is answered by a zero-byte packet: entropy coding is outside the hot path.
 * Not reproduced (picture decision / rate control, control plane): the low-delay-P structure tables of the parts of a short group
 * (those pictures are a P chain); the q index of KEY frames -- inter pictures follow the reference's fixed-QP rule per temporal layer
 * (QP_SCALING_MODE_0, host/qp_scaling.c), key frames are coded at the sequence's q index where the reference applies its adaptive
 * QP_SCALING_MODE_1 to I slices (Codec/EbRateControlProcess.c:4680-4722: a noticeably lower q): pictures that predict from a key frame
 * see a coarser reference here than upstream.  Rate control's decision: out of scope.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "shim_internal.h"
#include "../csrc/encdec_core.h" /* svt_tq_unit_is_origin: the block rules the device-side driver applies to a mode-info grid */

#define FAILED(s) __atomic_load_n(&(s)->failed, __ATOMIC_RELAXED)
#define SET_FAILED(s) __atomic_store_n(&(s)->failed, 1, __ATOMIC_RELAXED)

/* host/copy_pool.c of libsvtvp9_hip.so: rows copied by a few threads (the staging copy of the uploads uses it too) */
void svt_copy_rows_mt(uint8_t *dst, size_t dst_stride, const uint8_t *src, size_t src_stride, size_t width, size_t rows);

static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
static shim_state *state_of(EbComponentType *h) { return h ? (shim_state *)h->p_component_private : NULL; }

/* a failed device call ends the stream: every later call reports it (the reference posts a pipeline error and answers EB_ErrorMax from
 * then on, :437-452, 2914-2917).  Reached from the caller's thread and from the feeders: it touches nothing but the flag. */
static EbErrorType gpu_fail(shim_state *s) {
    fprintf(stderr, "SvtVp9Enc (GPU hot path): %s\n", svt_hip_last_error());
    SET_FAILED(s);
    return EB_ErrorMax;
}
#define GPU_TRY(call) do { if ((call) != SVT_HIP_OK) return gpu_fail(s); } while (0)
/* an error that is not the device's, found after work of the group has been enqueued: the stream ends the same way (later calls
 * answer EB_ErrorMax) instead of going on with a group that is half processed */
static EbErrorType stream_fail(shim_state *s, const char *why) {
    fprintf(stderr, "SvtVp9Enc (GPU hot path): %s\n", why);
    SET_FAILED(s);
    return EB_ErrorBadParameter;
}

/* A mode-decision callback's grid, checked on the host before it is uploaded (the pipeline is drained at that point anyway): the
 * rules the device-side driver applies (svt_tq_unit_is_origin: sizes, transform not larger than the block, blocks aligned to their
 * size and inside the picture) and the intra pass's (csrc/intra_kernel.hip: square blocks of 4x4 .. 32x32 with the transform of
 * their own size, modes 0..9).  The device would only flag such a grid and SKIP the offending blocks -- their area would keep the
 * slot's previous picture and be used as a reference.  Returns 1 when the grid is malformed. */
static int grid_malformed(const shim_state *s, const svt_lf_mode_info *g, int intra_picture) {
    for (int ur = 0; ur < s->mi_rows; ur++)
        for (int uc = 0; uc < s->mi_cols; uc++) {
            const int o = svt_tq_unit_is_origin(g, s->mi_cols, s->mi_rows, s->mi_cols, ur, uc);
            if (o < 0) return 1;
            if (!o) continue;
            const svt_lf_mode_info *b = &g[ur * s->mi_cols + uc];
            if (b->is_inter) { if (intra_picture) return 1; continue; }
            const int sub = b->sb_type == 0, w8 = (b->sb_type == 3 || sub) ? 1 : b->sb_type == 6 ? 2 : b->sb_type == 9 ? 4 : 0;
            if (!w8 || b->tx_size != (sub ? 0 : w8 == 1 ? 1 : w8 == 2 ? 2 : 3) || b->pad_[2] > 9) return 1;
            if (sub) { const int m4 = (int)b->pad_[1] | (int)b->pad_[0] << 8; for (int q = 0; q < 4; q++) if (((m4 >> (4 * q)) & 15) > 9) return 1; }
            else if (b->pad_[1] > 9) return 1;
        }
    return 0;
}

/* ------------------------------------------------------------------------------------------------ */
EbErrorType eb_vp9_svt_init_handle(EbComponentType **p_handle, void *p_app_data, EbSvtVp9EncConfiguration *config_ptr) {
    if (!p_handle) return EB_ErrorBadParameter;
    *p_handle = (EbComponentType *)malloc(sizeof(EbComponentType));
    if (!*p_handle) return EB_ErrorInsufficientResources;
    shim_state *s = (shim_state *)calloc(1, sizeof *s);
    if (!s) { free(*p_handle); *p_handle = NULL; return EB_ErrorInsufficientResources; }
    (*p_handle)->n_size = sizeof(EbComponentType);
    (*p_handle)->p_component_private = s;
    (*p_handle)->p_application_private = p_app_data;
    s->last_base = -1;
    if (!config_ptr) return EB_ErrorBadParameter; /* as eb_vp9_svt_enc_init_parameter */
    shim_load_defaults(config_ptr);
    return EB_ErrorNone;
}

EbErrorType eb_vp9_svt_enc_set_parameter(EbComponentType *h, EbSvtVp9EncConfiguration *p) {
    shim_state *s = state_of(h);
    if (!s || !p) return EB_ErrorBadParameter;
    if (shim_resolve_config(p, &s->cfg, &s->levels) != EB_ErrorNone) return EB_ErrorBadParameter;
    s->minigop = 1 << s->levels;
    s->intra_period = s->cfg.intra_period;
    s->configured = 1;
    return EB_ErrorNone;
}

/* planes of a slot's tight source / prediction picture and of its padded reference picture */
static svt_yuv_planes tight_planes(const shim_state *s, uint8_t *base) {
    svt_yuv_planes p;
    p.y = base; p.u = base + (size_t)s->W * s->H; p.v = p.u + (size_t)(s->W / 2) * (s->H / 2);
    p.y_stride = s->W; p.uv_stride = s->W / 2; p.width = s->W; p.height = s->H;
    return p;
}
static svt_yuv_planes rec_planes(const shim_state *s, uint8_t *base) {
    svt_yuv_planes p;
    p.y = base + SHIM_REF_PAD * s->pw + SHIM_REF_PAD;
    p.u = base + s->pw * s->ph + (SHIM_REF_PAD / 2) * s->cpw + SHIM_REF_PAD / 2;
    p.v = base + s->pw * s->ph + s->cpw * s->cph + (SHIM_REF_PAD / 2) * s->cpw + SHIM_REF_PAD / 2;
    p.y_stride = (int32_t)s->pw; p.uv_stride = (int32_t)s->cpw; p.width = s->W; p.height = s->H;
    return p;
}

/* a picture's three planes through one staging slot, one copy to the device (Y | Cb | Cr are back to back there) */
static int32_t upload_tight(const shim_state *s, svt_hip_ctx *cx, uint8_t *d_dst, const void *y, const void *cb, const void *cr, size_t y_stride, size_t cb_stride, size_t cr_stride) {
    const svt_yuv_planes sp = tight_planes(s, d_dst);
    void *const       dd[3] = {sp.y, sp.u, sp.v};
    const void *const ss[3] = {y, cb, cr};
    const size_t      W = (size_t)s->W, H = (size_t)s->H, src_st[3] = {y_stride, cb_stride, cr_stride}, wb[3] = {W, W / 2, W / 2}, rows[3] = {H, H / 2, H / 2};
    return svt_hip_mem_upload_planes_async(cx, 3, dd, wb, ss, src_st, wb, rows);
}

static void feeder_stop(shim_dev *d);
static void feeder_start(shim_state *s, shim_dev *d);
static EbErrorType join_all(shim_state *s);

static void free_dev(shim_dev *d) {
    feeder_stop(d);
    if (!d->ctx) return;
    if (d->slot) {
        for (int i = 0; i < d->n_slots; i++) {
            shim_slot *t = &d->slot[i];
            void *v[15] = {(void *)t->pa.full.buf, (void *)t->pa.quarter.buf, (void *)t->pa.sixteenth.buf, t->d_rec, t->d_results, t->d_mean, t->d_var, t->d_rcme,
                           t->d_stats, t->d_hist, t->d_mc_mi, t->d_lf_mi, t->d_eob_map, t->d_lfm, t->d_nz};
            for (int k = 0; k < 15; k++) svt_hip_mem_free(d->ctx, v[k]);
        }
        free(d->slot);
    }
    void *v[6] = {d->d_src_slab, d->d_pred_slab, d->d_q_slab, d->d_dq_slab, d->d_ois, d->d_intra_units};
    for (int k = 0; k < 6; k++) svt_hip_mem_free(d->ctx, v[k]);
    for (int k = 0; k < SHIM_WAVE_MAX; k++) svt_hip_mem_free(d->ctx, d->d_ois_mixed[k]);
    if (d->h_intra_units) svt_hip_host_free(d->ctx, d->h_intra_units);
    while (d->free_recon) { shim_recon *r = d->free_recon; d->free_recon = r->next; svt_hip_host_free(d->ctx, r->host); svt_hip_mem_free(d->ctx, r->d_tight); free(r); }
    if (d->work_key && d->work_key != d->work) svt_hip_encdec_work_destroy(d->ctx_key, d->work_key);
    if (d->work) svt_hip_encdec_work_destroy(d->ctx, d->work);
    if (d->work_deep) svt_hip_encdec_work_destroy(d->ctx_deep, d->work_deep);
    svt_hip_ctx *side[6] = {d->ctx_key, d->ctx_deep, d->ctx_me, d->ctx_up == d->ctx_in ? NULL : d->ctx_up, d->ctx_in, d->ctx_out};
    for (int k = 0; k < 6; k++) if (side[k] && side[k] != d->ctx) svt_hip_ctx_destroy(side[k]);
    svt_hip_ctx_destroy(d->ctx);
    memset(d, 0, sizeof *d); /* (the feeder has stopped: nothing of the device is left) */
}

/* a reconstruction record with its pinned host buffer and its tight device buffer; NULL when one of them cannot be had */
static shim_recon *new_recon(const shim_state *s, shim_dev *d) {
    shim_recon *r = (shim_recon *)calloc(1, sizeof *r);
    void       *hp = NULL, *dp = NULL;
    if (!r || svt_hip_host_alloc(d->ctx_out, s->pic_bytes, &hp) != SVT_HIP_OK || svt_hip_mem_alloc(d->ctx_out, s->pic_bytes, &dp) != SVT_HIP_OK) {
        if (hp) svt_hip_host_free(d->ctx_out, hp);
        free(r);
        return NULL;
    }
    r->host = (uint8_t *)hp; r->d_tight = (uint8_t *)dp;
    return r;
}

static int alloc_dev(shim_state *s, shim_dev *d) {
    const int W = s->W, H = s->H;
    const int pad[3] = {68, 32, 16}; /* PA reference paddings, Codec/EbEncHandle.c:1003-1026 */
    /* the mini-GOP being collected, the ones whose work is in flight, and the base picture before them (ring_groups = 2: one in flight) */
    d->n_slots = s->opt.ring_groups * s->minigop + 2;
    d->slot = (shim_slot *)calloc((size_t)d->n_slots, sizeof(shim_slot));
    if (!d->slot) return 0;
    const size_t n = (size_t)d->n_slots, units = (size_t)s->mi_rows * s->mi_cols;
    int ok = svt_hip_mem_alloc(d->ctx, n * s->pic_bytes, &d->d_src_slab) == SVT_HIP_OK && svt_hip_mem_alloc(d->ctx, n * s->pic_bytes, &d->d_pred_slab) == SVT_HIP_OK &&
             svt_hip_mem_alloc(d->ctx, n * s->coeffs * sizeof(int16_t), &d->d_q_slab) == SVT_HIP_OK &&
             svt_hip_encdec_work_create(d->ctx, SHIM_WAVE_MAX, W, H, &d->work) == SVT_HIP_OK &&
             (d->ctx_deep == d->ctx || svt_hip_encdec_work_create(d->ctx_deep, SHIM_WAVE_MAX, W, H, &d->work_deep) == SVT_HIP_OK);
    if (ok && d->ctx_key != d->ctx) ok = svt_hip_encdec_work_create(d->ctx_key, 1, W, H, &d->work_key) == SVT_HIP_OK;
    else d->work_key = d->work;
    if (ok && s->opt.intra_search) ok = svt_hip_mem_alloc(d->ctx, (size_t)s->n_sb * SVT_OIS_PER_SB * sizeof(svt_ois_block), &d->d_ois) == SVT_HIP_OK;
    if (ok && s->opt.inter_mixed) { /* the largest wave of a mini-GOP is its deepest layer: half its pictures */
        d->n_ois_mixed = s->minigop / 2 < 1 ? 1 : s->minigop / 2 > SHIM_WAVE_MAX ? SHIM_WAVE_MAX : s->minigop / 2;
        for (int k = 0; ok && k < d->n_ois_mixed; k++)
            ok = svt_hip_mem_alloc(d->ctx, (size_t)s->n_sb * SVT_OIS_PER_SB * sizeof(svt_ois_block), &d->d_ois_mixed[k]) == SVT_HIP_OK;
        void *hp = NULL;
        ok = ok && svt_hip_mem_alloc(d->ctx, SHIM_WAVE_MAX * sizeof(int32_t), &d->d_intra_units) == SVT_HIP_OK &&
             svt_hip_host_alloc(d->ctx, SHIM_WAVE_MAX * sizeof(int32_t), &hp) == SVT_HIP_OK;
        d->h_intra_units = (int32_t *)hp;
    }
    for (int i = 0; ok && i < d->n_slots; i++) {
        shim_slot *t = &d->slot[i];
        t->number = -1;
        svt_plane *pl[3] = {&t->pa.full, &t->pa.quarter, &t->pa.sixteenth};
        for (int k = 0; ok && k < 3; k++) {
            const int w = W >> k, hh = H >> k;
            void *p = NULL;
            ok = svt_hip_mem_alloc(d->ctx, (size_t)(w + 2 * pad[k]) * (size_t)(hh + 2 * pad[k]), &p) == SVT_HIP_OK;
            pl[k]->buf = (const uint8_t *)p; pl[k]->stride = w + 2 * pad[k]; pl[k]->origin_x = pl[k]->origin_y = pad[k];
            pl[k]->width = w; pl[k]->height = hh;
        }
        t->d_src = (uint8_t *)d->d_src_slab + (size_t)i * s->pic_bytes;
        t->d_pred = (uint8_t *)d->d_pred_slab + (size_t)i * s->pic_bytes;
        t->d_qcoeff = (int16_t *)d->d_q_slab + (size_t)i * s->coeffs;
        t->d_dqcoeff = NULL; /* the encode pass keeps the dequantised coefficients in registers (svt_encdec_picture.d_dqcoeff) */
        void        *rec = NULL;
        void       **buf[12] = {&rec, &t->d_results, &t->d_mean, &t->d_var, &t->d_rcme, &t->d_stats, &t->d_hist, &t->d_mc_mi, &t->d_lf_mi, &t->d_eob_map, &t->d_lfm, &t->d_nz};
        const size_t bytes[12] = {s->rec_bytes, (size_t)s->n_sb * 85 * sizeof(svt_me_pu_result), (size_t)s->n_sb * 85, (size_t)s->n_sb * 85 * sizeof(uint16_t),
                                  (size_t)s->n_sb * sizeof(uint32_t), (size_t)s->n_sb * sizeof(svt_me_sb_stats), (2 * SVT_SAD_INTERVALS + 1) * sizeof(uint32_t),
                                  units * sizeof(svt_mc_mode_info), units * sizeof(svt_lf_mode_info), (size_t)(W / 4) * (H / 4) * 3 / 2 * sizeof(uint16_t),
                                  (size_t)s->n_sb * sizeof(svt_lf_mask), units};
        for (int k = 0; ok && k < 12; k++) ok = svt_hip_mem_alloc(d->ctx, bytes[k], buf[k]) == SVT_HIP_OK;
        t->d_rec = (uint8_t *)rec;
        t->info.n_sb = (uint32_t)s->n_sb;
    }
    if (ok) { /* take the context's pinned staging buffers now (init is outside the clock of SURVEY 8(d)'s metric, the first pictures are
                 not): one throw-away upload per buffer of the ring */
        uint8_t *z = (uint8_t *)calloc((size_t)W, (size_t)H);
        if (z) {
            for (int i = 0; i < 4; i++) (void)upload_tight(s, d->ctx_up, d->slot[0].d_src, z, z, z, (size_t)W, (size_t)W / 2, (size_t)W / 2); /* (a whole picture per buffer) */
            (void)svt_hip_ctx_synchronize(d->ctx_up);
            free(z);
        }
        /* ... and every stream's hardware queue (created by the runtime at the first submission) */
        svt_hip_ctx *all[7] = {d->ctx, d->ctx_in, d->ctx_up, d->ctx_out, d->ctx_key, d->ctx_deep, d->ctx_me};
        const int    scr[7] = {1024, 0, 0, 0, 1024, 256, 256}; /* private segments: the intra pass's kernel (key context; main context: intra blocks of inter pictures), the 32x32 transform */
        for (int i = 0; i < 7; i++) if (all[i]) (void)svt_hip_ctx_warm_scratch(all[i], scr[i]);
        /* ... and the deblocking launches' descriptor buffers at their largest (growing one waits for its stream: the first key frame's intra pass) */
        (void)svt_hip_lf_reserve(d->ctx, SHIM_WAVE_MAX, s->mi_rows, s->mi_cols);
        if (d->ctx_key && d->ctx_key != d->ctx) (void)svt_hip_lf_reserve(d->ctx_key, 1, s->mi_rows, s->mi_cols);
        if (d->ctx_deep && d->ctx_deep != d->ctx) (void)svt_hip_lf_reserve(d->ctx_deep, SHIM_WAVE_MAX, s->mi_rows, s->mi_cols);
        /* ... and, with reconstructed output, the reconstruction records of two groups: page-locking 12.4 MB per 4K picture inside the stream
           cost the first groups ~1 ms per picture (not an error when one cannot be had: the pool grows on demand, reserve_recon) */
        for (int k = 0; s->cfg.recon_file && k < 2 * s->minigop + 2; k++) {
            shim_recon *r = new_recon(s, d);
            if (!r) break;
            r->next = d->free_recon; d->free_recon = r;
        }
    }
    return ok;
}

/* The environment's switches, read here and nowhere else: one line per switch (DESIGN.md section 7 has the table). */
static EbErrorType read_options(shim_options *o) {
    const char *e;
    memset(o, 0, sizeof *o);
    /* target_socket names a CPU socket in the reference (-1 = both); here the GPUs come from SVT_HIP_DEVICES (a comma-separated list
       of ordinals: closed GOPs are dealt round-robin to them) or SVT_HIP_DEVICE (one ordinal, default 0) */
    if ((e = getenv("SVT_HIP_DEVICES")) && *e)
        for (const char *p = e; *p && o->n_dev < SHIM_MAX_DEV;) {
            o->ordinal[o->n_dev++] = atoi(p);
            while (*p && *p != ',') p++;
            if (*p == ',') p++;
        }
    e = getenv("SVT_HIP_DEVICE");
    if (o->n_dev == 0) { o->ordinal[0] = e ? atoi(e) : 0; o->n_dev = 1; }
    /* how intra / inter pictures that no callback decides are decided: per encoder (two encoders of a process may differ) */
    e = getenv("SVT_HIP_INTRA_DECISION");
    if (e && *e && strcmp(e, "dc")) {
        if (strcmp(e, "search")) { fprintf(stderr, "SvtVp9Enc: SVT_HIP_INTRA_DECISION=%s: expected \"dc\" or \"search\"\n", e); return EB_ErrorBadParameter; }
        o->intra_search = 1;
    }
    e = getenv("SVT_HIP_INTER_DECISION");
    if (e && *e && strcmp(e, "default")) {
        if (strcmp(e, "mixed")) { fprintf(stderr, "SvtVp9Enc: SVT_HIP_INTER_DECISION=%s: expected \"default\" or \"mixed\"\n", e); return EB_ErrorBadParameter; }
        o->inter_mixed = 1;
    }
    o->ring_groups = (e = getenv("SVT_HIP_RING_GROUPS")) ? atoi(e) : 4;
    o->ring_groups = o->ring_groups < 2 ? 2 : o->ring_groups > 8 ? 8 : o->ring_groups;
    o->single_stream = (e = getenv("SVT_HIP_SINGLE_STREAM")) && atoi(e) != 0;
    o->no_upload_stream = (e = getenv("SVT_HIP_NO_UPLOAD_STREAM")) && atoi(e) != 0;
    o->deep_stream = (e = getenv("SVT_HIP_DEEP_STREAM")) && atoi(e) != 0;
    o->me_stream = (e = getenv("SVT_HIP_ME_STREAM")) ? atoi(e) != 0 : -1;
    o->no_key_stream = (e = getenv("SVT_HIP_NO_KEY_STREAM")) && atoi(e) != 0;
    o->share_streams = !((e = getenv("SVT_HIP_SHARE_STREAMS")) && atoi(e) == 0);
    o->split_gop = o->n_dev > 1 && (e = getenv("SVT_HIP_SPLIT_GOP")) && atoi(e) != 0;
    o->register_input = (e = getenv("SVT_HIP_REGISTER_INPUT")) && atoi(e) != 0;
    o->feeder = (e = getenv("SVT_HIP_FEEDER")) ? atoi(e) != 0 : 1;
    if ((e = getenv("SVT_HIP_NO_FEEDER")) && atoi(e) != 0) o->feeder = 0;
    o->profile = (e = getenv("SVT_HIP_SHIM_PROFILE")) ? atoi(e) : 0;
    o->warmup = !((e = getenv("SVT_HIP_WARMUP")) && atoi(e) == 0);
    return EB_ErrorNone;
}

static void shim_deinit(shim_state *s);
static void shim_warm_up(const shim_state *real);

/* the streams of device i (which switch opens which, and what each cost or bought: DESIGN.md section 7).  They belong to the DEVICE: when an
   ordinal repeats in SVT_HIP_DEVICES the later context runs on the streams of the first one of that ordinal (share_streams) */
static int create_contexts(shim_state *s, int i) {
    const shim_options *o = &s->opt;
    shim_dev           *d = &s->dev[i];
    const shim_dev     *peer = NULL;
    const int           ord = o->ordinal[i];
    if (o->share_streams) for (int k = 0; k < i && !peer; k++) if (s->dev[k].ordinal == ord) peer = &s->dev[k];
#define DEV_CTX_CREATE(field) (((peer && peer->field) ? svt_hip_ctx_create_on_stream(&d->field, ord, svt_hip_ctx_stream(peer->field)) : svt_hip_ctx_create(&d->field, ord)) == SVT_HIP_OK || (d->field = NULL, 0))
    if (!DEV_CTX_CREATE(ctx)) { fprintf(stderr, "SvtVp9Enc (GPU hot path): %s\n", svt_hip_last_error()); return 0; }
    d->ctx_in = d->ctx_out = d->ctx_up = d->ctx_deep = d->ctx_me = d->ctx_key = d->ctx;
    if (o->single_stream) return 1;
    if (!DEV_CTX_CREATE(ctx_in)) return 0;
    if (o->no_upload_stream) d->ctx_up = d->ctx_in;
    else if (!DEV_CTX_CREATE(ctx_up)) return 0;
    if (s->cfg.recon_file && !DEV_CTX_CREATE(ctx_out)) return 0; /* (no reconstruction is fetched: no output stream) */
    if (o->deep_stream && !DEV_CTX_CREATE(ctx_deep)) return 0;
    if ((o->me_stream < 0 ? !s->cfg.recon_file : o->me_stream) && !s->md_cb && !DEV_CTX_CREATE(ctx_me)) return 0;
    if (!o->no_key_stream && !s->md_cb && !DEV_CTX_CREATE(ctx_key)) return 0;
#undef DEV_CTX_CREATE
    return 1;
}

static EbErrorType shim_init(shim_state *s, const shim_options *opt) {
    s->opt = *opt;
    s->W = (int)s->cfg.source_width; s->H = (int)s->cfg.source_height;
    s->mi_rows = s->H >> 3; s->mi_cols = s->W >> 3;
    s->n_sb = svt_hip_sb_count(s->W, s->H);
    s->pic_bytes = (size_t)s->W * s->H * 3 / 2;
    s->pw = (size_t)s->W + 2 * SHIM_REF_PAD; s->ph = (size_t)s->H + 2 * SHIM_REF_PAD;
    s->cpw = (size_t)s->W / 2 + SHIM_REF_PAD; s->cph = (size_t)s->H / 2 + SHIM_REF_PAD;
    s->rec_bytes = (s->pw * s->ph + 2 * s->cpw * s->cph + 63) / 64 * 64;
    s->coeffs = (size_t)s->n_sb * SVT_SB_COEFFS;
    /* fixed QP: quantizer_to_qindex[qp] for every picture (the per-layer QP scaling is rate control's, Codec/EbRateControlProcess.c:4581-4735) */
    s->q_index = svt_hip_vp9_qindex_from_qp((int32_t)s->cfg.qp);
    s->filter_level = s->cfg.loop_filter ? svt_hip_lf_level_from_q(svt_hip_vp9_ac_step(s->q_index), 0) : 0;
    s->md_lambda = 4u * (uint32_t)svt_hip_vp9_ac_step(s->q_index);
    svt_hip_lf_thresh_init(&s->thr, 0);
    for (int i = 0; i < opt->n_dev; i++) {
        shim_dev *d = &s->dev[i];
        memset(d, 0, sizeof *d);
        d->ordinal = opt->ordinal[i];
        if (!create_contexts(s, i) || !alloc_dev(s, d)) { /* nothing half-initialised is left behind: the handle is back in its configured state */
            for (int k = i; k >= 0; k--) free_dev(&s->dev[k]); /* (reverse: a later context may run on an earlier one's streams) */
            return EB_ErrorInsufficientResources;
        }
    }
    s->n_dev = opt->n_dev;
    s->cur_dev = 0;
    if (opt->register_input) { svt_hip_host_registry_retain(); s->registry_held = 1; } /* released at deinit: the last encoder out unlocks the application's buffers */
    s->use_feeder = opt->feeder && !opt->single_stream && !s->md_cb && !opt->split_gop;
    memset(s->prof_s, 0, sizeof s->prof_s);
    for (int i = 0; i < s->n_dev; i++) feeder_start(s, &s->dev[i]);
    if (s->md_cb) {
        s->h_results = malloc((size_t)s->n_sb * 85 * sizeof(svt_me_pu_result));
        s->h_mc = malloc((size_t)s->mi_rows * s->mi_cols * sizeof(svt_mc_mode_info));
        s->h_lf = malloc((size_t)s->mi_rows * s->mi_cols * sizeof(svt_lf_mode_info));
        if (!s->h_results || !s->h_mc || !s->h_lf) { shim_deinit(s); return EB_ErrorInsufficientResources; }
    }
    s->initialised = 1;
    if (opt->warmup && !s->md_cb) shim_warm_up(s);
    return EB_ErrorNone;
}

EbErrorType eb_vp9_init_encoder(EbComponentType *h) {
    shim_state *s = state_of(h);
    if (!s || !s->configured) return EB_ErrorBadParameter;
    if (s->initialised) return EB_ErrorNone;
    shim_options opt;
    const EbErrorType e = read_options(&opt);
    return e != EB_ErrorNone ? e : shim_init(s, &opt);
}

/* Initialisation is outside the clock of SURVEY 8(d)'s metric (first send_picture -> EOS packet), the first pictures are not: the HIP runtime loads
 * a code object the first time one of its kernels is launched, and the first key frame / first group paid for that inside the stream (~8 ms of a
 * 130-picture run at 4K).  A throw-away encoder of the same preset and the same options on a small picture runs one closed GOP's first pictures
 * here -- every kernel of the path has been launched once when the real stream starts.  It warms nothing up itself and uploads through the staging
 * path: its private picture is never page-locked. */
static void shim_warm_up(const shim_state *real) {
    EbComponentType          *h = NULL;
    EbSvtVp9EncConfiguration  cfg;
    shim_options              opt = real->opt;
    const uint32_t            W = 256, H = 192;
    const int                 n = 1 + 2 * 16; /* a key frame and two mini-GOPs */
    uint8_t                  *pic = (uint8_t *)calloc((size_t)W * H * 3 / 2, 1), *rbuf = (uint8_t *)malloc((size_t)W * H * 3 / 2);
    opt.warmup = 0; opt.register_input = 0;
    if (pic && rbuf && eb_vp9_svt_init_handle(&h, NULL, &cfg) == EB_ErrorNone) {
        cfg = real->cfg;
        cfg.source_width = W; cfg.source_height = H;
        if (eb_vp9_svt_enc_set_parameter(h, &cfg) == EB_ErrorNone && shim_init(state_of(h), &opt) == EB_ErrorNone) {
            int eos = 0, recon_eos = !cfg.recon_file, guard = 0;
            for (int i = 0; i < n || !(eos && recon_eos); i++) {
                if (i < n) {
                    EbSvtEncInput      in;
                    EbBufferHeaderType b;
                    memset(&in, 0, sizeof in); memset(&b, 0, sizeof b);
                    in.luma = pic; in.cb = pic + (size_t)W * H; in.cr = in.cb + (size_t)W * H / 4;
                    in.y_stride = W; in.cb_stride = in.cr_stride = W / 2;
                    b.size = sizeof b; b.p_buffer = (uint8_t *)&in; b.n_filled_len = W * H * 3 / 2; b.pts = i;
                    b.flags = i == n - 1 ? EB_BUFFERFLAG_EOS : 0;
                    if (eb_vp9_svt_enc_send_picture(h, &b) != EB_ErrorNone) break;
                } else if (++guard > 100000) break;
                for (;;) {
                    EbBufferHeaderType *pk = NULL;
                    if (eb_vp9_svt_get_packet(h, &pk, (uint8_t)(i >= n - 1)) != EB_ErrorNone || !pk) break;
                    eos |= (pk->flags & EB_BUFFERFLAG_EOS) != 0;
                    eb_vp9_svt_release_out_buffer(&pk);
                }
                while (!recon_eos) {
                    EbBufferHeaderType r;
                    memset(&r, 0, sizeof r);
                    r.size = sizeof r; r.p_buffer = rbuf; r.n_alloc_len = W * H * 3 / 2;
                    if (eb_vp9_svt_get_recon(h, &r) != EB_ErrorNone) break;
                    recon_eos = (r.flags & EB_BUFFERFLAG_EOS) != 0;
                }
            }
        }
        (void)eb_vp9_deinit_handle(h);
    }
    free(pic); free(rbuf);
}

EbErrorType eb_vp9_svt_enc_stream_header(EbComponentType *h, EbBufferHeaderType **o) { (void)h; (void)o; return EB_ErrorNone; }
EbErrorType eb_vp9_svt_enc_eos_nal(EbComponentType *h, EbBufferHeaderType **o) { (void)h; (void)o; return EB_ErrorNone; }

/* ------------------------------------------------------------------------------------------------ */
static shim_slot *find_slot(shim_dev *d, int64_t number) {
    for (int i = 0; i < d->n_slots; i++) if (d->slot[i].number == number) return &d->slot[i];
    return NULL;
}
static shim_slot *find_any(shim_state *s, int64_t number, shim_dev **dev) { /* the picture where it was coded, not a handed-over copy */
    for (int k = 0; k < s->n_dev; k++)
        for (int i = 0; i < s->dev[k].n_slots; i++) {
            shim_slot *t = &s->dev[k].slot[i];
            if (t->number == number && !t->is_copy) { if (dev) *dev = &s->dev[k]; return t; }
        }
    return NULL;
}

/* split-GOP mode: the next mini-GOP is coded on device `to`; it predicts from the base picture the current device has just
 * finished -- its analysed planes (motion estimation) and its padded reconstruction (inter prediction) travel device to device,
 * ordered behind the producer's work and in front of the consumer's (svt_hip_ref_handoff_device) */
static EbErrorType handoff_base(shim_state *s, shim_dev *from, shim_dev *to, int64_t number) {
    shim_slot *a = find_slot(from, number);
    if (!a) return EB_ErrorBadParameter;
    shim_slot *b = &to->slot[to->accepted % to->n_slots];
    GPU_TRY(fence_wait_host(&b->done));
    GPU_TRY(fence_wait_host(&b->free_deep));
    fence_clear(&b->free_deep);
    GPU_TRY(fence_order(to->ctx, &b->out)); /* its old reconstruction may still be on its way out */
    fence_clear(&b->out);
    const svt_plane *pa[3] = {&a->pa.full, &a->pa.quarter, &a->pa.sixteenth}, *pb[3] = {&b->pa.full, &b->pa.quarter, &b->pa.sixteenth};
    for (int k = 0; k < 3; k++)
        GPU_TRY(svt_hip_ref_handoff_device(from->ctx, pa[k]->buf, to->ctx, (void *)pb[k]->buf, (size_t)pa[k]->stride * (size_t)(pa[k]->height + 2 * pa[k]->origin_y)));
    GPU_TRY(svt_hip_ref_handoff_device(from->ctx, a->d_rec, to->ctx, b->d_rec, s->rec_bytes));
    to->accepted++;
    b->number = number; b->pts = a->pts; b->info = a->info; b->processed = 1; b->coded = 1; b->is_copy = 1;
    GPU_TRY(fence_record(to->ctx, &b->done));
    b->free_main = b->done;
    return EB_ErrorNone;
}

/* a packet joins the queue (caller's thread only); done = the fence of its work when that is known already (else the group's feeder
 * completes it) */
static shim_packet *queue_packet(shim_state *s, int64_t pts, uint32_t flags, uint32_t pic_type, int dev, const shim_fence *done) {
    shim_packet *p = (shim_packet *)calloc(1, sizeof *p);
    if (!p) return NULL;
    p->hdr.size = sizeof(EbBufferHeaderType);
    p->hdr.pts = p->hdr.dts = pts;
    p->hdr.flags = flags;
    p->hdr.pic_type = pic_type;
    p->hdr.wrapper_ptr = p; /* the round trip of the reference's wrapper_ptr (:2923) */
    p->dev = dev;
    if (done) { p->done = *done; p->ready = 1; }
    if (s->q_tail) s->q_tail->next = p; else s->q_head = p;
    s->q_tail = p;
    return p;
}

/* the reconstruction of a picture on its way to eb_vp9_svt_get_recon: W x H luma, then Cb, then Cr (recon_output,
 * Codec/EbEncDecProcess.c:4693-4820), copied to pinned host memory behind the picture's last stage.
 * Caller's thread: a record with a pinned buffer joins the reconstruction queue, in coding order; fill_recon completes it */
static shim_recon *reserve_recon(shim_state *s, shim_dev *d, int64_t number) {
    shim_recon *r = d->free_recon;
    if (r) d->free_recon = r->next;
    else if (!(r = new_recon(s, d))) { (void)gpu_fail(s); return NULL; }
    r->dev = (int)(d - s->dev); r->pts = number; r->flags = 0; r->next = NULL; r->ready = 0; fence_clear(&r->done);
    if (s->r_tail) s->r_tail->next = r; else s->r_head = r;
    s->r_tail = r;
    return r;
}
/* enqueuing thread: the copies of picture t into the reserved record */
static EbErrorType fill_recon(shim_state *s, shim_dev *d, shim_slot *t, svt_hip_ctx *coded_on, shim_recon *r) {
    const svt_yuv_planes p = rec_planes(s, t->d_rec);
    const size_t W = (size_t)s->W, H = (size_t)s->H;
    /* the copy runs on the output stream, behind the coding stream's work enqueued so far (the picture's deblocking / padding) */
    shim_fence after = {0};
    if ((d->ctx_out != coded_on && (fence_record(coded_on, &after) != SVT_HIP_OK || fence_order(d->ctx_out, &after) != SVT_HIP_OK)) ||
        /* the interiors of the three padded planes are packed on the device and cross the link as ONE linear transfer (strided device-to-host
           copies ran at a third of the link's rate, profiles/r06_api.txt) */
        svt_hip_mem_copy_2d_device(d->ctx_out, r->d_tight, W, p.y, (size_t)p.y_stride, W, H) != SVT_HIP_OK ||
        svt_hip_mem_copy_2d_device(d->ctx_out, r->d_tight + W * H, W / 2, p.u, (size_t)p.uv_stride, W / 2, H / 2) != SVT_HIP_OK ||
        svt_hip_mem_copy_2d_device(d->ctx_out, r->d_tight + W * H + W * H / 4, W / 2, p.v, (size_t)p.uv_stride, W / 2, H / 2) != SVT_HIP_OK ||
        svt_hip_mem_download_2d_async(d->ctx_out, r->host, s->pic_bytes, r->d_tight, s->pic_bytes, s->pic_bytes, 1) != SVT_HIP_OK ||
        fence_record(d->ctx_out, &r->done) != SVT_HIP_OK)
        return gpu_fail(s); /* (the record stays in the queue, never ready: the stream has failed) */
    t->out = r->done;
    __atomic_store_n(&r->ready, 1, __ATOMIC_RELEASE);
    return EB_ErrorNone;
}

/* the parameters motion_estimate_sb reads for this picture, as the reference derives them */
static EbErrorType job_params(shim_state *s, const shim_plan_pic *j, svt_me_params *p) {
    svt_me_picture_config pc;
    memset(&pc, 0, sizeof pc);
    pc.pic_width = (int32_t)s->cfg.source_width; pc.pic_height = (int32_t)s->cfg.source_height;
    pc.enc_mode = s->cfg.enc_mode; pc.tune = s->cfg.tune;
    /* static_config.frame_rate >> 16, the value the reference's 4K HME widening tests (Codec/EbMotionEstimationProcess.c:55-324) */
    pc.frame_rate = (int32_t)(s->cfg.frame_rate >> 16);
    pc.num_ref_lists = j->n_lists; pc.temporal_layer_index = j->layer; pc.hierarchical_levels = j->levels;
    pc.is_used_as_reference = j->used_as_ref;
    pc.same_ref_poc = j->n_lists == 2 && j->ref0 == j->ref1;
    pc.rate_control_mode = (int32_t)s->cfg.rate_control_mode;
    if (svt_hip_me_params_derive(p, &pc) != SVT_HIP_OK) return EB_ErrorBadParameter;
    if (!s->cfg.use_default_me_hme) { /* eb_vp9_set_me_hme_params_from_config (Codec/EbMotionEstimationProcess.c:316-324) */
        /* verify_settings accepts 1..256 and the reference keeps the value in a uint8_t (256 wraps to 0 there: a configuration
           it cannot run); here the search area is clamped to what the kernel's record holds */
        const uint32_t w = s->cfg.search_area_width, hh = s->cfg.search_area_height;
        p->search_area_width  = (uint8_t)(w > 255 ? 255 : w < 1 ? 1 : w);
        p->search_area_height = (uint8_t)(hh > 255 ? 255 : hh < 1 ? 1 : hh);
        p->enable_hme_flag    = s->cfg.enable_hme_flag;
    }
    return EB_ErrorNone;
}

/* ---- what the inter waves and the intra pass share ---- */
static EbErrorType derive_flags(const shim_state *s, int layer, int used_as_ref, svt_encdec_flags *fl) {
    svt_encdec_flags_config fc;
    fc.enc_mode = s->cfg.enc_mode; fc.tune = s->cfg.tune; fc.temporal_layer_index = layer; fc.is_used_as_reference = used_as_ref;
    fc.recon_file = (int32_t)s->cfg.recon_file; fc.loop_filter = s->cfg.loop_filter;
    return svt_hip_encdec_flags_derive(&fc, fl) == SVT_HIP_OK ? EB_ErrorNone : EB_ErrorBadParameter;
}
/* the slot's own buffers as the encode pass takes them (an inter picture adds its motion grid, references and sub-pel rule) */
static void slot_picture(const shim_state *s, const shim_slot *t, svt_encdec_picture *p) {
    memset(p, 0, sizeof *p);
    p->d_lf_mi = (svt_lf_mode_info *)t->d_lf_mi;
    p->src = tight_planes(s, t->d_src); p->pred = tight_planes(s, t->d_pred); p->recon = rec_planes(s, t->d_rec);
    p->d_qcoeff = t->d_qcoeff; p->d_dqcoeff = t->d_dqcoeff; p->d_eob_map = (uint16_t *)t->d_eob_map; p->d_lfm = (svt_lf_mask *)t->d_lfm; p->d_nz = (uint8_t *)t->d_nz;
}
static void info_flags(shim_slot *t, int used_as_ref, const svt_encdec_flags *fl, int q_index, int level) {
    t->info.is_used_as_reference = used_as_ref; t->info.do_recon = fl->do_recon; t->info.apply_loop_filter = fl->apply_loop_filter;
    t->info.pad_reference = fl->pad_reference; t->info.q_index = q_index; t->info.filter_level = level; t->info.intra_recon_is_source = 0;
}
static int32_t upload_grid(const shim_state *s, svt_hip_ctx *cx, void *d_dst, const void *h_src, size_t elem) {
    return svt_hip_mem_upload_2d(cx, d_dst, (size_t)s->mi_cols * elem, h_src, (size_t)s->mi_cols * elem, (size_t)s->mi_cols * elem, (size_t)s->mi_rows);
}
/* the host's decision for picture t (the pipeline is drained at this point): *decided = 1 when the callback took the picture and its
 * grids are on the device.  h_results: the picture's ME results, NULL for an intra picture (which has no motion grid either). */
static EbErrorType ask_callback(shim_state *s, svt_hip_ctx *cx, shim_slot *t, const void *h_results, int *decided) {
    const int intra = !h_results;
    *decided = 0;
    memset(s->h_mc, 0, (size_t)s->mi_rows * s->mi_cols * sizeof(svt_mc_mode_info));
    memset(s->h_lf, 0, (size_t)s->mi_rows * s->mi_cols * sizeof(svt_lf_mode_info));
    if (s->md_cb(s->md_user, &t->info, h_results, s->h_mc, s->h_lf, s->mi_cols) != 0) return EB_ErrorNone;
    if (grid_malformed(s, (const svt_lf_mode_info *)s->h_lf, intra))
        return stream_fail(s, intra ? "mode-decision callback: malformed mode-info grid of an intra picture" : "mode-decision callback: malformed mode-info grid");
    if (!intra) GPU_TRY(upload_grid(s, cx, t->d_mc_mi, s->h_mc, sizeof(svt_mc_mode_info)));
    GPU_TRY(upload_grid(s, cx, t->d_lf_mi, s->h_lf, sizeof(svt_lf_mode_info)));
    t->info.decision_source = 1;
    *decided = 1;
    return EB_ErrorNone;
}

/* The stages behind mode decision for one batch of mutually independent pictures (a wave of the plan, or a part of one): decision ->
 * svt_hip_encdec_batch_device -> reconstruction output.  idx: the pictures' positions in the group's plan. */
static EbErrorType encode_wave(shim_state *s, shim_dev *d, const shim_group *G, const int *idx, int n, int deep) {
    svt_hip_ctx     *cx = deep ? d->ctx_deep : d->ctx;       /* the context (stream) this wave is enqueued on, and its driver workspace */
    svt_encdec_work *wk = deep ? d->work_deep : d->work;
    const shim_plan_pic *first = &G->plan.pic[idx[0]];
    svt_encdec_picture pics[SHIM_WAVE_MAX];
    shim_slot         *ts[SHIM_WAVE_MAX];
    svt_encdec_flags   fl;
    if (derive_flags(s, first->layer, first->used_as_ref, &fl) != EB_ErrorNone) return EB_ErrorBadParameter;
    /* fixed-QP mode: the wave's temporal layer scales the sequence QP (QP_SCALING_MODE_0 of the reference's rate-control kernel,
       svt_hip_vp9_layer_qindex); the deblocking level and the stand-in decision's lambda follow the picture's q index */
    const int      q_l = s->cfg.rate_control_mode == 0 ? svt_hip_vp9_layer_qindex((int32_t)s->cfg.qp, s->cfg.tune, first->levels, first->layer, 0) : s->q_index;
    const int      level_l = s->cfg.loop_filter ? svt_hip_lf_level_from_q(svt_hip_vp9_ac_step(q_l), 0) : 0;
    const uint32_t lambda_l = 4u * (uint32_t)svt_hip_vp9_ac_step(q_l);
    int n_stand_in = 0;
    int has_intra[SHIM_WAVE_MAX] = {0};
    int stand_in_pic[SHIM_WAVE_MAX]; /* picture of the wave behind the k-th stand-in decision */
    const svt_me_pu_result *res[SHIM_WAVE_MAX];
    svt_mc_mode_info       *mcs[SHIM_WAVE_MAX];
    svt_lf_mode_info       *lfs[SHIM_WAVE_MAX];
    for (int i = 0; i < n; i++) {
        const shim_plan_pic *j = &G->plan.pic[idx[i]];
        shim_slot *t = ts[i] = find_slot(d, j->number);
        shim_slot *r0 = find_slot(d, j->ref0), *r1 = j->n_lists == 2 ? find_slot(d, j->ref1) : r0;
        if (!t || !r0 || !r1) return stream_fail(s, "a picture of the group or one of its references is not resident");
        int decided = 0;
        t->info.decision_source = 0;
        t->info.q_index = q_l; t->info.filter_level = level_l; /* (the callback reads them: the level goes into its grid) */
        if (s->md_cb) { /* the host decides: it needs the ME results, so the pipeline drains here */
            GPU_TRY(svt_hip_mem_download(d->ctx, s->h_results, t->d_results, (size_t)s->n_sb * 85 * sizeof(svt_me_pu_result)));
            const EbErrorType e = ask_callback(s, d->ctx, t, s->h_results, &decided);
            if (e != EB_ErrorNone) return e;
            /* a host decision may hold intra blocks: they go through the intra pass behind the batch */
            const svt_lf_mode_info *g = (const svt_lf_mode_info *)s->h_lf;
            for (size_t u = 0; decided && u < (size_t)s->mi_rows * s->mi_cols && !has_intra[i]; u++) has_intra[i] = !g[u].is_inter;
        }
        if (!decided) {
            res[n_stand_in] = (const svt_me_pu_result *)t->d_results; mcs[n_stand_in] = (svt_mc_mode_info *)t->d_mc_mi; lfs[n_stand_in] = (svt_lf_mode_info *)t->d_lf_mi;
            stand_in_pic[n_stand_in++] = i;
            if (s->opt.inter_mixed) t->info.decision_source = 3;
        }
        svt_encdec_picture *p = &pics[i];
        slot_picture(s, t, p);
        p->d_mc_mi = (const svt_mc_mode_info *)t->d_mc_mi;
        p->ref[0] = rec_planes(s, r0->d_rec); p->ref[1] = rec_planes(s, r1->d_rec);
        /* pred_struct use_subpel_flag of the picture, as the encode pass reads it for its inter prediction (Codec/EbEncDecProcess.c:5507):
           the ME parameter derivation encodes it as "fractional search off" */
        p->use_subpel = G->me[idx[i]].fractional_search_model != 2;
        p->has_intra = has_intra[i];
        info_flags(t, j->used_as_ref, &fl, q_l, level_l);
    }
    if (n_stand_in && s->opt.inter_mixed) {
        /* the mixed stand-in: the open-loop intra search of the pictures' device-resident sources (no 4x4 phase: the rule makes no 4x4 unit),
           then the decision, in sub-batches of the search buffers; the counts of intra units cross to pinned memory and the feeder waits
           for them here -- has_intra selects the intra wavefront kernel behind the batch's transform stage.  intra_penalty = 2 lambda is an
           untuned stand-in value (an intra leaf pays for its modes instead of its vectors), like the rule itself */
        for (int b = 0; b < n_stand_in; b += d->n_ois_mixed) {
            const int            m = n_stand_in - b < d->n_ois_mixed ? n_stand_in - b : d->n_ois_mixed;
            svt_yuv_planes       srcs[SHIM_WAVE_MAX];
            svt_ois_block       *outs[SHIM_WAVE_MAX];
            svt_md_mixed_picture mp[SHIM_WAVE_MAX];
            for (int k = 0; k < m; k++) {
                srcs[k] = pics[stand_in_pic[b + k]].src;
                outs[k] = (svt_ois_block *)d->d_ois_mixed[k];
                mp[k].d_results = res[b + k]; mp[k].d_ois = outs[k]; mp[k].d_mc_mi = mcs[b + k]; mp[k].d_lf_mi = lfs[b + k];
            }
            GPU_TRY(svt_hip_intra_search_batch_device(cx, m, srcs, s->W, s->H, 0, outs));
            GPU_TRY(svt_hip_md_mixed_batch_device(cx, m, mp, s->W, s->H, lambda_l, 2u * lambda_l, level_l, s->mi_cols, (int32_t *)d->d_intra_units));
            shim_fence counts;
            GPU_TRY(svt_hip_mem_download_2d_async(cx, d->h_intra_units, (size_t)m * sizeof(int32_t), d->d_intra_units, (size_t)m * sizeof(int32_t),
                                                  (size_t)m * sizeof(int32_t), 1));
            GPU_TRY(fence_record(cx, &counts));
            GPU_TRY(fence_wait_host(&counts));
            for (int k = 0; k < m; k++) {
                const int i = stand_in_pic[b + k];
                has_intra[i] = d->h_intra_units[k] > 0;
                pics[i].has_intra = has_intra[i];
            }
        }
    }
    {   /* intra blocks need their neighbours' reconstruction: a wave that would not be reconstructed (the deepest layer without
           reconstructed output) is, when a host decision put intra blocks into it -- the reference reconstructs the SBs that hold them
           (is_intra_sb, Codec/EbEncDecProcess.c:3653-3657); the other flags of the wave stay */
        int any_intra = 0;
        for (int i = 0; i < n; i++) any_intra |= has_intra[i];
        if (any_intra && !fl.do_recon) {
            fl.do_recon = 1;
            for (int i = 0; i < n; i++) ts[i]->info.do_recon = 1;
        }
    }
    if (n_stand_in && !s->opt.inter_mixed)
        GPU_TRY(svt_hip_md_default_batch_device(cx, n_stand_in, res, s->W, s->H, lambda_l, level_l, mcs, lfs, s->mi_cols));
    GPU_TRY(svt_hip_encdec_batch_device(cx, wk, n, pics, s->W, s->H, s->mi_cols, q_l, &fl, &s->thr, SHIM_REF_PAD, SHIM_REF_PAD));
    for (int i = 0; i < n; i++) {
        ts[i]->coded = 1;
        if (s->cfg.recon_file) {
            if (!G->rec[idx[i]]) return stream_fail(s, "reconstruction record");
            const EbErrorType e = fill_recon(s, d, ts[i], cx, G->rec[idx[i]]);
            if (e != EB_ErrorNone) return e;
        }
    }
    return EB_ErrorNone;
}

/* an intra picture (key frame / intra refresh): the intra encode pass on the GPU (svt_hip_encdec_intra_device: reference samples,
 * predictors, transform / quantisation / reconstruction in coding-dependency order, then deblocking and border).  The host's callback
 * decides its blocks and modes when it wants to (info->is_intra = 1, no ME results); otherwise the stand-in: 16x16 DC, or with
 * SVT_HIP_INTRA_DECISION=search the open-loop intra search and the grid built from its records (decision_source 2). */
static EbErrorType encode_intra(shim_state *s, shim_dev *d, shim_slot *t) {
    svt_encdec_flags fl;
    svt_hip_ctx *cx = d->ctx_key; /* (the main context without a key stream) */
    GPU_TRY(fence_order(cx, &d->in)); /* the picture has been uploaded and analysed */
    if (derive_flags(s, 0, 1, &fl) != EB_ErrorNone) return EB_ErrorBadParameter;
    const int level = s->cfg.loop_filter ? svt_hip_lf_level_from_q(svt_hip_vp9_ac_step(s->q_index), 1) : 0; /* key-frame rule of eb_vp9_pick_filter_level */
    info_flags(t, 1, &fl, s->q_index, level);
    t->info.decision_source = 0;
    int decided = 0;
    if (s->md_cb) {
        const EbErrorType e = ask_callback(s, cx, t, NULL, &decided);
        if (e != EB_ErrorNone) return e;
    }
    const double tk0 = s->opt.profile > 1 ? now_s() : 0.0;
    if (!decided && s->opt.intra_search) {
        const svt_yuv_planes src = tight_planes(s, t->d_src);
        GPU_TRY(svt_hip_intra_search_device(cx, &src, s->W, s->H, (svt_ois_block *)d->d_ois));
        GPU_TRY(svt_hip_md_intra_search_device(cx, (const svt_ois_block *)d->d_ois, s->W, s->H, s->md_lambda, level, (svt_lf_mode_info *)t->d_lf_mi, s->mi_cols));
        t->info.decision_source = 2;
    } else if (!decided) GPU_TRY(svt_hip_md_intra_default_device(cx, s->W, s->H, level, (svt_lf_mode_info *)t->d_lf_mi, s->mi_cols));
    const double tk1 = s->opt.profile > 1 ? now_s() : 0.0;
    GPU_TRY(svt_hip_mem_set(cx, t->d_mc_mi, 0, (size_t)s->mi_rows * s->mi_cols * sizeof(svt_mc_mode_info))); /* no motion in an intra picture */
    const double tk2 = s->opt.profile > 1 ? now_s() : 0.0;
    svt_encdec_picture p;
    slot_picture(s, t, &p);
    GPU_TRY(svt_hip_encdec_intra_device(cx, d->work_key, &p, s->W, s->H, s->mi_cols, s->q_index, &fl, &s->thr, SHIM_REF_PAD, SHIM_REF_PAD));
    if (s->opt.profile > 1) fprintf(stderr, "SvtVp9Enc key frame %lld: decision %.1f  memset %.1f  intra pass %.1f us\n", (long long)t->number, 1e6 * (tk1 - tk0), 1e6 * (tk2 - tk1), 1e6 * (now_s() - tk2));
    t->coded = 1;
    if (s->cfg.recon_file) {
        shim_recon *r = reserve_recon(s, d, t->number);
        if (!r) return FAILED(s) ? EB_ErrorMax : EB_ErrorInsufficientResources;
        return fill_recon(s, d, t, cx, r);
    }
    return EB_ErrorNone;
}

/* The collected group on the current GOP's device: all its pictures go to the GPU's motion estimation in as few launches as their
 * parameter sets allow (one for a regular mini-GOP), followed by the per-SB statistics of every picture and by the stages behind mode
 * decision, one batch per wave of the plan.  Nothing here waits for the device (unless the host decides the modes).
 * Two halves: plan_group (caller's thread: the plan, the ME parameters, the group's packets and reconstruction records queued in output
 * order, the fences it follows) and run_group (the enqueuing: on the device's feeder thread when there is one). */
static EbErrorType plan_group(shim_state *s, int cut_by_intra, int end_of_stream, shim_group *G) {
    shim_dev   *d = &s->dev[s->cur_dev];
    shim_plan  *P = &G->plan;
    if (shim_plan_group(s->pending_first, s->pending, s->levels, cut_by_intra, s->last_base, P) != 0) return EB_ErrorBadParameter;
    for (int i = 0; i < P->n; i++) {
        const EbErrorType e = job_params(s, &P->pic[i], &G->me[i]);
        if (e != EB_ErrorNone) return e;
    }
    G->end_of_stream = end_of_stream; G->dev = s->cur_dev;
    G->in = d->in;
    G->key = d->key;
    fence_clear(&d->key); /* (the GOP's later groups follow this one on the main context) */
    /* the group's packets, in decode order; their fences follow when the work has been enqueued */
    for (int i = 0; i < P->n; i++) {
        shim_slot *t = find_slot(d, P->pic[i].number);
        if (!t) return EB_ErrorBadParameter;
        G->pkt[i] = queue_packet(s, t->pts, 0, P->pic[i].n_lists == 2 ? 0 /* EB_B_PICTURE */ : 1 /* EB_P_PICTURE */, s->cur_dev, NULL);
        if (!G->pkt[i]) return EB_ErrorInsufficientResources;
        G->rec[i] = NULL;
    }
    /* ... and its reconstructions, in coding order (wave by wave, as they are produced) */
    if (s->cfg.recon_file)
        for (int w = 0; w < P->n_waves; w++)
            for (int i = 0; i < P->n; i++)
                if (P->pic[i].wave == w) {
                    G->rec[i] = reserve_recon(s, d, P->pic[i].number);
                    if (!G->rec[i]) return FAILED(s) ? EB_ErrorMax : EB_ErrorInsufficientResources;
                }
    return EB_ErrorNone;
}

static EbErrorType run_group(shim_state *s, shim_group *G) {
    shim_dev            *d = &s->dev[G->dev];
    const shim_plan     *P = &G->plan;
    const shim_plan_pic *jobs = P->pic;
    const int            n = P->n;
    /* everything enqueued on the main context from here on sees the group's pictures uploaded and analysed */
    GPU_TRY(fence_order(d->ctx, &G->in));
    svt_hip_ctx *const cm = (d->ctx_me && !s->opt.split_gop) ? d->ctx_me : d->ctx; /* where the group's search runs */
    if (cm != d->ctx) GPU_TRY(fence_order(cm, &G->in));
    /* launches: classes of pictures whose parameter sets may share one (svt_hip_me_params_same_launch: the library's own field-by-field rule) */
    int done[SHIM_MAX_MINIGOP] = {0};
    for (int i = 0; i < n; i++) {
        if (done[i]) continue;
        svt_pa_picture    cur[SHIM_MAX_MINIGOP], r0[SHIM_MAX_MINIGOP], r1[SHIM_MAX_MINIGOP];
        svt_me_params     pp[SHIM_MAX_MINIGOP];
        svt_me_pu_result *res[SHIM_MAX_MINIGOP];
        uint32_t         *rc[SHIM_MAX_MINIGOP];
        int               m = 0;
        for (int k = i; k < n; k++) {
            if (done[k] || !svt_hip_me_params_same_launch(&G->me[i], &G->me[k])) continue;
            shim_slot *t = find_slot(d, jobs[k].number), *a = find_slot(d, jobs[k].ref0), *b = find_slot(d, jobs[k].n_lists == 2 ? jobs[k].ref1 : jobs[k].ref0);
            if (!t || !a || !b) return stream_fail(s, "a picture of the group or one of its references is not resident");
            cur[m] = t->pa; r0[m] = a->pa; r1[m] = b->pa;
            pp[m] = G->me[k]; res[m] = (svt_me_pu_result *)t->d_results; rc[m] = (uint32_t *)t->d_rcme;
            done[k] = 1;
            m++;
        }
        GPU_TRY(svt_hip_me_batch_layers_device(cm, m, cur, r0, r1, pp, res, s->cfg.rate_control_mode ? rc : NULL));
        __atomic_add_fetch(&s->me_launches, 1, __ATOMIC_RELAXED);
    }
    /* the tail of the ME kernel process per picture (Codec/EbMotionEstimationProcess.c:1047-1237): stationary-edge flags and the
       rate-control histograms from the ME results and the picture-analysis variances, all device resident */
    const int res_class = svt_hip_input_resolution((int32_t)s->cfg.source_width, (int32_t)s->cfg.source_height);
    for (int i = 0; i < n; i++) {
        shim_slot *t = find_slot(d, jobs[i].number);
        svt_me_sb_stats_params sp;
        memset(&sp, 0, sizeof sp);
        sp.pic_width = (int32_t)s->cfg.source_width; sp.pic_height = (int32_t)s->cfg.source_height; sp.input_resolution = res_class;
        sp.temporal_layer_index = jobs[i].layer; sp.slice_type = jobs[i].n_lists == 2 ? 0 : 1;
        sp.run_part2 = !G->end_of_stream; sp.rate_control_mode = (int32_t)s->cfg.rate_control_mode;
        GPU_TRY(svt_hip_mem_set(cm, t->d_hist, 0, (2 * SVT_SAD_INTERVALS + 1) * sizeof(uint32_t)));
        GPU_TRY(svt_hip_me_sb_stats_device(cm, &sp, (const svt_me_pu_result *)t->d_results, (const uint16_t *)t->d_var,
                                           s->cfg.rate_control_mode ? (const uint32_t *)t->d_rcme : NULL, (svt_me_sb_stats *)t->d_stats, (uint32_t *)t->d_hist,
                                           (uint32_t *)t->d_hist + 2 * SVT_SAD_INTERVALS));
        t->info.is_intra = 0; t->info.temporal_layer_index = jobs[i].layer; t->info.hierarchical_levels = jobs[i].levels;
        t->info.num_ref_lists = jobs[i].n_lists;
        t->info.ref_picture_number[0] = jobs[i].ref0; t->info.ref_picture_number[1] = jobs[i].ref1;
        t->info.device_ordinal = d->ordinal;
    }
    shim_fence searched;
    GPU_TRY(fence_record(cm, &searched));
    for (int i = 0; i < n; i++) { shim_slot *t = find_slot(d, jobs[i].number); t->processed = 1; t->done = searched; }
    GPU_TRY(fence_order(d->ctx, &searched)); /* the layers below read the search's results */
    /* the waves predict from the GOP's intra picture (directly or through pictures that did): behind its encode pass on the key context */
    GPU_TRY(fence_order(d->ctx, &G->key));
    /* the stages behind mode decision, wave by wave (their references belong to earlier waves).  The deep-eligible waves (the two deepest
       layers of a part) go to the deep-layer context when there is one, behind everything the main context holds at that point (the
       part's shallower waves: their references).  With a host decision callback the pipeline drains per picture anyway: everything
       stays on the main context. */
    shim_fence wave_done[SHIM_MAX_WAVES];
    int        any_deep = 0;
    for (int w = 0; w < P->n_waves; w++) {
        int idx[SHIM_MAX_MINIGOP], m = 0;
        for (int i = 0; i < n; i++) if (jobs[i].wave == w) idx[m++] = i;
        const int deep = m && P->wave[w].deep_eligible && d->ctx_deep != d->ctx && !s->md_cb;
        if (deep) {
            shim_fence behind;
            GPU_TRY(fence_record(d->ctx, &behind));
            GPU_TRY(fence_order(d->ctx_deep, &behind));
            any_deep = 1;
        }
        for (int b = 0; b < m; b += SHIM_WAVE_MAX) {
            const EbErrorType e = encode_wave(s, d, G, idx + b, m - b < SHIM_WAVE_MAX ? m - b : SHIM_WAVE_MAX, deep);
            if (e != EB_ErrorNone) return e;
        }
        GPU_TRY(fence_record(deep ? d->ctx_deep : d->ctx, &wave_done[w]));
    }
    for (int i = 0; i < n; i++) { /* the packets (queued in decode order by plan_group) learn what they wait for */
        shim_slot *t = find_slot(d, jobs[i].number);
        G->pkt[i]->done = t->done = wave_done[jobs[i].wave];
        __atomic_store_n(&G->pkt[i]->ready, 1, __ATOMIC_RELEASE);
    }
    /* from this point of the main stream on nothing enqueued so far reads the group's pictures or the pictures it predicted from: the
       input side may overwrite their slots behind it */
    shim_fence end_main, end_deep = {0};
    GPU_TRY(fence_record(d->ctx, &end_main));
    if (any_deep) GPU_TRY(fence_record(d->ctx_deep, &end_deep)); /* ... and the deep-layer context's readers */
    for (int i = 0; i < n; i++) {
        const int64_t who[3] = {jobs[i].number, jobs[i].ref0, jobs[i].ref1};
        for (int k = 0; k < 3; k++) {
            shim_slot *t = who[k] >= 0 ? find_slot(d, who[k]) : NULL;
            if (t) { t->free_main = end_main; if (any_deep) t->free_deep = end_deep; }
        }
    }
    return EB_ErrorNone;
}

/* ---- the device's feeder thread ---- */
static void *feeder_main(void *arg) {
    shim_dev *d = (shim_dev *)arg;
    pthread_mutex_lock(&d->mu);
    for (;;) {
        while (d->job_state != 1 && !d->stop) pthread_cond_wait(&d->cv, &d->mu);
        if (d->stop) break;
        d->job_state = 2;
        pthread_mutex_unlock(&d->mu);
        const EbErrorType e = run_group(d->owner, &d->group);
        pthread_mutex_lock(&d->mu);
        d->job_result = (int)e;
        d->job_state = 0;
        pthread_cond_broadcast(&d->cv);
    }
    pthread_mutex_unlock(&d->mu);
    return NULL;
}
/* the caller waits for the group it posted to this device; a failed group ends the stream here */
static EbErrorType dev_join(shim_state *s, shim_dev *d) {
    if (!d->outstanding) return EB_ErrorNone;
    pthread_mutex_lock(&d->mu);
    while (d->job_state != 0) pthread_cond_wait(&d->cv, &d->mu);
    const EbErrorType e = (EbErrorType)d->job_result;
    d->job_result = (int)EB_ErrorNone;
    pthread_mutex_unlock(&d->mu);
    d->outstanding = 0;
    if (e != EB_ErrorNone) { SET_FAILED(s); return e; }
    return EB_ErrorNone;
}
static EbErrorType join_all(shim_state *s) {
    EbErrorType r = EB_ErrorNone;
    for (int k = 0; k < s->n_dev; k++) { const EbErrorType e = dev_join(s, &s->dev[k]); if (e != EB_ErrorNone) r = e; }
    return r;
}
static void feeder_start(shim_state *s, shim_dev *d) {
    d->owner = s;
    pthread_mutex_init(&d->mu, NULL);
    pthread_cond_init(&d->cv, NULL);
    d->job_state = 0; d->stop = 0; d->outstanding = 0; d->job_result = (int)EB_ErrorNone;
    d->has_feeder = s->use_feeder && pthread_create(&d->feeder, NULL, feeder_main, d) == 0;
}
static void feeder_stop(shim_dev *d) {
    if (!d->owner) return;
    if (d->has_feeder) {
        pthread_mutex_lock(&d->mu);
        while (d->job_state != 0) pthread_cond_wait(&d->cv, &d->mu);
        d->stop = 1;
        pthread_cond_broadcast(&d->cv);
        pthread_mutex_unlock(&d->mu);
        pthread_join(d->feeder, NULL);
        d->has_feeder = 0;
    }
    pthread_mutex_destroy(&d->mu);
    pthread_cond_destroy(&d->cv);
    d->owner = NULL;
}

static EbErrorType flush_pending(shim_state *s, int cut_by_intra, int end_of_stream) {
    if (!s->pending) return EB_ErrorNone;
    shim_dev *d = &s->dev[s->cur_dev];
    { const EbErrorType e = dev_join(s, d); if (e != EB_ErrorNone) return e; } /* one group per device at a time */
    shim_group *G = &d->group;
    { const EbErrorType e = plan_group(s, cut_by_intra, end_of_stream, G); if (e != EB_ErrorNone) { SET_FAILED(s); return e; } }
    s->last_base = G->plan.last;
    s->pending = 0;
    /* a regular group goes to the device's feeder; what the caller follows up at once (the intra picture behind a cut group, the
       end of the stream, a hand-over to another device) is enqueued here */
    if (d->has_feeder && !cut_by_intra && !end_of_stream && !s->opt.split_gop) {
        pthread_mutex_lock(&d->mu);
        d->job_state = 1;
        pthread_cond_broadcast(&d->cv);
        pthread_mutex_unlock(&d->mu);
        d->outstanding = 1;
        return EB_ErrorNone;
    }
    { const EbErrorType e = run_group(s, G); if (e != EB_ErrorNone) { SET_FAILED(s); return e; } }
    if (s->opt.split_gop && !cut_by_intra && !end_of_stream) { /* the next mini-GOP of this GOP goes to the next device */
        const int next = (s->cur_dev + 1) % s->n_dev;
        const EbErrorType e = handoff_base(s, d, &s->dev[next], s->last_base);
        if (e != EB_ErrorNone) return e;
        s->cur_dev = next;
    }
    return EB_ErrorNone;
}

static EbErrorType send_picture(shim_state *s, EbBufferHeaderType *b) {
    const int end = !b || !b->p_buffer || (b->flags & EB_BUFFERFLAG_EOS);
    EbErrorType e = EB_ErrorNone;
    const double t_enter = s->opt.profile ? now_s() : 0.0;
    double       tp = t_enter;
#define PROF(k) do { if (s->opt.profile) { const double n_ = now_s(); s->prof_s[k] += n_ - tp; tp = n_; } } while (0)
    if (b && b->p_buffer) {
        const EbSvtEncInput *in = (const EbSvtEncInput *)b->p_buffer;
        if (!in->luma || in->y_stride < s->cfg.source_width) return EB_ErrorBadParameter;
        if ((in->cb && in->cb_stride < s->cfg.source_width / 2) || (in->cr && in->cr_stride < s->cfg.source_width / 2)) return EB_ErrorBadParameter;
        const int64_t n = s->next_number;
        const int     W = s->W, H = s->H;
        const int     intra = n == 0 || (s->intra_period >= 0 && n % (s->intra_period + 1) == 0);
        if (intra) { /* an intra refresh closes the GOP: what is waiting is coded on its own device, cut as the reference cuts it */
            if ((e = flush_pending(s, 1, 0)) != EB_ErrorNone) return e;
            if (n) { s->gop++; if (!s->opt.split_gop) s->cur_dev = svt_hip_gop_owner(s->gop, s->n_dev); }
            s->last_base = -1;
        }
        PROF(3);
        shim_dev  *d = &s->dev[s->cur_dev];
        shim_slot *t = &d->slot[d->accepted % d->n_slots];
        /* the group the device's feeder is enqueuing may still write this slot's fences (never with the ring's regular distance of two
           mini-GOPs + 2; short GOPs on several devices can come closer): wait for it */
        if (d->outstanding && t->number >= d->group.plan.oldest) { if ((e = dev_join(s, d)) != EB_ErrorNone) return e; }
        /* the slot's previous picture (2 mini-GOPs + 2 ago on this device) must have left the GPU before its buffers are overwritten:
           the upload stream waits behind its last reader on the main context (else behind its own work), on the deep-layer context and
           on the output context (device-side waits; the host blocks only in the staging ring of the upload below, as the reference
           blocks when its picture pool is exhausted) */
        GPU_TRY(fence_order(d->ctx_up, t->free_main.set ? &t->free_main : &t->done));
        GPU_TRY(fence_order(d->ctx_up, &t->free_deep));
        GPU_TRY(fence_order(d->ctx_up, &t->out));
        /* the copy the reference makes in copy_frame_buffer (:2743-2796), into pinned staging: the caller's planes are free again
           on return; the transfer and the analysis below run asynchronously */
        const svt_yuv_planes sp = tight_planes(s, t->d_src);
        /* register_input: the application promises that its input buffers stay allocated while the encoder lives (a fixed pool,
           as the reference's application has): they are page-locked on first sight and read by the DMA engines directly, without the
           staging copy (svt_hip_mem_upload_2d_direct) */
        PROF(0);
        if (!s->opt.register_input && in->cb && in->cr) GPU_TRY(upload_tight(s, d->ctx_up, t->d_src, in->luma, in->cb, in->cr, in->y_stride, in->cb_stride, in->cr_stride));
        else {
            int32_t (*up)(svt_hip_ctx *, void *, size_t, const void *, size_t, size_t, size_t) = s->opt.register_input ? svt_hip_mem_upload_2d_direct : svt_hip_mem_upload_2d_async;
            GPU_TRY(up(d->ctx_up, sp.y, (size_t)W, in->luma, in->y_stride, (size_t)W, (size_t)H));
            if (in->cb) GPU_TRY(up(d->ctx_up, sp.u, (size_t)W / 2, in->cb, in->cb_stride, (size_t)W / 2, (size_t)H / 2));
            else GPU_TRY(svt_hip_mem_set(d->ctx_up, sp.u, 128, (size_t)(W / 2) * (H / 2)));
            if (in->cr) GPU_TRY(up(d->ctx_up, sp.v, (size_t)W / 2, in->cr, in->cr_stride, (size_t)W / 2, (size_t)H / 2));
            else GPU_TRY(svt_hip_mem_set(d->ctx_up, sp.v, 128, (size_t)(W / 2) * (H / 2)));
        }
        PROF(1);
        const uint8_t *lum = sp.y;
        const int32_t  stride = W;
        if (d->ctx_up != d->ctx_in) { /* the analysis follows the picture's copy (and, through it, the slot's release) */
            shim_fence uploaded;
            GPU_TRY(fence_record(d->ctx_up, &uploaded));
            GPU_TRY(fence_order(d->ctx_in, &uploaded));
        }
        GPU_TRY(svt_hip_pa_prepare_batch_device(d->ctx_in, 1, &lum, &stride, &t->pa, 1));
        GPU_TRY(svt_hip_pa_mean_variance_device(d->ctx_in, &t->pa.full, (uint8_t *)t->d_mean, (uint16_t *)t->d_var));
        GPU_TRY(fence_record(d->ctx_in, &d->in));
        /* direct uploads: the caller's planes have been read when this returns (the analysis kernels above are enqueued behind the copies
           and are not waited for) */
        if (s->opt.register_input) GPU_TRY(svt_hip_mem_upload_wait(d->ctx_up));
        PROF(2);
        /* the picture is accepted from here on */
        s->next_number = n + 1;
        d->accepted++;
        t->number = n; t->pts = b->pts; t->processed = 0; t->coded = 0; t->is_copy = 0;
        fence_clear(&t->done); fence_clear(&t->free_main); fence_clear(&t->free_deep); fence_clear(&t->out);
        memset(&t->info, 0, sizeof t->info);
        t->info.picture_number = (uint64_t)n; t->info.n_sb = (uint32_t)s->n_sb; t->info.device_ordinal = d->ordinal;
        if (intra) {
            t->info.is_intra = 1; t->info.num_ref_lists = 0; t->info.temporal_layer_index = 0; t->info.hierarchical_levels = s->levels;
            t->info.ref_picture_number[0] = t->info.ref_picture_number[1] = -1;
            /* the intra pass is enqueued here: on the key context (nothing the device's feeder touches -- unless reconstructions are
               fetched: the output context is shared), or on the device's main context */
            if (d->ctx_key == d->ctx || s->cfg.recon_file) { if ((e = dev_join(s, d)) != EB_ErrorNone) return e; }
            if ((e = encode_intra(s, d, t)) != EB_ErrorNone) return e;
            GPU_TRY(fence_record(d->ctx_key, &t->done));
            t->processed = 1;
            if (d->ctx_key == d->ctx) t->free_main = t->done;
            d->key = t->done;
            if (!queue_packet(s, t->pts, 0, 2 /* EB_I_PICTURE */, s->cur_dev, &t->done)) return EB_ErrorInsufficientResources;
            s->last_base = n;
            if (s->opt.profile > 1) fprintf(stderr, "SvtVp9Enc key frame %lld: %.1f us on the caller's thread\n", (long long)n, 1e6 * (now_s() - tp));
            PROF(4);
        } else {
            if (!s->pending) s->pending_first = n;
            if (++s->pending == s->minigop) e = flush_pending(s, 0, 0);
            PROF(3);
        }
    }
    if (end && e == EB_ErrorNone) {
        e = flush_pending(s, 0, 1);
        s->eos = 1;
        if (e == EB_ErrorNone) {
            if (s->q_tail) s->q_tail->hdr.flags |= EB_BUFFERFLAG_EOS; /* the last picture's packet closes the stream */
            else {
                shim_fence now;
                GPU_TRY(fence_record(s->dev[s->cur_dev].ctx, &now));
                if (!queue_packet(s, b ? b->pts : 0, EB_BUFFERFLAG_EOS, 0, s->cur_dev, &now)) e = EB_ErrorInsufficientResources;
            }
            if (s->r_tail) s->r_tail->flags |= EB_BUFFERFLAG_EOS; /* ... and the last reconstruction the recon stream (recon_output :4711-4713) */
        }
    }
    if (s->opt.profile) s->prof_s[5] += now_s() - t_enter;
#undef PROF
    return e;
}

/* The entry owns the upload context: direct uploads (register_input) read the CALLER's planes, and this is the only entry that starts
 * one -- whatever failed inside, it does not return while one may still be in flight. */
EbErrorType eb_vp9_svt_enc_send_picture(EbComponentType *h, EbBufferHeaderType *b) {
    shim_state *s = state_of(h);
    if (!s || !s->initialised) return EB_ErrorBadParameter;
    if (FAILED(s)) return EB_ErrorMax;
    if (s->eos) return EB_ErrorBadParameter;
    const EbErrorType e = send_picture(s, b);
    if (e != EB_ErrorNone && s->opt.register_input) (void)svt_hip_mem_upload_wait(s->dev[s->cur_dev].ctx_up);
    return e;
}

/* Non-blocking while pictures are still being sent (EB_NoErrorEmptyQueue when the next packet's GPU work has not finished);
 * with pic_send_done the call waits for it, as eb_vp9_svt_get_packet does (:2880-2915: eb_vp9_get_full_object vs the
 * non-blocking variant). */
EbErrorType eb_vp9_svt_get_packet(EbComponentType *h, EbBufferHeaderType **p_buffer, uint8_t pic_send_done) {
    shim_state *s = state_of(h);
    if (!s || !p_buffer) return EB_ErrorBadParameter;
    if (FAILED(s)) return EB_ErrorMax;
    shim_packet *p = s->q_head;
    if (!p) return EB_NoErrorEmptyQueue;
    /* the newest packet stays in the queue until the library knows whether it is the last one (it then carries EB_BUFFERFLAG_EOS): the
       end-of-stream buffer arrives in a send_picture call of its own (App/EbAppProcessCmd.c:483-494) */
    if (p == s->q_tail && !s->eos) return EB_NoErrorEmptyQueue;
    if (!__atomic_load_n(&p->ready, __ATOMIC_ACQUIRE)) { /* its group is still with the device's feeder */
        if (!pic_send_done) return EB_NoErrorEmptyQueue;
        const EbErrorType je = dev_join(s, &s->dev[p->dev]);
        if (je != EB_ErrorNone) return je;
        if (!__atomic_load_n(&p->ready, __ATOMIC_ACQUIRE)) return EB_ErrorMax;
    }
    if (pic_send_done) { GPU_TRY(fence_wait_host(&p->done)); }
    else {
        const int32_t q = fence_query(&p->done);
        if (q < 0) return gpu_fail(s);
        if (q == 0) return EB_NoErrorEmptyQueue;
    }
    s->q_head = p->next;
    if (!s->q_head) s->q_tail = NULL;
    p->next = NULL;
    *p_buffer = &p->hdr;
    return EB_ErrorNone;
}

void eb_vp9_svt_release_out_buffer(EbBufferHeaderType **p_buffer) {
    if (p_buffer && *p_buffer && (*p_buffer)->wrapper_ptr) {
        free((*p_buffer)->wrapper_ptr);
        *p_buffer = NULL;
    }
}

/* eb_vp9_svt_get_recon (:2837-2865): non-blocking; the next reconstructed picture, copied into the caller's p_buffer (the caller
 * allocates W * H * 3 / 2 bytes, App/EbAppContext.c allocate_output_recon_buffers), with the header fields copy_output_recon_buffer
 * copies (:2815-2830) */
EbErrorType eb_vp9_svt_get_recon(EbComponentType *h, EbBufferHeaderType *p_buffer) {
    shim_state *s = state_of(h);
    if (!s) return EB_ErrorBadParameter;
    if (!s->cfg.recon_file) return EB_ErrorMax; /* recon is not enabled */
    if (FAILED(s)) return EB_ErrorMax;
    shim_recon *r = s->r_head;
    if (!r || !p_buffer) return EB_NoErrorEmptyQueue;
    if (r == s->r_tail && !s->eos) return EB_NoErrorEmptyQueue; /* as for packets: the last reconstruction carries EB_BUFFERFLAG_EOS */
    shim_dev *d = &s->dev[r->dev];
    if (!__atomic_load_n(&r->ready, __ATOMIC_ACQUIRE)) return EB_NoErrorEmptyQueue; /* its group is still with the device's feeder */
    const int32_t q = fence_query(&r->done);
    if (q < 0) return gpu_fail(s);
    if (q == 0) return EB_NoErrorEmptyQueue;
    if (p_buffer->p_buffer) {
        if (p_buffer->n_alloc_len && p_buffer->n_alloc_len < s->pic_bytes) return EB_ErrorBadParameter;
        /* Y | Cb | Cr, tight: W x (H * 3 / 2) bytes as rows of W for the library's copy pool (a few threads) */
        svt_copy_rows_mt((uint8_t *)p_buffer->p_buffer, (size_t)s->W, r->host, (size_t)s->W, (size_t)s->W, (size_t)s->H * 3 / 2);
    }
    p_buffer->size = sizeof(EbBufferHeaderType);
    p_buffer->n_filled_len = (uint32_t)s->pic_bytes;
    p_buffer->pts = r->pts; p_buffer->dts = 0;
    p_buffer->flags = r->flags;
    p_buffer->pic_type = 0;
    s->r_head = r->next;
    if (!s->r_head) s->r_tail = NULL;
    r->next = d->free_recon;
    d->free_recon = r;
    return EB_ErrorNone;
}

static void shim_deinit(shim_state *s) {
    (void)join_all(s);
    while (s->q_head) { shim_packet *p = s->q_head; s->q_head = p->next; free(p); }
    s->q_tail = NULL;
    while (s->r_head) { /* undelivered reconstructions go back to their device's pool, which is freed with the device */
        shim_recon *r = s->r_head;
        s->r_head = r->next;
        r->next = s->dev[r->dev].free_recon;
        s->dev[r->dev].free_recon = r;
    }
    s->r_tail = NULL;
    for (int k = s->n_dev - 1; k >= 0; k--) free_dev(&s->dev[k]); /* (reverse: a later context may run on an earlier one's streams) */
    s->n_dev = 0;
    /* every stream has drained (join_all, free_dev): nothing reads the application's input buffers any more -- the page locks this encoder
       took on them go with it (the registry is process-wide and counted: the last encoder that leaves unlocks) */
    if (s->registry_held) { svt_hip_host_registry_release(); s->registry_held = 0; }
    if (s->opt.profile && s->next_number)
        fprintf(stderr, "SvtVp9Enc host time per picture (us): slot wait %.1f  upload %.1f  analysis %.1f  group hand-over %.1f  intra %.1f  | send_picture %.1f  (%lld pictures)\n",
                1e6 * s->prof_s[0] / (double)s->next_number, 1e6 * s->prof_s[1] / (double)s->next_number, 1e6 * s->prof_s[2] / (double)s->next_number,
                1e6 * s->prof_s[3] / (double)s->next_number, 1e6 * s->prof_s[4] / (double)s->next_number, 1e6 * s->prof_s[5] / (double)s->next_number, (long long)s->next_number);
    free(s->h_results); free(s->h_mc); free(s->h_lf);
    s->h_results = s->h_mc = s->h_lf = NULL;
    s->initialised = 0;
}

EbErrorType eb_vp9_deinit_encoder(EbComponentType *h) {
    shim_state *s = state_of(h);
    if (s) shim_deinit(s); /* the reference accepts a NULL component here (:1846) */
    return EB_ErrorNone;
}

EbErrorType eb_vp9_deinit_handle(EbComponentType *h) {
    if (!h) return EB_ErrorInvalidComponent;
    EbErrorType e = EB_ErrorNone;
    if (h->p_component_private) {
        (void)eb_vp9_deinit_encoder(h);
        free(h->p_component_private);
    } else {
        e = EB_ErrorUndefined;
    }
    free(h);
    return e;
}

/* part of the reference library's exported surface (EB_API, Codec/EbEncHandle.c:3086-3110): its sample application links it for its
 * own string handling (App/EbAppConfig.c) */
size_t eb_vp9_strnlen_ss(const char *str, size_t max_len) {
    if (!str || max_len == 0 || max_len > (4ul << 10)) return 0;
    size_t n = 0;
    while (n < max_len && str[n]) n++;
    return n;
}

/* ---- extensions ---- */
EbErrorType svt_vp9_shim_set_mode_decision(EbComponentType *h, svt_vp9_shim_md_callback cb, void *user) {
    shim_state *s = state_of(h);
    if (!s || s->initialised) return EB_ErrorBadParameter; /* before eb_vp9_init_encoder */
    s->md_cb = cb;
    s->md_user = user;
    return EB_ErrorNone;
}

/* what every getter starts with: the feeders joined, the picture found where it was coded, its work (need_coded: the stages behind mode
 * decision; else its ME / analysis) enqueued -- a picture that waits in an incomplete mini-GOP has no results yet, neither has one the
 * ring has already given away: EB_NoErrorEmptyQueue -- and complete */
static EbErrorType settled_slot(shim_state *s, uint64_t picture_number, int need_coded, shim_dev **d, shim_slot **t) {
    if (!s || !s->initialised) return EB_ErrorBadParameter;
    { const EbErrorType je = join_all(s); if (je != EB_ErrorNone) return je; }
    *t = find_any(s, (int64_t)picture_number, d);
    if (!*t || !(need_coded ? (*t)->coded : (*t)->processed)) return EB_NoErrorEmptyQueue;
    GPU_TRY(fence_wait_host(&(*t)->done));
    return EB_ErrorNone;
}

EbErrorType svt_vp9_shim_get_me_results(EbComponentType *h, uint64_t picture_number, svt_vp9_shim_picture_info *info, void *out,
                                        uint64_t out_bytes) {
    shim_state *s = state_of(h);
    shim_dev *d = NULL; shim_slot *t = NULL;
    { const EbErrorType e = settled_slot(s, picture_number, 0, &d, &t); if (e != EB_ErrorNone) return e; }
    if (info) *info = t->info;
    if (out && !t->info.is_intra) {
        const uint64_t need = (uint64_t)t->info.n_sb * 85 * sizeof(svt_me_pu_result);
        if (out_bytes < need) return EB_ErrorBadParameter;
        GPU_TRY(svt_hip_mem_download(d->ctx, out, t->d_results, (size_t)need));
    }
    return EB_ErrorNone;
}

EbErrorType svt_vp9_shim_get_sb_stats(EbComponentType *h, uint64_t picture_number, void *stats, uint64_t stats_bytes, uint32_t *histograms,
                                      uint8_t *mean, uint16_t *variance) {
    shim_state *s = state_of(h);
    shim_dev *d = NULL; shim_slot *t = NULL;
    { const EbErrorType e = settled_slot(s, picture_number, 0, &d, &t); if (e != EB_ErrorNone) return e; }
    const size_t n_sb = t->info.n_sb;
    if (stats && !t->info.is_intra) {
        if (stats_bytes < n_sb * sizeof(svt_me_sb_stats)) return EB_ErrorBadParameter;
        GPU_TRY(svt_hip_mem_download(d->ctx, stats, t->d_stats, n_sb * sizeof(svt_me_sb_stats)));
    }
    if (histograms && !t->info.is_intra) GPU_TRY(svt_hip_mem_download(d->ctx, histograms, t->d_hist, (2 * SVT_SAD_INTERVALS + 1) * sizeof(uint32_t)));
    if (mean) GPU_TRY(svt_hip_mem_download(d->ctx, mean, t->d_mean, n_sb * 85));
    if (variance) GPU_TRY(svt_hip_mem_download(d->ctx, variance, t->d_var, n_sb * 85 * sizeof(uint16_t)));
    return EB_ErrorNone;
}

EbErrorType svt_vp9_shim_get_coded_picture(EbComponentType *h, uint64_t picture_number, svt_vp9_shim_picture_info *info, void *mc_mode_info,
                                           void *lf_mode_info, int16_t *qcoeff, uint16_t *eob_map) {
    shim_state *s = state_of(h);
    shim_dev *d = NULL; shim_slot *t = NULL;
    { const EbErrorType e = settled_slot(s, picture_number, 1, &d, &t); if (e != EB_ErrorNone) return e; }
    if (info) *info = t->info;
    const size_t units = (size_t)s->mi_rows * s->mi_cols;
    if (mc_mode_info) GPU_TRY(svt_hip_mem_download(d->ctx, mc_mode_info, t->d_mc_mi, units * sizeof(svt_mc_mode_info)));
    if (lf_mode_info) GPU_TRY(svt_hip_mem_download(d->ctx, lf_mode_info, t->d_lf_mi, units * sizeof(svt_lf_mode_info)));
    if (qcoeff) GPU_TRY(svt_hip_mem_download(d->ctx, qcoeff, t->d_qcoeff, s->coeffs * sizeof(int16_t)));
    if (eob_map) GPU_TRY(svt_hip_mem_download(d->ctx, eob_map, t->d_eob_map, (size_t)(s->W / 4) * (s->H / 4) * 3 / 2 * sizeof(uint16_t)));
    return EB_ErrorNone;
}

EbErrorType svt_vp9_shim_get_reference_picture(EbComponentType *h, uint64_t picture_number, uint8_t *out, uint64_t bytes) {
    shim_state *s = state_of(h);
    shim_dev *d = NULL; shim_slot *t = NULL;
    if (!out) return EB_ErrorBadParameter;
    { const EbErrorType e = settled_slot(s, picture_number, 1, &d, &t); if (e != EB_ErrorNone) return e; }
    const size_t need = s->pw * s->ph + 2 * s->cpw * s->cph;
    if (bytes < need) return EB_ErrorBadParameter;
    GPU_TRY(svt_hip_mem_download(d->ctx, out, t->d_rec, need));
    return EB_ErrorNone;
}

EbErrorType svt_vp9_shim_get_counters(EbComponentType *h, uint64_t *me_launches, uint64_t *pictures_sent) {
    shim_state *s = state_of(h);
    if (!s) return EB_ErrorBadParameter;
    (void)join_all(s);
    if (me_launches) *me_launches = s->me_launches;
    if (pictures_sent) *pictures_sent = (uint64_t)s->next_number;
    return EB_ErrorNone;
}

/*
 * mvrefs_stage.h -- the stage -> derive -> status skeleton of the stages that walk the 11 x 11 window of mvrefs_core.h (mvrefs.hip,
 * md_inter.hip): grids -> svt_mi_inter_ext records, candidate records and sums over a picture's leaves.
 *
 * Every candidate of a block lies in the window that starts 3 units above and 3 left of its SB, so, in the shape of syntax_stage.h:
 *   mvs_stage_window      a wave's 64 lanes pack the window's 121 units into LDS, three dwords a unit; what packs a unit is the caller's
 *   mvs_derive_kernel<S>  one wave per (picture, SB), one lane per 8x8 unit in z-order: the window of svt_mvr_pack, is the unit's record
 *                         one the stage takes, svt_mvr_unit from LDS alone, the unit's records (mvs_store_records: dwords / uint4, or
 *                         halves where a buffer has only the records' own alignment of 2; a null buffer is left out), and the wave's
 *                         S::N sums -- or SVT_MODES_BAD_GRID S::N times -- in the picture's part of the context's scratch
 *   mvs_status_kernel<S>  one workgroup per picture: the sums of the SBs -> d_status[0 .. S::STATUS_WORDS), in the shape of
 *                         syn_scan_kernel; the words behind the sums are 0; SVT_MODES_BAD_GRID in every word of a grid not taken
 * 1 452 bytes of LDS per wave: the 160 KB of a CU hold far more waves than its SIMDs take.  No atomics, and workgroups do not talk to
 * each other: the passes are separate launches in stream order.
 *
 * A stage is a policy struct S:
 *   picture, pic_dev       the caller's picture descriptor; what the kernels read of a picture: svt_mvr_view v, svt_mi_inter_ext *ext_out,
 *                          svt_mvref_cand *cand, uint32_t *status, *part ([n_sb][N]), and the stage's own fields
 *   N, STATUS_WORDS        sums per unit; words of d_status
 *   PART_SLOT              the context's slot of the per-SB sums
 *   NAME                   the prefix of the stage's error strings
 *   also_refused           what a unit that passed svt_mvr_check must satisfy besides (0: taken)
 *   sums                   the N sums' terms of one unit from its svt_mvr_unit_out
 *   fill                   checks a picture and fills its pic_dev but for part: the error string without prefix, or nullptr
 *   scratch                after the device is set: the stage's further slots and the fields that point into them; false: out of memory
 * The kernels are templates so that each stage's code object holds its own, named mvs_*_kernel<S>.
 */
#ifndef SVT_MVREFS_STAGE_H
#define SVT_MVREFS_STAGE_H
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "svt_ctx.h"
#include "mvrefs_core.h"
#include "wave_ops.h"

enum { MVS_MAX_PICS = 32 };

template <class S> struct mvs_batch_dev {
    typename S::pic_dev pic[MVS_MAX_PICS];
    svt_tok_geom        g;
    int32_t             n_sb, sb_cols;
};

/* the lane's place in a launch of one wave per (picture, SB): unit (r, c) = (sb_r + ur, sb_c + uc), which may lie outside the picture */
struct mvs_lane {
    int sb, pic, lane, sb_r, sb_c, ur, uc, r, c;
};
__device__ __forceinline__ mvs_lane mvs_lane_of(int n_sb, int sb_cols) {
    mvs_lane w;
    w.sb = (int)blockIdx.x % n_sb; w.pic = (int)blockIdx.x / n_sb; w.lane = (int)threadIdx.x;
    w.sb_r = (w.sb / sb_cols) * 8; w.sb_c = (w.sb % sb_cols) * 8;
    svt_tok_unit_of(w.lane, &w.ur, &w.uc);
    w.r = w.sb_r + w.ur; w.c = w.sb_c + w.uc;
    return w;
}

/* pack(r, c): the svt_mvr_entry of a unit inside the picture.  The caller's barrier stands between this and the first read */
template <class Pack> __device__ __forceinline__ void mvs_stage_window(uint32_t *s_win, const svt_tok_geom *g, const mvs_lane &w, Pack pack) {
    for (int i = w.lane; i < SVT_MVR_WIN * SVT_MVR_WIN; i += 64) {
        int           r, c;
        svt_mvr_entry e = svt_mvr_no_entry();
        if (svt_mvr_window_unit(g, w.sb_r, w.sb_c, i, &r, &c)) e = pack(r, c);
        svt_mvr_window_put(s_win, i, e);
    }
}

__device__ __forceinline__ void mvs_store_halves(uint16_t *d, uint32_t w) { d[0] = (uint16_t)w; d[1] = (uint16_t)(w >> 16); }
__device__ __forceinline__ void mvs_store_records(const svt_mvr_unit_out &o, svt_mi_inter_ext *ext_out, svt_mvref_cand *cand, size_t idx) {
    const uint32_t k[8] = {o.k0, o.k1, o.k2, o.k3, o.k4, o.k5, o.k6, o.k7};
    if (ext_out) {
        if (((uintptr_t)ext_out & 3) == 0) {
            uint32_t *d = (uint32_t *)(ext_out + idx);
            d[0] = o.e0; d[1] = o.e1; d[2] = o.e2;
        } else { /* (the record's own alignment is 2) */
            uint16_t *d = (uint16_t *)(ext_out + idx);
            mvs_store_halves(d, o.e0); mvs_store_halves(d + 2, o.e1); mvs_store_halves(d + 4, o.e2);
        }
    }
    if (cand) {
        if (((uintptr_t)cand & 15) == 0) {
            uint4 *d = (uint4 *)(cand + idx);
            d[0] = make_uint4(k[0], k[1], k[2], k[3]);
            d[1] = make_uint4(k[4], k[5], k[6], k[7]);
        } else {
            uint16_t *d = (uint16_t *)(cand + idx);
#pragma unroll
            for (int j = 0; j < 8; j++) mvs_store_halves(d + 2 * j, k[j]);
        }
    }
}

template <class S> __global__ __launch_bounds__(64) void mvs_derive_kernel(const mvs_batch_dev<S> *__restrict__ B) {
    __shared__ uint32_t s_win[SVT_MVR_WIN_WORDS];
    const mvs_lane               w = mvs_lane_of(B->n_sb, B->sb_cols);
    const typename S::pic_dev   &P = B->pic[w.pic];
    const svt_tok_geom           g = B->g;
    mvs_stage_window(s_win, &g, w, [&](int r, int c) { return svt_mvr_pack(&P.v, &g, r, c); });
    const int  r = w.r, c = w.c;
    const bool in = r < g.mi_rows && c < g.mi_cols;
    const bool bad = in && (svt_mvr_check(&P.v, &g, r, c) || S::also_refused(P, &g, r, c));
    const int  any_bad = wave_sum(bad ? 1 : 0);
    __syncthreads();
    int s[S::N] = {};
    /* (an SB with a record the stage does not take is not analysed: its fields may be anything) */
    if (in && !any_bad) {
        const svt_mvr_unit_out o = svt_mvr_unit(&P.v, &g, s_win, w.ur + 3, w.uc + 3, r, c);
        S::sums(P, &g, r, c, o, s);
        mvs_store_records(o, P.ext_out, P.cand, (size_t)r * g.mi_stride + c);
    }
#pragma unroll
    for (int k = 0; k < S::N; k++) {
        const int n = wave_sum(s[k]);
        if (w.lane == 0) P.part[S::N * w.sb + k] = any_bad ? SVT_MODES_BAD_GRID : (uint32_t)n;
    }
}

/* part[0 .. n_sb) -> status[0 .. STATUS_WORDS): the N sums and zeros, or SVT_MODES_BAD_GRID in every word */
template <class S> __global__ __launch_bounds__(256) void mvs_status_kernel(const mvs_batch_dev<S> *__restrict__ B) {
    __shared__ uint32_t s_sum[S::N][256];
    __shared__ uint32_t s_bad;
    const typename S::pic_dev &P = B->pic[blockIdx.x];
    const uint32_t            *a = P.part;
    const int n = B->n_sb, t = (int)threadIdx.x, per = (n + 255) / 256, b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    if (t == 0) s_bad = 0;
    __syncthreads();
    uint32_t s[S::N] = {};
    bool     bad = false;
    for (int i = b; i < e; i++) {
        bad |= a[S::N * i] == SVT_MODES_BAD_GRID;
#pragma unroll
        for (int k = 0; k < S::N; k++) s[k] += a[S::N * i + k];
    }
    if (bad) s_bad = 1;
#pragma unroll
    for (int k = 0; k < S::N; k++) s_sum[k][t] = s[k];
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) {
#pragma unroll
            for (int k = 0; k < S::N; k++) s_sum[k][t] += s_sum[k][t + d];
        }
        __syncthreads();
    }
    if (t < S::STATUS_WORDS) P.status[t] = s_bad ? SVT_MODES_BAD_GRID : t < S::N ? s_sum[t][0] : 0u;
}

template <class S> int32_t mvs_error(int32_t code, const char *what) {
    char msg[192];
    snprintf(msg, sizeof msg, "%s: %s", S::NAME, what);
    return svt_set_error(code, msg);
}

/* the checks and fields of a picture that are every stage's; ext: the records the view reads, if the caller holds them; view_null: a
 * null pointer among the stage's own */
template <class S> const char *mvs_fill_common(const typename S::picture &p, typename S::pic_dev &P, const svt_mi_inter_ext *ext, bool view_null) {
    if (view_null || !p.d_lf_mi || !p.d_mc_mi || !p.d_status) return "null picture field";
    if (p.ref_mask & 0xF1) return "ref_mask names a reference frame outside 1 .. 3";
    P.v = svt_mvr_view_of(p.d_lf_mi, p.d_mc_mi, ext, p.ref_mask, p.restrict_ref_mvs, p.ref_frame_sign_bias);
    P.ext_out = p.d_ext_out; P.cand = p.d_cand; P.status = p.d_status;
    return nullptr;
}

/* launch(dB, n_sb): the stage's launches on ctx->stream, bracketed by the context's events */
template <class S, class Launch>
int32_t mvs_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const typename S::picture *pics, int32_t width, int32_t height, int32_t mi_stride, Launch launch) {
    mvs_batch_dev<S> hb;
    memset(&hb, 0, sizeof hb);
    if (!ctx || !pics || n_pics < 1 || n_pics > MVS_MAX_PICS || svt_tok_geom_of(width, height, mi_stride, &hb.g, &hb.sb_cols, &hb.n_sb))
        return mvs_error<S>(SVT_HIP_ERR_BAD_PARAMETER, "bad argument");
    for (int i = 0; i < n_pics; i++)
        if (const char *what = S::fill(pics[i], hb.pic[i])) return mvs_error<S>(SVT_HIP_ERR_BAD_PARAMETER, what);
    HIP_TRY(hipSetDevice(ctx->device));
    uint32_t *part = (uint32_t *)svt_ctx_slot(ctx, S::PART_SLOT, sizeof(uint32_t) * S::N * (size_t)n_pics * (size_t)hb.n_sb);
    const bool own = S::scratch(ctx, hb, n_pics); /* (both are asked for, as before, whichever fails) */
    if (!part || !own) return mvs_error<S>(SVT_HIP_ERR_NO_RESOURCES, "scratch");
    for (int i = 0; i < n_pics; i++) hb.pic[i].part = part + S::N * (size_t)i * (size_t)hb.n_sb;
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof hb, &h, &d)) return mvs_error<S>(SVT_HIP_ERR_NO_RESOURCES, "descriptor buffers");
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    memcpy(h, &hb, sizeof hb);
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof hb));
    launch((const mvs_batch_dev<S> *)d, hb.n_sb);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}
#endif

/*
 * syntax_stage.h -- the count -> scan -> emit skeleton of the mode-info syntax stages (modeinfo.hip, modeinfo_inter.hip): grids -> raw
 * bool records + the segment list that interleaves them with the tokeniser's records for the bool coder.
 *
 * The bools of an 8x8 unit are a function of the grids alone, so, in the shape of the tokeniser:
 *   syn_count_kernel<S>  one wave per (picture, SB), one lane per 8x8 unit in z-order (= coding order): is the unit's record one the
 *                        syntax takes, and how many bools start at it -- no probabilities are read
 *   syn_scan_kernel<S>   one workgroup per picture: first bool of every SB, the picture's total or SVT_MODES_BAD_GRID (written always)
 *   syn_emit_kernel<S>   S::EMIT_WAVES waves per workgroup, one per (picture, SB): the unit analysis again, now with the unit's place in
 *                        the SB; a lane writes its records into the wave's part of LDS, the wave stores the SB's records as consecutive
 *                        dwords (a 2-byte store only at an odd first / last record), and every lane writes its unit's four segment
 *                        slots as three 16-byte stores -- every slot of the list, so the list needs no clearing pass
 * No atomics, and workgroups do not talk to each other: the passes are separate launches in stream order.
 *
 * A stage is a policy struct S:
 *   picture, view, tables     the caller's picture descriptor, what the core functions read of a picture, the probabilities
 *   UNIT_BOOLS, EMIT_WAVES    most bools of a unit; a wave's part of LDS is 64 * UNIT_BOOLS records
 *   SCRATCH_SLOT, TABLES_SLOT the context's slots of the per-SB offsets and of the tables
 *   NAME                      the prefix of the stage's error strings, "svt_hip_<NAME>_set_tables" its table setter
 *   check, unit_bools, grid   the core's two functions of a unit; the svt_lf_mode_info grid of a view
 *   fill                      checks a picture and fills its syn_pic_dev but for sb_off: the error string without prefix, or nullptr
 * The kernels are templates so that each stage's code object holds its own three, named syn_*_kernel<S>.
 */
#ifndef SVT_SYNTAX_STAGE_H
#define SVT_SYNTAX_STAGE_H
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "svt_ctx.h"
#include "modeinfo_core.h"
#include "wave_ops.h"

enum { SYN_MAX_PICS = 32 };

template <class S> struct syn_pic_dev {
    typename S::view v;
    const uint16_t  *eob_map;
    const uint32_t  *tok_off;
    uint16_t        *bools;
    uint4           *segs;
    uint32_t        *n_bools, *sb_off;
    uint32_t         capacity, pad_;
};
template <class S> struct syn_batch_dev {
    syn_pic_dev<S> pic[SYN_MAX_PICS];
    svt_tok_geom   g;
    int32_t        n_sb, sb_cols;
};

template <class S> __global__ __launch_bounds__(64) void syn_count_kernel(const syn_batch_dev<S> *__restrict__ B) {
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const syn_pic_dev<S> &P = B->pic[pic];
    const svt_tok_geom    g = B->g;
    int ur, uc;
    svt_tok_unit_of(lane, &ur, &uc);
    const int  r = (sb / B->sb_cols) * 8 + ur, c = (sb % B->sb_cols) * 8 + uc;
    const bool in = r < g.mi_rows && c < g.mi_cols;
    const bool bad = in && S::check(P.v, &g, r, c);
    const int  any_bad = wave_sum(bad ? 1 : 0);
    /* (an SB with a record the syntax does not take is not analysed: its own and its neighbours' fields may be anything) */
    const int  total = wave_sum(in && !any_bad ? S::unit_bools(P.v, &g, r, c, nullptr, nullptr) : 0);
    if (lane == 0) P.sb_off[sb] = any_bad ? SVT_MODES_BAD_GRID : (uint32_t)total;
}

/* in place: sb_off[0 .. n_sb) counts -> exclusive prefixes, sb_off[n_sb] = *n_bools = the total, or SVT_MODES_BAD_GRID */
template <class S> __global__ __launch_bounds__(256) void syn_scan_kernel(const syn_batch_dev<S> *__restrict__ B) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t s_bad;
    const syn_pic_dev<S> &P = B->pic[blockIdx.x];
    uint32_t             *a = P.sb_off;
    const int n = B->n_sb, t = (int)threadIdx.x, per = (n + 255) / 256, b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    if (t == 0) s_bad = 0;
    __syncthreads();
    uint32_t s = 0;
    bool     bad = false;
    for (int i = b; i < e; i++) { bad |= a[i] == SVT_MODES_BAD_GRID; s += a[i]; }
    if (bad) s_bad = 1;
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int i = b; i < e; i++) { const uint32_t v = a[i]; a[i] = run; run += v; }
    if (t == 255) {
        const uint32_t total = s_bad ? SVT_MODES_BAD_GRID : part[255];
        a[n] = total;
        *P.n_bools = total;
    }
}

template <class S> __global__ __launch_bounds__(64 * S::EMIT_WAVES) void syn_emit_kernel(const syn_batch_dev<S> *__restrict__ B, const typename S::tables *__restrict__ tables) {
    __shared__ uint16_t s_bools[S::EMIT_WAVES][64 * S::UNIT_BOOLS];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, sb = (int)blockIdx.x * S::EMIT_WAVES + wave;
    const syn_pic_dev<S> &P = B->pic[blockIdx.y];
    const svt_tok_geom    g = B->g;
    const bool live = sb < B->n_sb;
    uint16_t  *s = s_bools[wave];
    uint32_t   base = 0;
    int        total = 0;
    if (live) {
        const bool ok = P.sb_off[B->n_sb] != SVT_MODES_BAD_GRID;
        int ur, uc;
        svt_tok_unit_of(lane, &ur, &uc);
        const int  r = (sb / B->sb_cols) * 8 + ur, c = (sb % B->sb_cols) * 8 + uc;
        const bool in = ok && r < g.mi_rows && c < g.mi_cols;
        const int  cnt = in ? S::unit_bools(P.v, &g, r, c, nullptr, nullptr) : 0;
        const int  pre = wave_excl_prefix(cnt, lane);
        total = wave_sum(cnt);
        base = P.sb_off[sb];
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0, q2 = q0; /* the unit's four {first, count, kind} */
        if (cnt) {
            (void)S::unit_bools(P.v, &g, r, c, tables, s + pre);
            uint32_t first[3], count[3];
            svt_mi_leaf_tokens(S::grid(P.v), P.eob_map, P.tok_off, &g, r, c, first, count);
            q0 = make_uint4(base + (uint32_t)pre, (uint32_t)cnt, 1u, count[0] ? first[0] : 0u);
            q1 = make_uint4(count[0], 0u, count[1] ? first[1] : 0u, count[1]);
            q2 = make_uint4(0u, count[2] ? first[2] : 0u, count[2], 0u);
        }
        uint4 *dst = P.segs + 3 * ((size_t)sb * 64 + lane);
        dst[0] = q0; dst[1] = q1; dst[2] = q2;
    }
    __syncthreads();
    if (live && total) { /* records [0, total) of s go to bools[base ..): dwords from the first even index on */
        const uint32_t n = (uint32_t)total, cap = P.capacity, head = base & 1u, pairs = (n - head) >> 1;
        if (lane == 0 && head && base < cap) P.bools[base] = s[0];
        for (uint32_t j = (uint32_t)lane; j < pairs; j += 64) {
            const uint32_t i = head + 2 * j, gi = base + i;
            if (gi + 1 < cap) *(uint32_t *)(P.bools + gi) = (uint32_t)s[i] | (uint32_t)s[i + 1] << 16;
            else if (gi < cap) P.bools[gi] = s[i];
        }
        if (lane == 63 && ((n - head) & 1u) && base + n - 1 < cap) P.bools[base + n - 1] = s[n - 1];
    }
}

template <class S> int32_t syn_error(int32_t code, const char *what) {
    char msg[192];
    snprintf(msg, sizeof msg, "%s: %s", S::NAME, what);
    return svt_set_error(code, msg);
}

/* the checks and fields of a picture that are every stage's; view_null: a null pointer among the stage's own */
template <class S> const char *syn_fill_common(const typename S::picture &p, syn_pic_dev<S> &P, bool view_null) {
    if (view_null || !p.d_eob_map || !p.d_tok_off || !p.d_segments || !p.d_n_bools || (!p.d_bools && p.capacity)) return "null picture field";
    if (((uintptr_t)p.d_segments & 15) || ((uintptr_t)p.d_bools & 3)) return "d_segments must be 16-byte aligned, d_bools 4-byte aligned";
    P.eob_map = p.d_eob_map; P.tok_off = p.d_tok_off; P.bools = p.d_bools; P.segs = (uint4 *)p.d_segments; P.n_bools = p.d_n_bools;
    P.capacity = p.capacity;
    return nullptr;
}

template <class S> int32_t syn_set_tables(svt_hip_ctx *ctx, const typename S::tables *tables) {
    return svt_ctx_set_tables(ctx, S::TABLES_SLOT, tables, sizeof(typename S::tables), S::NAME);
}

template <class S> int32_t syn_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const typename S::picture *pics, int32_t width, int32_t height, int32_t mi_stride) {
    syn_batch_dev<S> hb;
    memset(&hb, 0, sizeof hb);
    if (!ctx || !pics || n_pics < 1 || n_pics > SYN_MAX_PICS || svt_tok_geom_of(width, height, mi_stride, &hb.g, &hb.sb_cols, &hb.n_sb))
        return syn_error<S>(SVT_HIP_ERR_BAD_PARAMETER, "bad argument");
    for (int i = 0; i < n_pics; i++)
        if (const char *what = S::fill(pics[i], hb.pic[i])) return syn_error<S>(SVT_HIP_ERR_BAD_PARAMETER, what);
    if (!ctx->slot_bytes[S::TABLES_SLOT]) {
        char what[96];
        snprintf(what, sizeof what, "svt_hip_%s_set_tables has not been called", S::NAME);
        return syn_error<S>(SVT_HIP_ERR_BAD_PARAMETER, what);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    uint32_t *sb_off = (uint32_t *)svt_ctx_slot(ctx, S::SCRATCH_SLOT, sizeof(uint32_t) * (size_t)n_pics * ((size_t)hb.n_sb + 1));
    if (!sb_off) return syn_error<S>(SVT_HIP_ERR_NO_RESOURCES, "scratch");
    for (int i = 0; i < n_pics; i++) hb.pic[i].sb_off = sb_off + (size_t)i * ((size_t)hb.n_sb + 1);
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof hb, &h, &d)) return syn_error<S>(SVT_HIP_ERR_NO_RESOURCES, "descriptor buffers");
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    memcpy(h, &hb, sizeof hb);
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof hb));
    const syn_batch_dev<S>   *dB = (const syn_batch_dev<S> *)d;
    const typename S::tables *dT = (const typename S::tables *)ctx->slot[S::TABLES_SLOT];
    hipLaunchKernelGGL(syn_count_kernel<S>, dim3(n_pics * hb.n_sb), dim3(64), 0, ctx->stream, dB);
    hipLaunchKernelGGL(syn_scan_kernel<S>, dim3(n_pics), dim3(256), 0, ctx->stream, dB);
    hipLaunchKernelGGL(syn_emit_kernel<S>, dim3((hb.n_sb + S::EMIT_WAVES - 1) / S::EMIT_WAVES, n_pics), dim3(64 * S::EMIT_WAVES), 0, ctx->stream, dB, dT);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}
#endif

/*
 * modeinfo_inter.hip -- the mode-info syntax of batches of inter pictures (gfx950): grids -> raw bool records + the segment list that
 * interleaves them with the tokeniser's records for the bool coder.  The counterpart of modeinfo.hip for every picture that is not
 * intra-only.
 *
 * Replaces write_partition and pack_inter_mode_mvs as eb_vp9_entropy_coding_kernel calls them per block in front of pack_mb_tokens
 * (Codec/EbEntropyCodingProcess.c:60-449, Source/Lib/VPX/vp9_bitstream.c:206-321, 399-417).
 *
 * Every context is a function of the grid (modeinfo_inter_core.h), and the bools of a unit are a function of its own records and its
 * two neighbours'.  So, in the shape of the key-frame stage:
 *   svt_mii_count_kernel  one wave per (picture, SB), one lane per 8x8 unit in z-order (= coding order): are the unit's records ones
 *                         this syntax takes, and how many bools start at it -- no probabilities and no neighbours are read; the MV
 *                         differences decide joint, class, fraction and the high-precision bit
 *   svt_mii_scan_kernel   one workgroup per picture: first bool of every SB, the picture's total or SVT_MODES_BAD_GRID (written
 *                         always) -- svt_mi_scan_kernel's algorithm
 *   svt_mii_emit_kernel   two waves per workgroup, one per (picture, SB): the unit analysis again, now with the neighbours' contexts
 *                         and the unit's place in the SB; a lane writes its records into the wave's part of LDS, the wave stores the
 *                         SB's records as consecutive dwords (a 2-byte store only at an odd first / last record), and every lane
 *                         writes its unit's four segment slots as three 16-byte stores -- every slot of the list
 * A wave's part of LDS holds 64 units x SVT_MII_UNIT_BOOLS (111) records = 14 208 bytes; two waves a workgroup = 28 416 bytes, so the
 * 160 KB of a CU hold five workgroups = ten waves (four waves a workgroup: two workgroups = eight waves).  No atomics, and workgroups
 * do not talk to each other: the passes are separate launches in stream order.
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"
#include "modeinfo_inter_core.h"

#define MII_MAX_PICS 32
#define MII_SCRATCH_SLOT 52
#define MII_TABLES_SLOT 53
#define MII_EMIT_WAVES 2
#define MII_WAVE_BOOLS (64 * SVT_MII_UNIT_BOOLS)

namespace {

struct mii_pic_dev {
    svt_mii_view    v;
    const uint16_t *eob_map;
    const uint32_t *tok_off;
    uint16_t       *bools;
    uint4          *segs;
    uint32_t       *n_bools, *sb_off;
    uint32_t        capacity, pad_;
};
struct mii_batch_dev {
    mii_pic_dev  pic[MII_MAX_PICS];
    svt_tok_geom g;
    int32_t      n_sb, sb_cols;
};

__device__ __forceinline__ int mii_wave_sum(int v) {
    _Pragma("unroll") for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int mii_wave_excl_prefix(int v, int lane) {
    int incl = v;
    _Pragma("unroll") for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    return incl - v;
}

__global__ __launch_bounds__(64) void svt_mii_count_kernel(const mii_batch_dev *__restrict__ B) {
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const mii_pic_dev &P = B->pic[pic];
    const svt_tok_geom g = B->g;
    int ur, uc;
    svt_tok_unit_of(lane, &ur, &uc);
    const int  r = (sb / B->sb_cols) * 8 + ur, c = (sb % B->sb_cols) * 8 + uc;
    const bool in = r < g.mi_rows && c < g.mi_cols;
    const bool bad = in && svt_mii_check(&P.v, &g, r, c);
    const int  any_bad = mii_wave_sum(bad ? 1 : 0);
    /* (an SB with a record the syntax does not take is not analysed: its fields may be anything) */
    const int  total = mii_wave_sum(in && !any_bad ? svt_mii_unit_bools(&P.v, &g, r, c, nullptr, nullptr) : 0);
    if (lane == 0) P.sb_off[sb] = any_bad ? SVT_MODES_BAD_GRID : (uint32_t)total;
}

/* in place: sb_off[0 .. n_sb) counts -> exclusive prefixes, sb_off[n_sb] = *n_bools = the total, or SVT_MODES_BAD_GRID */
__global__ __launch_bounds__(256) void svt_mii_scan_kernel(const mii_batch_dev *__restrict__ B) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t s_bad;
    const mii_pic_dev &P = B->pic[blockIdx.x];
    uint32_t          *a = P.sb_off;
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

__global__ __launch_bounds__(64 * MII_EMIT_WAVES) void svt_mii_emit_kernel(const mii_batch_dev *__restrict__ B, const svt_modes_inter_tables *__restrict__ tables) {
    __shared__ uint16_t s_bools[MII_EMIT_WAVES][MII_WAVE_BOOLS];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, sb = (int)blockIdx.x * MII_EMIT_WAVES + wave;
    const mii_pic_dev &P = B->pic[blockIdx.y];
    const svt_tok_geom g = B->g;
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
        const int  cnt = in ? svt_mii_unit_bools(&P.v, &g, r, c, nullptr, nullptr) : 0;
        const int  pre = mii_wave_excl_prefix(cnt, lane);
        total = mii_wave_sum(cnt);
        base = P.sb_off[sb];
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0, q2 = q0; /* the unit's four {first, count, kind} */
        if (cnt) {
            (void)svt_mii_unit_bools(&P.v, &g, r, c, tables, s + pre);
            uint32_t first[3], count[3];
            svt_mi_leaf_tokens(P.v.mi, P.eob_map, P.tok_off, &g, r, c, first, count);
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

} // namespace

extern "C" int32_t svt_hip_modes_inter_set_tables(svt_hip_ctx *ctx, const svt_modes_inter_tables *tables) {
    if (!ctx || !tables) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "modes_inter: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream)); /* (a call in flight may still read the tables) */
    void *d = svt_ctx_slot(ctx, MII_TABLES_SLOT, sizeof(svt_modes_inter_tables));
    if (!d) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "modes_inter: tables");
    HIP_TRY(hipMemcpyAsync(d, tables, sizeof(svt_modes_inter_tables), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_modes_inter_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_modes_inter_picture *pics, int32_t width, int32_t height,
                                                    int32_t mi_stride) {
    if (!ctx || !pics || n_pics < 1 || n_pics > MII_MAX_PICS || width < 8 || height < 8 || width > 8192 || height > 8192 || (width & 7) || (height & 7) ||
        mi_stride < (width >> 3))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "modes_inter: bad argument");
    for (int i = 0; i < n_pics; i++) {
        const svt_modes_inter_picture &p = pics[i];
        if (!p.d_lf_mi || !p.d_mc_mi || !p.d_ext || !p.d_eob_map || !p.d_tok_off || !p.d_segments || !p.d_n_bools || (!p.d_bools && p.capacity))
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "modes_inter: null picture field");
        if (((uintptr_t)p.d_segments & 15) || ((uintptr_t)p.d_bools & 3))
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "modes_inter: d_segments must be 16-byte aligned, d_bools 4-byte aligned");
        const svt_mii_frame f = svt_mii_frame_of(&p);
        if (svt_mii_bad_frame(&f)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "modes_inter: reference_mode above 2, or a compound reference outside 1 .. 3");
    }
    if (!ctx->slot_bytes[MII_TABLES_SLOT]) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "modes_inter: svt_hip_modes_inter_set_tables has not been called");
    HIP_TRY(hipSetDevice(ctx->device));
    mii_batch_dev hb;
    memset(&hb, 0, sizeof hb);
    hb.g.mi_stride = mi_stride; hb.g.mi_rows = height >> 3; hb.g.mi_cols = width >> 3; hb.g.w4 = width >> 2; hb.g.h4 = height >> 2;
    hb.sb_cols = (width + 63) >> 6;
    hb.n_sb = hb.sb_cols * ((height + 63) >> 6);
    uint32_t *sb_off = (uint32_t *)svt_ctx_slot(ctx, MII_SCRATCH_SLOT, sizeof(uint32_t) * (size_t)n_pics * ((size_t)hb.n_sb + 1));
    if (!sb_off) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "modes_inter: scratch");
    for (int i = 0; i < n_pics; i++) {
        const svt_modes_inter_picture &p = pics[i];
        mii_pic_dev &P = hb.pic[i];
        P.v.mi = p.d_lf_mi; P.v.mc = p.d_mc_mi; P.v.ext = p.d_ext; P.v.f = svt_mii_frame_of(&p);
        P.eob_map = p.d_eob_map; P.tok_off = p.d_tok_off; P.bools = p.d_bools; P.segs = (uint4 *)p.d_segments; P.n_bools = p.d_n_bools;
        P.sb_off = sb_off + (size_t)i * ((size_t)hb.n_sb + 1);
        P.capacity = p.capacity;
    }
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof hb, &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "modes_inter: descriptor buffers");
    HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
    memcpy(h, &hb, sizeof hb);
    HIP_TRY(hipMemcpyAsync(d, h, sizeof hb, hipMemcpyHostToDevice, ctx->stream));
    svt_ctx_stage_commit(ctx);
    const mii_batch_dev          *dB = (const mii_batch_dev *)d;
    const svt_modes_inter_tables *dT = (const svt_modes_inter_tables *)ctx->slot[MII_TABLES_SLOT];
    hipLaunchKernelGGL(svt_mii_count_kernel, dim3(n_pics * hb.n_sb), dim3(64), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_mii_scan_kernel, dim3(n_pics), dim3(256), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_mii_emit_kernel, dim3((hb.n_sb + MII_EMIT_WAVES - 1) / MII_EMIT_WAVES, n_pics), dim3(64 * MII_EMIT_WAVES), 0, ctx->stream, dB, dT);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->timed = 1;
    return SVT_HIP_OK;
}

/*
 * tokenize.hip -- coefficient tokenisation of batches of transform blocks and of whole pictures (gfx950).
 *
 * Replaces eb_vp9_tokenize_sb -> tokenize_b (Source/Lib/VPX/vp9_tokenize.c:275-349, 397-430) as eb_vp9_entropy_coding_kernel calls it
 * for every coded block in front of the bool coder (Codec/EbEntropyCodingProcess.c:381-398).
 *
 * The reference walks SBs, blocks and scan positions serially and carries above / left entropy contexts along, but nothing in the walk
 * is a true chain (see rate_kernel.hip): a token depends on its own coefficient, its context on two earlier-scanned neighbours'
 * coefficients, its band on the position; a block emits eob + (eob < n) tokens, so every offset follows from the eob map alone; a
 * block's entropy context is "does the transform block above / left of it have coefficients", which the eob map gives as well.  So:
 *   pass A  svt_tok_count_kernel   one wave per (picture, SB), one lane per 8x8 unit (in z-order = coefficient order): tokens of the SB
 *           svt_tok_scan_kernel    one workgroup per picture: first token of every SB, picture total (written always)
 *   pass B  svt_tok_emit_kernel    one workgroup per run of 8 SBs of a picture: wave 0 repeats the unit analysis, now with the SB's
 *                                  base, writes tok_off (every entry: an offset or SVT_TOK_NONE) and leaves the SB's transform
 *                                  blocks in LDS; then 16 lanes take one block, lane l the scan positions l, l + 16, .. -- one 4-byte store per token to base + c, consecutive
 *                                  lanes consecutive dwords.  4x4 / 8x8 coefficients are staged in LDS with 16-byte loads; the
 *                                  context neighbours are arithmetic on the position (tokenize_core.h), no neighbour table is read.
 * Counts: a histogram private to the workgroup in LDS (two 16-bit bins per dword: a workgroup sees fewer than 65536 tokens), flushed
 * once with one global integer atomic per non-zero bin.  Integer sums: the result does not depend on the order.  Workgroups do not
 * talk to each other: the passes are separate launches in stream order.
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"
#include "tokenize_core.h"
#include "wave_ops.h"

#define TOK_MAX_PICS 32
#define TOK_SB_RUN 8          /* SBs per workgroup of the emit kernel: 8 x 6144 tokens at most (< 65536) */
#define TOK_BLOCK_RUN 64      /* blocks per workgroup of the block-level kernel: a bin receives at most 1003 tokens of a block (band 5 of a 32x32) */
#define TOK_SCAN_ENTRIES (4 * (50 + 194 + 770 + 3074))

namespace {

struct tok_pic_dev {
    const svt_lf_mode_info *mi;
    const int16_t          *q;
    const uint16_t         *eob_map;
    uint32_t               *tokens, *tok_off, *sb_off, *counts;
    uint32_t                capacity, pad_;
};
struct tok_batch_dev {
    tok_pic_dev  pic[TOK_MAX_PICS];
    svt_tok_geom g;
    int32_t      n_sb, sb_cols;
};

/* the (at most) six transform blocks that start in the 8x8 unit `lane` (z-order) of an SB: four luma 4x4 units, one chroma unit per
 * plane.  info[i] = packed description or 0xFFFFFFFF, cnt[i] = tokens */
#define TOK_INFO(k, ptype) ((uint32_t)(k).eob | (uint32_t)(k).ts << 16 | (uint32_t)(k).tt << 18 | (uint32_t)(ptype) << 20 | (uint32_t)(k).inter << 21 | (uint32_t)(k).ctx << 22)
__device__ __forceinline__ void unit_blocks(const tok_pic_dev &P, const svt_tok_geom &g, int sr, int sc, int lane, uint32_t (&info)[6], int (&cnt)[6]) {
    int r, c;
    svt_tok_unit_of(lane, &r, &c);
    const int x8 = sc * 8 + c, y8 = sr * 8 + r;
    _Pragma("unroll") for (int i = 0; i < 6; i++) {
        const int plane = i < 4 ? 0 : i - 3;
        const int x4 = i < 4 ? 2 * x8 + (i & 1) : x8, y4 = i < 4 ? 2 * y8 + (i >> 1) : y8;
        svt_tok_block k;
        info[i] = 0xFFFFFFFFu; cnt[i] = 0;
        if (x8 < g.mi_cols && y8 < g.mi_rows && svt_tok_block_at(P.mi, P.eob_map, &g, plane, x4, y4, &k)) {
            info[i] = TOK_INFO(k, plane != 0);
            cnt[i] = svt_tok_count(&k);
        }
    }
}

__global__ __launch_bounds__(64) void svt_tok_count_kernel(const tok_batch_dev *__restrict__ B) {
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const tok_pic_dev &P = B->pic[pic];
    uint32_t info[6];
    int      cnt[6];
    unit_blocks(P, B->g, sb / B->sb_cols, sb % B->sb_cols, lane, info, cnt);
    const int total = wave_sum(cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4] + cnt[5]);
    if (lane == 0) P.sb_off[sb] = (uint32_t)total;
}

/* in place: a[0 .. n) counts -> exclusive prefixes, a[n] = total.  One workgroup per array (blockIdx.x-th picture, or the one array of
 * the block-level form) */
__device__ __forceinline__ void scan_in_place(uint32_t *a, int n, uint32_t *part) {
    const int t = (int)threadIdx.x, nt = (int)blockDim.x, per = (n + nt - 1) / nt, b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    uint32_t  s = 0;
    for (int i = b; i < e; i++) s += a[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < nt; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int i = b; i < e; i++) { const uint32_t v = a[i]; a[i] = run; run += v; }
    if (t == nt - 1) a[n] = part[nt - 1];
}
__global__ __launch_bounds__(256) void svt_tok_scan_kernel(const tok_batch_dev *__restrict__ B) {
    __shared__ uint32_t part[256];
    scan_in_place(B->pic[blockIdx.x].sb_off, B->n_sb, part);
}
__global__ __launch_bounds__(1024) void svt_tok_block_scan_kernel(const svt_rate_block *__restrict__ blocks, int n_blocks, uint32_t *__restrict__ tok_off) {
    __shared__ uint32_t part[1024];
    for (int i = (int)threadIdx.x; i < n_blocks; i += 1024) {
        const uint32_t w = ((const uint32_t *)(blocks + i))[2];
        const int      eob = (int)(w & 0xffff), n = 16 << (2 * (int)((w >> 16) & 3));
        tok_off[i] = (uint32_t)(eob < n ? eob + 1 : n);
    }
    __syncthreads();
    scan_in_place(tok_off, n_blocks, part);
}

/* the tokens of one block by the 16 lanes of a group.  info: TOK_INFO; out + c is written when off + c < capacity */
__device__ __forceinline__ void emit_block(const int16_t *__restrict__ qg, uint4 *s_q, const int16_t *__restrict__ scan_all, uint32_t info, uint32_t off,
                                           uint32_t *__restrict__ tokens, uint32_t capacity, uint32_t *s_hist, int lane) {
    const int eob = (int)(info & 0xffff), ts = (int)(info >> 16) & 3, tt = (int)(info >> 18) & 3, ptype = (int)(info >> 20) & 1, inter = (int)(info >> 21) & 1,
              ctx0 = (int)(info >> 22) & 3;
    const int n = 16 << (2 * ts);
    const int16_t *scan = scan_all + svt_tok_scan_offset(ts, tt);
    const int16_t *q = qg;
    if (ts <= 1) { /* (no barrier: the 16 lanes of a group sit in one wave, whose LDS accesses are ordered; the wave-scope fence only keeps the
                      compiler from moving the 16-bit reads in front of the 16-byte stores, which it may take for unrelated types) */
        if (eob && lane < (n >> 3)) s_q[lane] = ((const uint4 *)qg)[lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        q = (const int16_t *)s_q;
    }
    for (int c = lane; c <= eob && c < n; c += 16) {
        const uint32_t rec = svt_tok_position(q, scan, c, eob, ts, tt, ptype, inter, ctx0);
        if (off + (uint32_t)c < capacity) tokens[off + c] = rec;
        if (s_hist) {
            const uint32_t bin = SVT_TOK_PROB_ROW(rec) * 12 + SVT_TOK_TOKEN(rec);
            atomicAdd(&s_hist[bin >> 1], 1u << (16 * (bin & 1)));
        }
    }
}
__device__ __forceinline__ void hist_clear(uint32_t *s_hist) {
    for (int i = (int)threadIdx.x; i < SVT_TOK_COUNTS / 2; i += 256) s_hist[i] = 0;
}
__device__ __forceinline__ void hist_flush(const uint32_t *s_hist, uint32_t *__restrict__ counts) {
    for (int i = (int)threadIdx.x; i < SVT_TOK_COUNTS / 2; i += 256) {
        const uint32_t v = s_hist[i];
        if (v & 0xffff) atomicAdd(&counts[2 * i], v & 0xffff);
        if (v >> 16) atomicAdd(&counts[2 * i + 1], v >> 16);
    }
}

__global__ __launch_bounds__(256) void svt_tok_emit_kernel(const tok_batch_dev *__restrict__ B, const int16_t *__restrict__ scan_all) {
    __shared__ uint32_t s_hist[SVT_TOK_COUNTS / 2];
    __shared__ uint4    s_q[16][8];
    __shared__ uint32_t s_info[384], s_off[384], s_coeff[384];
    __shared__ int      s_n;
    const tok_pic_dev &P = B->pic[blockIdx.y];
    const svt_tok_geom g = B->g;
    const int tid = (int)threadIdx.x, grp = tid >> 4, lane = tid & 15;
    uint32_t *hist = P.counts ? s_hist : nullptr;
    if (hist) hist_clear(s_hist);
    const int sb_end = ((int)blockIdx.x + 1) * TOK_SB_RUN < B->n_sb ? ((int)blockIdx.x + 1) * TOK_SB_RUN : B->n_sb;
    for (int sb = (int)blockIdx.x * TOK_SB_RUN; sb < sb_end; sb++) {
        if (tid == 0) s_n = 0;
        __syncthreads();
        if (tid < 64) {
            uint32_t info[6];
            int      cnt[6];
            unit_blocks(P, g, sb / B->sb_cols, sb % B->sb_cols, tid, info, cnt);
            const int cy = cnt[0] + cnt[1] + cnt[2] + cnt[3];
            const int tot_y = wave_sum(cy), tot_u = wave_sum(cnt[4]);
            uint32_t  off[6];
            off[0] = P.sb_off[sb] + (uint32_t)wave_excl_prefix(cy, tid);
            off[1] = off[0] + cnt[0]; off[2] = off[1] + cnt[1]; off[3] = off[2] + cnt[2];
            off[4] = P.sb_off[sb] + (uint32_t)(tot_y + wave_excl_prefix(cnt[4], tid));
            off[5] = P.sb_off[sb] + (uint32_t)(tot_y + tot_u + wave_excl_prefix(cnt[5], tid));
            int r, c;
            svt_tok_unit_of(tid, &r, &c);
            const int x8 = (sb % B->sb_cols) * 8 + c, y8 = (sb / B->sb_cols) * 8 + r;
            /* every entry of tok_off belongs to exactly one unit of the picture: the unit writes all six of its entries, so the map needs no clearing pass */
            if (x8 < g.mi_cols && y8 < g.mi_rows) _Pragma("unroll") for (int i = 0; i < 6; i++) {
                const int plane = i < 4 ? 0 : i - 3, pw4 = plane ? g.w4 >> 1 : g.w4;
                const int x4 = i < 4 ? 2 * x8 + (i & 1) : x8, y4 = i < 4 ? 2 * y8 + (i >> 1) : y8;
                P.tok_off[svt_tok_map_offset(&g, plane) + y4 * pw4 + x4] = info[i] != 0xFFFFFFFFu ? off[i] : SVT_TOK_NONE;
                if (info[i] != 0xFFFFFFFFu) {
                    const int slot = atomicAdd(&s_n, 1);
                    s_info[slot] = info[i]; s_off[slot] = off[i];
                    s_coeff[slot] = (uint32_t)sb * SVT_SB_COEFFS + (plane == 0 ? (uint32_t)(tid * 4 + i) * 16u : (plane == 1 ? 4096u : 5120u) + (uint32_t)tid * 16u);
                }
            }
        }
        __syncthreads();
        const int n_blk = s_n;
        for (int b = grp; b < n_blk; b += 16) emit_block(P.q + s_coeff[b], s_q[grp], scan_all, s_info[b], s_off[b], P.tokens, P.capacity, hist, lane);
        __syncthreads();
    }
    if (hist) hist_flush(s_hist, P.counts);
}

__global__ __launch_bounds__(256) void svt_tok_blocks_kernel(const int16_t *__restrict__ qcoeff, const svt_rate_block *__restrict__ blocks, int n_blocks,
                                                             const int16_t *__restrict__ scan_all, const uint32_t *__restrict__ tok_off, uint32_t *__restrict__ tokens,
                                                             uint32_t capacity, uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_hist[SVT_TOK_COUNTS / 2];
    __shared__ uint4    s_q[16][8];
    const int tid = (int)threadIdx.x, grp = tid >> 4, lane = tid & 15;
    uint32_t *hist = counts ? s_hist : nullptr;
    if (hist) { hist_clear(s_hist); __syncthreads(); }
    for (int it = 0; it < TOK_BLOCK_RUN / 16; it++) {
        const int b = (int)blockIdx.x * TOK_BLOCK_RUN + it * 16 + grp;
        if (b < n_blocks) {
            const uint4 kw = *(const uint4 *)(blocks + b);
            const int   ts = (int)(kw.z >> 16) & 3, n = 16 << (2 * ts);
            const int   tt = ((int)kw.y - svt_tok_scan_offset(ts, 0)) / (3 * n + 2) & 3; /* canonical layout: the table names the transform type */
            int         eob = (int)(kw.z & 0xffff);
            eob = eob < n ? eob : n;
            const uint32_t info = (uint32_t)eob | (uint32_t)ts << 16 | (uint32_t)tt << 18 | ((kw.z >> 24) & 1u) << 20 | (kw.w & 1u) << 21 | ((kw.w >> 8) & 3u) << 22;
            emit_block(qcoeff + kw.x, s_q[grp], scan_all, info, tok_off[b], tokens, capacity, hist, lane);
        }
    }
    if (hist) { __syncthreads(); hist_flush(s_hist, counts); }
}

/* the canonical scan array on the device: uploaded once per context */
const int16_t *device_scan(svt_hip_ctx *ctx) {
    const bool first = ctx->slot_bytes[SVT_SLOT_TOK_SCAN] == 0;
    int16_t   *d = (int16_t *)svt_ctx_slot(ctx, SVT_SLOT_TOK_SCAN, sizeof(int16_t) * TOK_SCAN_ENTRIES);
    if (!d) return nullptr;
    if (first) {
        int32_t        entries = 0;
        const int16_t *h = svt_hip_vp9_scan_tables(nullptr, &entries);
        if (entries != TOK_SCAN_ENTRIES || hipMemcpyAsync(d, h, sizeof(int16_t) * TOK_SCAN_ENTRIES, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            ctx->slot_bytes[SVT_SLOT_TOK_SCAN] = 0; /* (the buffer stays; the next call uploads again) */
            (void)hipFree(ctx->slot[SVT_SLOT_TOK_SCAN]);
            ctx->slot[SVT_SLOT_TOK_SCAN] = nullptr;
            return nullptr;
        }
    }
    return d;
}

} // namespace

extern "C" int32_t svt_hip_tokenize_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_tok_picture *pics, int32_t width, int32_t height, int32_t mi_stride) {
    tok_batch_dev hb;
    memset(&hb, 0, sizeof hb);
    if (!ctx || !pics || n_pics < 1 || n_pics > TOK_MAX_PICS || svt_tok_geom_of(width, height, mi_stride, &hb.g, &hb.sb_cols, &hb.n_sb))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tokenize: bad argument");
    for (int i = 0; i < n_pics; i++) {
        const svt_tok_picture &p = pics[i];
        if (!p.d_lf_mi || !p.d_qcoeff || !p.d_eob_map || !p.d_tok_off || !p.d_sb_off || (!p.d_tokens && p.capacity))
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tokenize: null picture field");
        if ((uintptr_t)p.d_qcoeff & 15) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tokenize: coefficient arrays must be 16-byte aligned");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const int16_t *d_scan = device_scan(ctx);
    if (!d_scan) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "tokenize: scan tables");
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    for (int i = 0; i < n_pics; i++) {
        const svt_tok_picture &p = pics[i];
        tok_pic_dev &P = hb.pic[i];
        P.mi = p.d_lf_mi; P.q = p.d_qcoeff; P.eob_map = p.d_eob_map; P.tokens = p.d_tokens; P.tok_off = p.d_tok_off; P.sb_off = p.d_sb_off; P.counts = p.d_counts;
        P.capacity = p.capacity;
        if (p.d_counts) HIP_TRY(hipMemsetAsync(p.d_counts, 0, SVT_TOK_COUNTS * sizeof(uint32_t), ctx->stream));
    }
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof hb, &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "tokenize: descriptor buffers");
    memcpy(h, &hb, sizeof hb);
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof hb));
    const tok_batch_dev *dB = (const tok_batch_dev *)d;
    hipLaunchKernelGGL(svt_tok_count_kernel, dim3(n_pics * hb.n_sb), dim3(64), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_tok_scan_kernel, dim3(n_pics), dim3(256), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_tok_emit_kernel, dim3((hb.n_sb + TOK_SB_RUN - 1) / TOK_SB_RUN, n_pics), dim3(256), 0, ctx->stream, dB, d_scan);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_tokenize_blocks_device(svt_hip_ctx *ctx, const int16_t *d_qcoeff, const svt_rate_block *d_blocks, int32_t n_blocks, uint32_t *d_tokens,
                                                  uint32_t capacity, uint32_t *d_tok_off, uint32_t *d_counts) {
    if (!ctx || !d_qcoeff || !d_blocks || n_blocks < 1 || !d_tok_off || (!d_tokens && capacity)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tokenize: null argument");
    if (((uintptr_t)d_blocks & 15) || ((uintptr_t)d_qcoeff & 15)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tokenize: block / coefficient arrays must be 16-byte aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    const int16_t *d_scan = device_scan(ctx);
    if (!d_scan) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "tokenize: scan tables");
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    if (d_counts) HIP_TRY(hipMemsetAsync(d_counts, 0, SVT_TOK_COUNTS * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(svt_tok_block_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_blocks, n_blocks, d_tok_off);
    hipLaunchKernelGGL(svt_tok_blocks_kernel, dim3((n_blocks + TOK_BLOCK_RUN - 1) / TOK_BLOCK_RUN), dim3(256), 0, ctx->stream, d_qcoeff, d_blocks, n_blocks, d_scan,
                       (const uint32_t *)d_tok_off, d_tokens, capacity, d_counts);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_tokenize_blocks(svt_hip_ctx *ctx, const int16_t *qcoeff, size_t coeff_count, const svt_rate_block *blocks, int32_t n_blocks, uint32_t *tokens,
                                           uint32_t capacity, uint32_t *tok_off, uint32_t *counts) {
    if (!ctx || !qcoeff || !blocks || n_blocks < 1 || !tok_off || (!tokens && capacity)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tokenize: null argument");
    for (int i = 0; i < n_blocks; i++) {
        const size_t   n = (size_t)16 << (2 * blocks[i].tx_size);
        const uint32_t first = blocks[i].tx_size > 3 ? 0 : (uint32_t)svt_tok_scan_offset(blocks[i].tx_size, 0);
        if (blocks[i].tx_size > 3 || blocks[i].plane_type > 1 || blocks[i].is_inter > 1 || blocks[i].ctx > 2 || blocks[i].eob > n || blocks[i].coeff_off + n > coeff_count ||
            (blocks[i].coeff_off & 7) || blocks[i].scan_off < first || (blocks[i].scan_off - first) % (3 * n + 2) || (blocks[i].scan_off - first) / (3 * n + 2) > 3)
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tokenize: bad block (scan_off must name a table of the canonical layout)");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    int16_t        *dq = (int16_t *)svt_ctx_slot(ctx, SVT_SLOT_TOK_QCOEFF, sizeof(int16_t) * coeff_count);
    svt_rate_block *db = (svt_rate_block *)svt_ctx_slot(ctx, SVT_SLOT_TOK_BLOCKS, sizeof(svt_rate_block) * (size_t)n_blocks);
    uint32_t       *dt = (uint32_t *)svt_ctx_slot(ctx, SVT_SLOT_TOK_TOKENS, sizeof(uint32_t) * ((size_t)capacity + 1));
    uint32_t       *doff = (uint32_t *)svt_ctx_slot(ctx, SVT_SLOT_TOK_OFF, sizeof(uint32_t) * ((size_t)n_blocks + 1));
    uint32_t       *dc = (uint32_t *)svt_ctx_slot(ctx, SVT_SLOT_TOK_COUNTS, sizeof(uint32_t) * SVT_TOK_COUNTS);
    if (!dq || !db || !dt || !doff || !dc) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "tokenize: device buffers");
    HIP_TRY(hipMemcpyAsync(dq, qcoeff, sizeof(int16_t) * coeff_count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(db, blocks, sizeof(svt_rate_block) * (size_t)n_blocks, hipMemcpyHostToDevice, ctx->stream));
    const int32_t rc = svt_hip_tokenize_blocks_device(ctx, dq, db, n_blocks, dt, capacity, doff, counts ? dc : nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(tok_off, doff, sizeof(uint32_t) * ((size_t)n_blocks + 1), hipMemcpyDeviceToHost, ctx->stream));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, dc, sizeof(uint32_t) * SVT_TOK_COUNTS, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t got = tok_off[n_blocks] < capacity ? tok_off[n_blocks] : capacity;
    if (got) {
        HIP_TRY(hipMemcpyAsync(tokens, dt, sizeof(uint32_t) * got, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return SVT_HIP_OK;
}

/*
 * intra_search.hip -- open-loop intra search (OIS) of a picture (gfx950) and the stand-in intra decision built on its records.
 *
 * svt_ois_kernel: the per-block, per-mode cost of every VP9 intra predictor from the SOURCE samples (include/svtvp9_hip.h states the
 * rules).  Nothing depends on a reconstruction, so every SB is independent: one workgroup (four waves) per SB.  The SB's source -- 64x64
 * luma and two 32x32 chroma blocks, plus the row above, the column to the left and the corner, with the picture-edge constants of the
 * intra pass already in place (127 above the picture, 129 left of it) -- is staged in LDS once; every block then builds its reference
 * samples (the e[] layout of intra_pred_row, intra_pred.h) from the staged samples, in two phases that share one edge buffer (4x4 luma
 * blocks; then 8x8 .. 32x32 luma and every chroma block).  A lane owns one row of one block (for chroma: one row of the Cb or the Cr
 * block, the two planes side by side), keeps its source row in registers and runs the ten predictors over it: intra_pred_row builds the
 * packed prediction row, v_sad_u8 takes its SAD, a butterfly over the block's lanes (N lanes, 2N for chroma: SAD_Cb + SAD_Cr) sums the
 * rows.  The mode is uniform over the wave (one branch per mode).  The minimum over the modes is kept in a register as (sad << 4 | mode):
 * ties go to the lowest mode index by construction.  Every (block, size) is owned by exactly one lane group, so the result goes to LDS
 * with a plain store and the records leave the workgroup together.
 *
 * svt_md_intra_search_kernel: the decision of encdec_core.h (svt_md_intra_search_unit, the same text as the host form) for one SB per
 * wave, one lane per 8x8 unit, from the SB's records staged in LDS.
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"
#include "encdec_core.h"
#include "intra_pred.h"

namespace {

constexpr int OIS_THREADS = 256;
constexpr int OIS_YS = 72, OIS_CS = 40; /* staged row strides: sample (row, col), row / col from -1, at (row + 1) * S + col + 4 (rows dword-aligned) */
constexpr int OIS_EDGE = 7168;          /* the larger phase: 4 x 32x32, 16 x 16x16, 64 x 8x8 luma + 2 x (4 x 16x16, 16 x 8x8, 64 x 4x4) chroma */
constexpr int OIS_CBEST = SVT_OIS_PER_SB; /* chroma results after the luma ones: 16x16 at +0, 8x8 at +4, 4x4 at +20 */

struct ois_lds {
    uint8_t  y[65 * OIS_YS];
    uint8_t  c[2][33 * OIS_CS];
    uint8_t  edge[OIS_EDGE]; /* reference samples of every block of a phase: a slot of 4N bytes per block, B(-N) .. B(2N) */
    uint32_t best[SVT_OIS_PER_SB + 84]; /* sad << 4 | mode, or UINT32_MAX outside the picture */
};
static_assert(sizeof(ois_lds) <= 16384, "the search shares its CU with other work: at most 16 KB of LDS per workgroup");

/* the even bits of a z-order index, compacted (x of the block; x of (b >> 1) is its y) */
__device__ __forceinline__ int ois_deint(int v) {
    v &= 0x55;
    v = (v | (v >> 1)) & 0x33;
    return (v | (v >> 2)) & 0x0f;
}

/* slot of block b (z-order) of size N in plane 0 (luma) or 1 / 2 (chroma); luma 4x4 blocks have a phase of their own */
template <int N, bool CH> __device__ __forceinline__ int ois_slot(int plane, int b) {
    if (!CH) return (N == 4 || N == 32 ? 0 : N == 16 ? 512 : 1536) + b * 4 * N;
    return (N == 16 ? 3584 : N == 8 ? 4096 : 5120) + (plane - 1) * (32 / N) * (32 / N) * 4 * N + b * 4 * N;
}
template <int N, bool CH> __device__ __forceinline__ int ois_best_index(int b) {
    if (!CH) return (N == 32 ? 0 : N == 16 ? 4 : N == 8 ? 20 : 84) + b;
    return OIS_CBEST + (N == 16 ? 0 : N == 8 ? 4 : 20) + b;
}

/* reference samples of the N x N block at (bx, by) of the SB's staged plane, as generate_intra_reference_samples builds them for a block
 * inside the picture (the picture-edge constants are in the staged border): slot[k + N] = B(k), k = -N .. 2N */
__device__ __forceinline__ void ois_build_edge(const ois_lds &L, int plane, int n, int bx, int by, int have_right, uint8_t *slot) {
    const uint8_t *P = plane ? L.c[plane - 1] : L.y;
    const int      S = plane ? OIS_CS : OIS_YS;
    auto at = [&](int row, int col) { return P[(row + 1) * S + col + 4]; };
    for (int j = 0; j <= 3 * n; j++) {
        const int k = j - n;
        slot[j] = k < 0 ? at(by - k - 1, bx - 1) : (k <= n || have_right) ? at(by - 1, bx + k - 1) : at(by - 1, bx + n - 1);
    }
}

/* one wave: 64 rows of the blocks of size N (luma, or chroma with Cb and Cr side by side), all ten modes */
template <int N, bool CH> __device__ __forceinline__ void ois_task(ois_lds &L, int task, int sx, int sy, int width, int height, int lane) {
    constexpr int G = CH ? 2 * N : N; /* lanes of one block */
    const int q = task * 64 + lane, b = q / G, g = q % G, plane = CH ? 1 + g / N : 0, r = g % N;
    const int bx = ois_deint(b) * N, by = ois_deint(b >> 1) * N;
    const int px = (CH ? sx >> 1 : sx) + bx, py = (CH ? sy >> 1 : sy) + by;
    const bool inside = px + N <= (CH ? width >> 1 : width) && py + N <= (CH ? height >> 1 : height);
    const uint8_t *P = plane ? L.c[plane - 1] : L.y;
    const int      S = plane ? OIS_CS : OIS_YS;
    const uint32_t *sp = (const uint32_t *)(P + (by + r + 1) * S + bx + 4);
    uint32_t        srow[N / 4];
    _Pragma("unroll") for (int k = 0; k < N / 4; k++) srow[k] = sp[k];
    const int      eo = ois_slot<N, CH>(plane, b) + N - 32; /* e[k + 32] = B(k) */
    uint32_t       best = 0xFFFFFFFFu;
    _Pragma("unroll 1") for (int mode = 0; mode < 10; mode++) {
        /* (the offset and the row are opaque to the compiler inside the loop: what depends on them alone -- reference-sample loads,
           per-sample lane masks -- is not hoisted out of the mode loop, where it held ~100 VGPRs and spilled SGPRs of a 32x32 row) */
        int eom = eo, rm = r;
        asm volatile("" : "+v"(eom), "+v"(rm));
        const uint8_t *e = L.edge + eom;
        uint32_t prow[N / 4];
        intra_pred_row<N>(e, mode, rm, px > 0, py > 0, prow);
        uint32_t sad = 0;
        _Pragma("unroll") for (int k = 0; k < N / 4; k++) sad = __builtin_amdgcn_sad_u8(prow[k], srow[k], sad);
        _Pragma("unroll") for (int m = 1; m < G; m <<= 1) sad += (uint32_t)__shfl_xor((int)sad, m);
        const uint32_t key = sad << 4 | (uint32_t)mode;
        best = key < best ? key : best;
    }
    if (g == 0) L.best[ois_best_index<N, CH>(b)] = inside ? best : 0xFFFFFFFFu;
}

/* the search of SB `sb` of one picture by one workgroup.  WITH_4X4 = false leaves phase 1 out (the 256 luma 4x4 blocks, 16 of the 44 wave
 * tasks): records 84 .. 339 are then written as "none" */
template <bool WITH_4X4>
__device__ __forceinline__ void ois_sb(ois_lds &L, const uint8_t *__restrict__ src_y, const uint8_t *__restrict__ src_u, const uint8_t *__restrict__ src_v,
                                       int y_stride, int uv_stride, int width, int height, int sb_cols, int sb, uint32_t *__restrict__ out) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sx = (sb % sb_cols) * 64, sy = (sb / sb_cols) * 64;
    /* stage the SB with its border: 127 above the picture (the corner too), 129 left of it (and the corner below the picture's top row),
       0 outside the picture on the right / bottom (only blocks that are not inside read it; their records are discarded) */
    for (int i = tid; i < 65 * 65; i += OIS_THREADS) {
        const int row = i / 65 - 1, col = i % 65 - 1, x = sx + col, y = sy + row;
        uint8_t   v;
        if (row < 0) v = sy == 0 ? 127 : (col < 0 && sx == 0) ? 129 : x < width ? src_y[(size_t)y * y_stride + x] : 0;
        else if (col < 0) v = sx == 0 ? 129 : y < height ? src_y[(size_t)y * y_stride + x] : 0;
        else v = x < width && y < height ? src_y[(size_t)y * y_stride + x] : 0;
        L.y[(row + 1) * OIS_YS + col + 4] = v;
    }
    {
        const int cx = sx >> 1, cy = sy >> 1, cw = width >> 1, ch = height >> 1;
        for (int i = tid; i < 2 * 33 * 33; i += OIS_THREADS) {
            const int      p = i / (33 * 33), j = i % (33 * 33), row = j / 33 - 1, col = j % 33 - 1, x = cx + col, y = cy + row;
            const uint8_t *s = p ? src_v : src_u;
            uint8_t        v;
            if (row < 0) v = cy == 0 ? 127 : (col < 0 && cx == 0) ? 129 : x < cw ? s[(size_t)y * uv_stride + x] : 0;
            else if (col < 0) v = cx == 0 ? 129 : y < ch ? s[(size_t)y * uv_stride + x] : 0;
            else v = x < cw && y < ch ? s[(size_t)y * uv_stride + x] : 0;
            L.c[p][(row + 1) * OIS_CS + col + 4] = v;
        }
    }
    __syncthreads();
    /* phase 1: the 256 luma 4x4 blocks (one per thread builds its samples; a block in the left half of its 8x8 unit reads the true
       above-right samples) */
    if (WITH_4X4) {
        {
            const int b = tid, x4 = ois_deint(b);
            ois_build_edge(L, 0, 4, 4 * x4, 4 * ois_deint(b >> 1), !(x4 & 1), L.edge + b * 16);
        }
        __syncthreads();
        for (int t = wave; t < 16; t += OIS_THREADS / 64) ois_task<4, false>(L, t, sx, sy, width, height, lane);
        __syncthreads();
    }
    /* phase 2: 4 + 16 + 64 luma blocks of 32x32 / 16x16 / 8x8 and 2 x (4 + 16 + 64) chroma blocks (252 threads, one block each) */
    if (tid < 252) {
        int plane = 0, n, b, off;
        if (tid < 4) { n = 32; b = tid; off = ois_slot<32, false>(0, b); }
        else if (tid < 20) { n = 16; b = tid - 4; off = ois_slot<16, false>(0, b); }
        else if (tid < 84) { n = 8; b = tid - 20; off = ois_slot<8, false>(0, b); }
        else if (tid < 92) { n = 16; plane = 1 + (tid - 84) / 4; b = (tid - 84) % 4; off = ois_slot<16, true>(plane, b); }
        else if (tid < 124) { n = 8; plane = 1 + (tid - 92) / 16; b = (tid - 92) % 16; off = ois_slot<8, true>(plane, b); }
        else { n = 4; plane = 1 + (tid - 124) / 64; b = (tid - 124) % 64; off = ois_slot<4, true>(plane, b); }
        ois_build_edge(L, plane, n, n * ois_deint(b), n * ois_deint(b >> 1), 0, L.edge + off);
    }
    __syncthreads();
    /* 28 wave tasks of 64 rows, the long ones first and spread over the four waves (a task costs ~N samples per lane and mode) */
    for (int t = wave; t < 28; t += OIS_THREADS / 64) {
        if (t < 2) ois_task<32, false>(L, t, sx, sy, width, height, lane);
        else if (t < 4) ois_task<16, true>(L, t - 2, sx, sy, width, height, lane);
        else if (t < 8) ois_task<16, false>(L, t - 4, sx, sy, width, height, lane);
        else if (t < 12) ois_task<8, true>(L, t - 8, sx, sy, width, height, lane);
        else if (t < 20) ois_task<8, false>(L, t - 12, sx, sy, width, height, lane);
        else ois_task<4, true>(L, t - 20, sx, sy, width, height, lane);
    }
    __syncthreads();
    /* the SB's records: three dwords each (sad, uv_sad, mode | uv_mode << 8) */
    uint32_t *o = out + (size_t)sb * SVT_OIS_PER_SB * 3;
    for (int i = tid; i < SVT_OIS_PER_SB; i += OIS_THREADS) {
        const uint32_t y = WITH_4X4 || i < 84 ? L.best[i] : 0xFFFFFFFFu;
        const uint32_t c = i < 84 ? L.best[OIS_CBEST + (i < 4 ? i : i < 20 ? 4 + (i - 4) : 20 + (i - 20))] : 0xFFFFFFFFu;
        o[3 * i + 0] = y == 0xFFFFFFFFu ? y : y >> 4;
        o[3 * i + 1] = c == 0xFFFFFFFFu ? c : c >> 4;
        o[3 * i + 2] = (y == 0xFFFFFFFFu ? 0xFFu : (y & 15u)) | (c == 0xFFFFFFFFu ? 0xFFu : (c & 15u)) << 8;
    }
}

__global__ __launch_bounds__(OIS_THREADS) void svt_ois_kernel(const uint8_t *__restrict__ src_y, const uint8_t *__restrict__ src_u, const uint8_t *__restrict__ src_v,
                                                              int y_stride, int uv_stride, int width, int height, int sb_cols, uint32_t *__restrict__ out) {
    __shared__ ois_lds L;
    ois_sb<true>(L, src_y, src_u, src_v, y_stride, uv_stride, width, height, sb_cols, (int)blockIdx.x, out);
}

/* several pictures of one geometry in one launch: workgroup (picture, SB), the picture's planes and records from the staged descriptor */
constexpr int OIS_MAX_PICS = 32;
struct ois_pic_dev {
    const uint8_t *y, *u, *v;
    uint32_t      *out;
    int32_t        y_stride, uv_stride;
};
struct ois_batch_dev {
    ois_pic_dev pic[OIS_MAX_PICS];
    int32_t     n_sb, sb_cols, width, height;
};
template <bool WITH_4X4> __global__ __launch_bounds__(OIS_THREADS) void svt_ois_batch_kernel(const ois_batch_dev *__restrict__ B) {
    __shared__ ois_lds L;
    const int          pic = (int)blockIdx.x / B->n_sb, sb = (int)blockIdx.x % B->n_sb;
    const ois_pic_dev &P = B->pic[pic];
    ois_sb<WITH_4X4>(L, P.y, P.u, P.v, P.y_stride, P.uv_stride, B->width, B->height, B->sb_cols, sb, P.out);
}

/* stand-in intra decision: one wave per SB, one lane per 8x8 unit, the SB's records in LDS */
__global__ __launch_bounds__(64) void svt_md_intra_search_kernel(const svt_ois_block *__restrict__ ois, int sb_cols, int mi_rows, int mi_cols, uint32_t lambda,
                                                                 int filter_level, svt_lf_mode_info *__restrict__ mi, int mi_stride) {
    __shared__ svt_ois_block s[SVT_OIS_PER_SB];
    const int sb = (int)blockIdx.x, lane = (int)threadIdx.x;
    {
        const uint32_t *g = (const uint32_t *)(ois + (size_t)sb * SVT_OIS_PER_SB);
        uint32_t       *d = (uint32_t *)s;
        for (int i = lane; i < SVT_OIS_PER_SB * 3; i += 64) d[i] = g[i];
    }
    __syncthreads();
    const int r = lane >> 3, c = lane & 7, sr = sb / sb_cols, sc = sb % sb_cols, ur = sr * 8 + r, uc = sc * 8 + c;
    if (ur >= mi_rows || uc >= mi_cols) return;
    svt_lf_mode_info m;
    svt_md_intra_search_unit(s, r, c, sr, sc, mi_rows, mi_cols, lambda, filter_level, &m);
    mi[ur * mi_stride + uc] = m;
}

} // namespace

extern "C" int32_t svt_hip_intra_search_device(svt_hip_ctx *ctx, const svt_yuv_planes *src, int32_t width, int32_t height, svt_ois_block *d_out) {
    if (!ctx || !src || !src->y || !src->u || !src->v || !d_out || width < 8 || height < 8 || (width & 7) || (height & 7) || src->y_stride < width ||
        src->uv_stride < (width >> 1) || ((uintptr_t)d_out & 3))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "intra_search: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    const int sb_cols = (width + 63) >> 6, n_sb = sb_cols * ((height + 63) >> 6);
    hipLaunchKernelGGL(svt_ois_kernel, dim3(n_sb), dim3(OIS_THREADS), 0, ctx->stream, (const uint8_t *)src->y, (const uint8_t *)src->u, (const uint8_t *)src->v,
                       src->y_stride, src->uv_stride, width, height, sb_cols, (uint32_t *)d_out);
    HIP_TRY(hipGetLastError());
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_intra_search_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_yuv_planes *srcs, int32_t width, int32_t height, int32_t with_4x4,
                                                     svt_ois_block *const *d_out) {
    if (!ctx || n_pics < 1 || !srcs || !d_out || width < 8 || height < 8 || (width & 7) || (height & 7) || (with_4x4 != 0 && with_4x4 != 1))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "intra_search_batch: bad argument");
    for (int i = 0; i < n_pics; i++) /* (every picture is looked at before anything is launched) */
        if (!srcs[i].y || !srcs[i].u || !srcs[i].v || !d_out[i] || srcs[i].y_stride < width || srcs[i].uv_stride < (width >> 1) || ((uintptr_t)d_out[i] & 3))
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "intra_search_batch: bad picture");
    HIP_TRY(hipSetDevice(ctx->device));
    const int sb_cols = (width + 63) >> 6, n_sb = sb_cols * ((height + 63) >> 6);
    for (int first = 0; first < n_pics; first += OIS_MAX_PICS) {
        const int n = n_pics - first < OIS_MAX_PICS ? n_pics - first : OIS_MAX_PICS;
        void     *h = nullptr, *d = nullptr;
        if (svt_ctx_stage(ctx, sizeof(ois_batch_dev), &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "intra_search_batch: descriptor buffers");
        ois_batch_dev *hb = (ois_batch_dev *)h;
        memset(hb, 0, sizeof *hb);
        hb->n_sb = n_sb; hb->sb_cols = sb_cols; hb->width = width; hb->height = height;
        for (int i = 0; i < n; i++) {
            const svt_yuv_planes &s = srcs[first + i];
            hb->pic[i].y = s.y; hb->pic[i].u = s.u; hb->pic[i].v = s.v; hb->pic[i].out = (uint32_t *)d_out[first + i];
            hb->pic[i].y_stride = s.y_stride; hb->pic[i].uv_stride = s.uv_stride;
        }
        HIP_TRY(svt_ctx_stage_send(ctx, sizeof(ois_batch_dev)));
        if (with_4x4) hipLaunchKernelGGL(svt_ois_batch_kernel<true>, dim3(n * n_sb), dim3(OIS_THREADS), 0, ctx->stream, (const ois_batch_dev *)d);
        else hipLaunchKernelGGL(svt_ois_batch_kernel<false>, dim3(n * n_sb), dim3(OIS_THREADS), 0, ctx->stream, (const ois_batch_dev *)d);
        HIP_TRY(hipGetLastError());
    }
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_md_intra_search_device(svt_hip_ctx *ctx, const svt_ois_block *d_ois, int32_t width, int32_t height, uint32_t lambda, int32_t filter_level,
                                                  svt_lf_mode_info *d_lf_mi, int32_t mi_stride) {
    if (!ctx || !d_ois || !d_lf_mi || width < 8 || height < 8 || (width & 7) || (height & 7) || mi_stride < (width >> 3) || filter_level < 0 || filter_level > 63 ||
        ((uintptr_t)d_ois & 3))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_intra_search: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    const int sb_cols = (width + 63) >> 6, n_sb = sb_cols * ((height + 63) >> 6);
    hipLaunchKernelGGL(svt_md_intra_search_kernel, dim3(n_sb), dim3(64), 0, ctx->stream, d_ois, sb_cols, height >> 3, width >> 3, lambda, filter_level, d_lf_mi, mi_stride);
    HIP_TRY(hipGetLastError());
    return SVT_HIP_OK;
}

/* host form of svt_hip_md_intra_search_device (the same text) */
extern "C" int32_t svt_hip_md_intra_search_picture(const svt_ois_block *ois, int32_t width, int32_t height, uint32_t lambda, int32_t filter_level,
                                                   svt_lf_mode_info *lf_mi, int32_t mi_stride) {
    if (!ois || !lf_mi || width < 8 || height < 8 || (width & 7) || (height & 7) || mi_stride < (width >> 3) || filter_level < 0 || filter_level > 63)
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_intra_search: bad argument");
    const int mi_rows = height >> 3, mi_cols = width >> 3, sb_cols = (width + 63) >> 6, sb_rows = (height + 63) >> 6;
    for (int sr = 0; sr < sb_rows; sr++)
        for (int sc = 0; sc < sb_cols; sc++)
            for (int u = 0; u < 64; u++) {
                const int r = u >> 3, c = u & 7, ur = sr * 8 + r, uc = sc * 8 + c;
                if (ur >= mi_rows || uc >= mi_cols) continue;
                svt_md_intra_search_unit(ois + (size_t)(sr * sb_cols + sc) * SVT_OIS_PER_SB, r, c, sr, sc, mi_rows, mi_cols, lambda, filter_level,
                                         &lf_mi[ur * mi_stride + uc]);
            }
    return SVT_HIP_OK;
}

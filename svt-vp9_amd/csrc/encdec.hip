/*
 * encdec.hip -- picture-level EncDec driver (gfx950): everything the encode pass does with mode decision's output, for a batch of
 * mutually independent pictures, device resident from the mode-info grid to the padded reference picture.
 *
 * Replaces the data path of eb_vp9_enc_dec_kernel behind mode decision (Source/Lib/Codec/EbEncDecProcess.c:5306):
 *   encode_pass_sb (:3627-4241): inter prediction (:3787-3802)  -> svt_mc_kernel
 *                                perform_coding_loop per block   -> svt_tq_kernel<N> over lists built here from the grid
 *                                skip flags (:4069-4098)         -> svt_tq_skip_kernel + svt_skip_update_kernel
 *   last SB of the picture (:5625-5697): eb_vp9_build_mask_frame -> svt_lf_mask_kernel (device form of svt_hip_lf_build_masks)
 *                                eb_vp9_loop_filter_frame        -> svt_lf_kernel
 *                                pad_ref_and_set_flags           -> svt_refpad_kernel
 * The reference walks SBs and blocks one at a time on the host; here the host only enqueues: the block lists, skip flags and
 * filter masks are derived on the device from the grid (rules: encdec_core.h, shared with the host forms the CPU tests pin), so a
 * picture costs no per-block descriptor traffic over PCIe and no host wait between the stages.
 *
 * List building is three small kernels: count (one wave per SB, one lane per 8x8 unit; per-SB totals per transform size), an
 * exclusive scan over [size][picture][SB] (one workgroup), emit (same mapping; a lane's place inside its SB comes from a wave
 * prefix sum).  The order is deterministic: size, picture, SB raster, unit raster, luma / Cb / Cr -- SB-ordered inside a size, so
 * the blocks a wave of the transform kernel takes lie next to each other in the planes.  These kernels move a few MB per picture
 * and are bound by launch latency, not by bandwidth; they exist to keep the chain on the device.
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "svt_ctx.h"
#include "encdec_core.h"
#include "wave_ops.h"

#define ED_MAX_PICS 32
#define ED_MAX_SETS 8 /* reconstruction base pointers a transform launch can address (svt_tq_block.pad_[0] bits 4-6) */

struct svt_encdec_work {
    int           max_pics, width, height, n_sb, sb_cols, mi_rows, mi_cols;
    size_t        cap_per_pic;   /* transform blocks of a picture at most: all 4x4 */
    svt_tq_block *d_blocks;      /* only when a host asks for the descriptor list (svt_hip_encdec_work_download): allocated and filled then */
    void         *last_hb;       /* host copy of the latest batch's parameter block (for that) */
    uint32_t     *d_pos;
    uint16_t     *d_eob;
    int32_t      *d_counts;      /* [4][max_pics][n_sb], turned into offsets by the scan */
    int32_t      *d_totals, *d_bases; /* [4][max_pics]: blocks of a (size, picture) / its first block */
    int32_t      *d_off_cnt;     /* [8]: first block / number of blocks per size */
    int32_t      *d_status;      /* = d_off_cnt + 8 (svt_hip_encdec_work_status reads both in one copy); != 0: a malformed grid was seen */
    int32_t      *d_intra_sync;  /* ticket and per-(plane, 16x16 cell) flags of the intra kernel: 2 + 3 * (at most 16 per SB) dwords */
    svt_quant_tables *d_qtabs;   /* [2] luma, chroma of the batch's q index */
    int16_t      *d_iscan;
    svt_encdec_stage_hook hook;  /* profiling aid: called on the enqueueing thread at every stage boundary */
    void         *hook_user;
};

namespace {

struct ed_pic_dev {
    const svt_me_pu_result *res;    /* stand-in decision only */
    svt_mc_mode_info       *mc_mi;
    svt_lf_mode_info       *lf_mi;
    uint8_t                *nz;
    uint16_t               *eob_map;
    svt_lf_mask            *lfm;
    svt_tq_pic_geom         g;
};
struct ed_batch_dev {
    ed_pic_dev pic[ED_MAX_PICS];
    uint32_t   iscan_off[16];
    int32_t    n_pics, n_sb, sb_cols, mi_rows, mi_cols, mi_stride, width, height;
    uint32_t   lambda;
    int32_t    filter_level;
};

/* one wave per (picture, SB), one lane per 8x8 unit: per-SB number of transform blocks of each size; also clears the unit's
 * "has coefficients" scratch byte for the skip pass */
__global__ __launch_bounds__(64) void svt_tq_count_kernel(const ed_batch_dev *__restrict__ B, int32_t *__restrict__ counts, int32_t *__restrict__ status) {
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const ed_pic_dev &P = B->pic[pic];
    const int ur = (sb / B->sb_cols) * 8 + (lane >> 3), uc = (sb % B->sb_cols) * 8 + (lane & 7);
    int cnt[4] = {0, 0, 0, 0};
    if (ur < B->mi_rows && uc < B->mi_cols) P.nz[ur * B->mi_stride + uc] = 0;
    const int o = svt_tq_unit_is_origin(P.lf_mi, B->mi_stride, B->mi_rows, B->mi_cols, ur, uc);
    if (o < 0) atomicOr(status, 1);
    if (o == 1) svt_tq_unit_counts(P.lf_mi, B->mi_stride, ur, uc, cnt);
    _Pragma("unroll") for (int s = 0; s < 4; s++) {
        const int v = wave_sum(cnt[s]);
        if (lane == 0) counts[(s * B->n_pics + pic) * B->n_sb + sb] = v;
    }
}

/* Offsets of the lists, two small kernels instead of one long serial one.  Level 1: one workgroup per (size, picture) turns the
 * picture's per-SB counts into exclusive prefixes in place and leaves the picture's total in totals[size * n_pics + picture].  Level 2:
 * one wave turns the totals into the first block of every (size, picture) (bases[], in list order: size, then picture) and into
 * off_cnt[s] / off_cnt[4 + s] = first block / number of blocks of size s.  The emit kernel adds bases[] to the per-SB prefixes. */
__global__ __launch_bounds__(256) void svt_scan_sb_kernel(int32_t *__restrict__ a, int n_sb, int32_t *__restrict__ totals) {
    __shared__ int32_t part[256];
    int32_t *p = a + (size_t)blockIdx.x * n_sb;
    const int t = (int)threadIdx.x, per = (n_sb + 255) / 256, b = t * per, e = b + per < n_sb ? b + per : n_sb;
    int s = 0;
    for (int i = b; i < e; i++) s += p[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = b; i < e; i++) { const int v = p[i]; p[i] = run; run += v; }
    if (t == 255) totals[blockIdx.x] = part[255];
}
__global__ __launch_bounds__(64) void svt_scan_pic_kernel(const int32_t *__restrict__ totals, int n_pics, int32_t *__restrict__ bases, int32_t *__restrict__ off_cnt) {
    if (threadIdx.x != 0) return; /* 4 x n_pics (<= 128) values: not worth more than one lane */
    int run = 0;
    for (int s = 0; s < 4; s++) {
        off_cnt[s] = run;
        for (int p = 0; p < n_pics; p++) { bases[s * n_pics + p] = run; run += totals[s * n_pics + p]; }
        off_cnt[4 + s] = run - off_cnt[s];
    }
}

/* the descriptor list a host may ask for (svt_hip_encdec_work_download): rebuilt from the position codes, the transform size of the range a
 * block sits in and the pictures' geometry -- the same function the transform kernels call per block */
__global__ __launch_bounds__(256) void svt_tq_expand_kernel(const ed_batch_dev *__restrict__ B, const int32_t *__restrict__ off_cnt, const uint32_t *__restrict__ pos,
                                                           svt_tq_block *__restrict__ blocks) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x, total = off_cnt[3] + off_cnt[7];
    if (i >= total) return;
    const int      ts = i >= off_cnt[3] ? 3 : i >= off_cnt[2] ? 2 : i >= off_cnt[1] ? 1 : 0;
    const uint32_t p = pos[i];
    svt_tq_block   k;
    svt_tq_block_from_pos(p, ts, &B->pic[svt_tq_pos_pic(p)].g, B->iscan_off, B->sb_cols, &k);
    blocks[i] = k;
}

/* same mapping as the count kernel: every block-origin lane writes its descriptors at offsets[size][picture][SB] + (blocks of that
 * size of the lanes before it) */
__global__ __launch_bounds__(64) void svt_tq_emit_kernel(const ed_batch_dev *__restrict__ B, const int32_t *__restrict__ offsets, const int32_t *__restrict__ bases,
                                                         svt_tq_block *__restrict__ blocks, uint32_t *__restrict__ pos) {
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const ed_pic_dev &P = B->pic[pic];
    const int ur = (sb / B->sb_cols) * 8 + (lane >> 3), uc = (sb % B->sb_cols) * 8 + (lane & 7);
    int cnt[4] = {0, 0, 0, 0};
    const int o = svt_tq_unit_is_origin(P.lf_mi, B->mi_stride, B->mi_rows, B->mi_cols, ur, uc);
    if (o == 1) svt_tq_unit_counts(P.lf_mi, B->mi_stride, ur, uc, cnt);
    uint32_t base[4];
    _Pragma("unroll") for (int s = 0; s < 4; s++) base[s] = (uint32_t)(bases[s * B->n_pics + pic] + offsets[(s * B->n_pics + pic) * B->n_sb + sb] + wave_excl_prefix(cnt[s], lane));
    if (o == 1) svt_tq_unit_emit(P.lf_mi, B->mi_stride, ur, uc, &P.g, B->iscan_off, base, blocks, pos);
}

/* after the transform stage: the eob of every block goes to its place in the picture's eob map, and a block with coefficients marks
 * the prediction block it belongs to (the skip flag of the reference is "no coefficient in any transform block of the block",
 * Codec/EbEncDecProcess.c:4069-4098; the four 4x4 quadrants of a sub-8x8 unit share one flag the same way) */
__global__ __launch_bounds__(256) void svt_tq_skip_kernel(const ed_batch_dev *__restrict__ B, const int32_t *__restrict__ off_cnt, const uint32_t *__restrict__ pos,
                                                          const uint16_t *__restrict__ eob) {
    const int total = off_cnt[3] + off_cnt[7];
    const int w4 = B->width >> 2, h4 = B->height >> 2;
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
        const uint32_t p = pos[i];
        const int      pic = (int)(p >> 24) & 63, plane = (int)(p >> 22) & 3, y4 = (int)(p >> 11) & 0x7ff, x4 = (int)p & 0x7ff;
        const ed_pic_dev &P = B->pic[pic];
        const int      e = eob[i];
        const int      pw4 = plane ? w4 >> 1 : w4;
        const int      off = plane == 0 ? 0 : w4 * h4 + (plane == 2 ? (w4 >> 1) * (h4 >> 1) : 0);
        P.eob_map[off + y4 * pw4 + x4] = (uint16_t)e;
        if (e) {
            const int uy = plane ? y4 : y4 >> 1, ux = plane ? x4 : x4 >> 1;
            const svt_lf_mode_info b = P.lf_mi[uy * B->mi_stride + ux];
            const int w8 = svt_blk_w8(b.sb_type), h8 = svt_blk_h8(b.sb_type);
            P.nz[(uy - uy % h8) * B->mi_stride + (ux - ux % w8)] = 1;
        }
    }
}
/* the eob maps of the batch read 0 before the blocks write theirs: one launch for all pictures (16 bytes per lane) */
__global__ __launch_bounds__(256) void svt_eob_map_clear_kernel(const ed_batch_dev *__restrict__ B, int n16) {
    uint4 *m = (uint4 *)B->pic[blockIdx.y].eob_map;
    for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < n16; i += (int)(gridDim.x * 256)) m[i] = make_uint4(0, 0, 0, 0);
}
/* every unit takes the skip flag of its block */
__global__ __launch_bounds__(256) void svt_skip_update_kernel(const ed_batch_dev *__restrict__ B) {
    const int units = B->mi_rows * B->mi_cols;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= units * B->n_pics) return;
    const int pic = i / units, u = i % units, ur = u / B->mi_cols, uc = u % B->mi_cols;
    const ed_pic_dev &P = B->pic[pic];
    svt_lf_mode_info *b = &P.lf_mi[ur * B->mi_stride + uc];
    if (b->sb_type > 12) return;
    const int w8 = svt_blk_w8(b->sb_type), h8 = svt_blk_h8(b->sb_type);
    b->skip = P.nz[(ur - ur % h8) * B->mi_stride + (uc - uc % w8)] ? 0 : 1;
}

/* one wave per (picture, SB), one lane per 8x8 unit: the unit's contribution (svt_lf_mask_unit, the text svt_hip_lf_build_masks runs
 * on the host) and a wave-wide OR; lane u writes lfl_y[u], lanes 0..18 the mask words */
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    _Pragma("unroll") for (int d = 32; d >= 1; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}
__global__ __launch_bounds__(64) void svt_lf_mask_kernel(const ed_batch_dev *__restrict__ B, int32_t *__restrict__ status) {
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const ed_pic_dev &P = B->pic[pic];
    svt_lf_unit_masks u;
    svt_lf_mask_unit(P.lf_mi, B->mi_stride, B->mi_rows, B->mi_cols, sb / B->sb_cols, sb % B->sb_cols, lane >> 3, lane & 7, &u);
    if (u.bad && status) atomicOr(status, 1);
    /* the 160-byte mask is assembled in LDS and leaves as 40 consecutive dwords (one coalesced store instead of a dozen partial ones) */
    __shared__ uint32_t sm[40];
    uint64_t            w64[9];
    _Pragma("unroll") for (int i = 0; i < 4; i++) { w64[i] = u.left_y[i]; w64[4 + i] = u.above_y[i]; }
    w64[8] = u.int_4x4_y;
    _Pragma("unroll") for (int i = 0; i < 9; i++) {   /* left_y[4], above_y[4], int_4x4_y: the first nine quadwords of the mask */
        const uint32_t lo = wave_or((uint32_t)w64[i]), hi = wave_or((uint32_t)(w64[i] >> 32));
        if (lane == i) { sm[2 * i] = lo; sm[2 * i + 1] = hi; }
    }
    /* the nine 16-bit chroma words, two per dword: left_uv[0..3], above_uv[0..3], int_4x4_uv (bytes 72..89) */
    const uint32_t c0 = wave_or((uint32_t)u.left_uv[0] | (uint32_t)u.left_uv[1] << 16), c1 = wave_or((uint32_t)u.left_uv[2] | (uint32_t)u.left_uv[3] << 16);
    const uint32_t c2 = wave_or((uint32_t)u.above_uv[0] | (uint32_t)u.above_uv[1] << 16), c3 = wave_or((uint32_t)u.above_uv[2] | (uint32_t)u.above_uv[3] << 16);
    const uint32_t c4 = wave_or((uint32_t)u.int_4x4_uv);
    if (lane == 9) { sm[18] = c0; sm[19] = c1; sm[20] = c2; sm[21] = c3; sm[22] = c4; sm[38] = 0; sm[39] = 0; } /* (dword 22's upper half and dwords 38-39 are rewritten below) */
    __syncthreads();
    ((uint8_t *)sm)[90 + lane] = u.level;   /* lfl_y[64]: bytes 90..153 */
    __syncthreads();
    if (lane < 40) ((uint32_t *)&P.lfm[sb])[lane] = sm[lane];
}

/* stand-in decision: one wave per (picture, SB), one lane per unit */
__global__ __launch_bounds__(64) void svt_md_default_kernel(const ed_batch_dev *__restrict__ B) {
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const ed_pic_dev &P = B->pic[pic];
    const int r = lane >> 3, c = lane & 7, sr = sb / B->sb_cols, sc = sb % B->sb_cols, ur = sr * 8 + r, uc = sc * 8 + c;
    if (ur >= B->mi_rows || uc >= B->mi_cols) return;
    svt_md_default_unit(P.res + (size_t)sb * SVT_ME_PU_COUNT, r, c, sr, sc, B->mi_rows, B->mi_cols, B->lambda, B->filter_level, &P.mc_mi[ur * B->mi_stride + uc],
                        &P.lf_mi[ur * B->mi_stride + uc]);
}

/* the batch's parameter block goes to the device through the context's descriptor ring */
int stage_batch(svt_hip_ctx *ctx, const ed_batch_dev &hb, const ed_batch_dev **d_out) {
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof hb, &h, &d)) return -1;
    memcpy(h, &hb, sizeof hb);
    if (svt_ctx_stage_send(ctx, sizeof hb) != hipSuccess) return -1;
    *d_out = (const ed_batch_dev *)d;
    return 0;
}

void fill_dims(ed_batch_dev &hb, int n_pics, int width, int height, int mi_stride) {
    hb.n_pics = n_pics; hb.width = width; hb.height = height;
    hb.sb_cols = (width + 63) >> 6;
    hb.n_sb = hb.sb_cols * ((height + 63) >> 6);
    hb.mi_rows = height >> 3; hb.mi_cols = width >> 3; hb.mi_stride = mi_stride;
}

} // namespace

extern "C" int32_t svt_hip_encdec_work_create(svt_hip_ctx *ctx, int32_t max_pics, int32_t width, int32_t height, svt_encdec_work **out) {
    if (!ctx || !out || max_pics < 1 || max_pics > ED_MAX_PICS || width < 8 || height < 8 || (width & 7) || (height & 7))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "encdec_work: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    svt_encdec_work *w = (svt_encdec_work *)calloc(1, sizeof *w);
    if (!w) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "encdec_work: malloc");
    w->max_pics = max_pics; w->width = width; w->height = height;
    w->sb_cols = (width + 63) >> 6; w->n_sb = w->sb_cols * ((height + 63) >> 6);
    w->mi_rows = height >> 3; w->mi_cols = width >> 3;
    w->cap_per_pic = (size_t)width * height * 3 / 32;
    const size_t cap = w->cap_per_pic * (size_t)max_pics;
    const size_t n_cnt = (size_t)4 * max_pics * w->n_sb;
    uint32_t const *offs = nullptr;
    int32_t         entries = 0;
    const int16_t  *isc = svt_hip_vp9_iscan_tables(&offs, &entries);
    /* the lists are position codes (4 bytes per transform block; the 32-byte descriptors are rebuilt in registers where they are used) */
    bool ok = hipMalloc((void **)&w->d_pos, cap * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void **)&w->d_eob, cap * sizeof(uint16_t)) == hipSuccess &&
              hipMalloc((void **)&w->d_counts, (n_cnt + 9 + 8 * ED_MAX_PICS + 2 + 48 * (size_t)w->n_sb) * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&w->d_qtabs, 2 * sizeof(svt_quant_tables)) == hipSuccess && hipMalloc((void **)&w->d_iscan, (size_t)entries * sizeof(int16_t)) == hipSuccess;
    if (ok) {
        w->d_off_cnt = w->d_counts + n_cnt;
        w->d_status = w->d_off_cnt + 8;
        w->d_totals = w->d_status + 1;
        w->d_bases = w->d_totals + 4 * ED_MAX_PICS;
        w->d_intra_sync = w->d_bases + 4 * ED_MAX_PICS;
        ok = hipMemsetAsync(w->d_off_cnt, 0, 9 * sizeof(int32_t), ctx->stream) == hipSuccess &&
             hipMemcpyAsync(w->d_iscan, isc, (size_t)entries * sizeof(int16_t), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
             hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    if (!ok) {
        svt_hip_encdec_work_destroy(ctx, w);
        return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "encdec_work: device memory");
    }
    *out = w;
    return SVT_HIP_OK;
}

extern "C" void svt_hip_encdec_work_destroy(svt_hip_ctx *ctx, svt_encdec_work *w) {
    if (!w) return;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    void *v[6] = {w->d_blocks, w->d_pos, w->d_eob, w->d_counts, w->d_qtabs, w->d_iscan};
    for (int i = 0; i < 6; i++) if (v[i]) (void)hipFree(v[i]);
    free(w->last_hb);
    free(w);
}

/* profiling hook at a stage boundary of the batch entries (svt_hip_encdec_work_set_stage_hook); w: the workspace */
#define ED_STAGE(k) do { if (w->hook) w->hook(w->hook_user, (k)); } while (0)

namespace {

/* what a batch entry hands to its launches: the parameter block (host copy and its device twin), the base pointers of the batch's
 * 32-bit offset spaces and the per-picture descriptors of the stages behind the transform */
struct ed_setup {
    ed_batch_dev        hb;
    const ed_batch_dev *dB;
    uintptr_t           src_lo, pred_lo, q_lo, dq_lo;
    uint8_t            *recon_set[ED_MAX_SETS];
    int                 n_sets;
    svt_mc_picture      mcp[ED_MAX_PICS];
    svt_yuv_planes      rec[ED_MAX_PICS], rec_pad[ED_MAX_PICS];
    int                 n_rec_pad;
    const svt_lf_mask  *lfm[ED_MAX_PICS];
    int32_t             lfm_stride[ED_MAX_PICS], mi_rows_a[ED_MAX_PICS], mi_cols_a[ED_MAX_PICS];
};

/* an error under the name of the entry it belongs to: "encdec: ...", "decode: ...", "encdec_intra: ...", "decode_intra: ..." */
int32_t ed_bad(const char *who, const char *what, int32_t code = SVT_HIP_ERR_BAD_PARAMETER) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return svt_set_error(code, msg);
}

/* quantiser tables of the q index -> the work area's pair */
int32_t ed_send_qtabs(svt_hip_ctx *ctx, svt_encdec_work *w, const svt_quant_tables (&qt)[2], const char *who) {
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof qt, &h, &d)) return ed_bad(who, "descriptor buffers", SVT_HIP_ERR_NO_RESOURCES);
    memcpy(h, qt, sizeof qt);
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof qt, w->d_qtabs)); /* (the work area's tables, not the slot's device twin) */
    return SVT_HIP_OK;
}

/* The stages the entries share.  Each is the launches of one step of a batch entry in their order; the entries keep the stage markers
 * whose place differs between them (MC, LISTS, TQ, SKIP). */

/* transform blocks from the grids: the lists of the batch in w->d_pos, their offsets and counts in w->d_off_cnt */
int32_t ed_lists(svt_hip_ctx *ctx, svt_encdec_work *w, const ed_batch_dev &hb, const ed_batch_dev *dB) {
    const int nwg = hb.n_pics * hb.n_sb;
    hipLaunchKernelGGL(svt_tq_count_kernel, dim3(nwg), dim3(64), 0, ctx->stream, dB, w->d_counts, w->d_status);
    hipLaunchKernelGGL(svt_scan_sb_kernel, dim3(4 * hb.n_pics), dim3(256), 0, ctx->stream, w->d_counts, hb.n_sb, w->d_totals);
    hipLaunchKernelGGL(svt_scan_pic_kernel, dim3(1), dim3(64), 0, ctx->stream, (const int32_t *)w->d_totals, hb.n_pics, w->d_bases, w->d_off_cnt);
    hipLaunchKernelGGL(svt_tq_emit_kernel, dim3(nwg), dim3(64), 0, ctx->stream, dB, (const int32_t *)w->d_counts, (const int32_t *)w->d_bases, (svt_tq_block *)nullptr, w->d_pos);
    HIP_TRY(hipGetLastError());
    if (!w->last_hb) w->last_hb = malloc(sizeof hb);
    if (w->last_hb) memcpy(w->last_hb, &hb, sizeof hb);
    return SVT_HIP_OK;
}

/* blocks of each transform size the batch holds at most */
void ed_block_caps(const ed_batch_dev &hb, int32_t cap[4]) {
    for (int s = 0; s < 4; s++) cap[s] = (int32_t)((size_t)hb.n_pics * hb.width * hb.height * 3 / 2 / (size_t)(16 << (2 * s)));
}

/* skip flags.  from_lists: the eob of every listed block goes to its picture's eob map and marks its unit first (the batch entries; the
 * wavefront kernels of the intra entries have written both themselves) */
int32_t ed_skip(svt_hip_ctx *ctx, svt_encdec_work *w, const ed_batch_dev &hb, const ed_batch_dev *dB, const bool from_lists) {
    if (from_lists) {
        const int total_cap = (int)(w->cap_per_pic * (size_t)hb.n_pics);
        int       g = (total_cap + 255) / 256;
        if (g > ctx->cu_count * 8) g = ctx->cu_count * 8;
        hipLaunchKernelGGL(svt_tq_skip_kernel, dim3(g), dim3(256), 0, ctx->stream, dB, (const int32_t *)w->d_off_cnt, (const uint32_t *)w->d_pos, (const uint16_t *)w->d_eob);
    }
    hipLaunchKernelGGL(svt_skip_update_kernel, dim3((hb.n_pics * hb.mi_rows * hb.mi_cols + 255) / 256), dim3(256), 0, ctx->stream, dB);
    HIP_TRY(hipGetLastError());
    return SVT_HIP_OK;
}

/* loop-filter masks of n_pics pictures from their grids (status may be null) */
int32_t ed_lf_masks(svt_hip_ctx *ctx, const ed_batch_dev *dB, int n_pics, int n_sb, int32_t *status) {
    hipLaunchKernelGGL(svt_lf_mask_kernel, dim3(n_pics * n_sb), dim3(64), 0, ctx->stream, dB, status);
    HIP_TRY(hipGetLastError());
    return SVT_HIP_OK;
}

/* the tail of every entry: deblocking (thr = NULL: none) of the hb.n_pics pictures rec[], then the borders of rec_pad[0 .. n_rec_pad)
 * (0: none), with the LF / PAD / END markers */
int32_t ed_tail(svt_hip_ctx *ctx, svt_encdec_work *w, const ed_batch_dev &hb, const ed_batch_dev *dB, const svt_yuv_planes *rec, const svt_lf_mask *const *lfm,
                const int32_t *lfm_stride, const int32_t *mi_rows_a, const int32_t *mi_cols_a, const svt_lf_thresh *thr, int n_rec_pad, const svt_yuv_planes *rec_pad,
                int32_t pad_x, int32_t pad_y) {
    ED_STAGE(SVT_ENCDEC_STAGE_LF);
    if (thr) {
        int32_t rc = ed_lf_masks(ctx, dB, hb.n_pics, hb.n_sb, w->d_status);
        if (rc) return rc;
        rc = svt_hip_lf_batch_device(ctx, hb.n_pics, rec, lfm, lfm_stride, thr, mi_rows_a, mi_cols_a, 0);
        if (rc) return rc;
    }
    /* the reconstruction becomes a reference picture */
    ED_STAGE(SVT_ENCDEC_STAGE_PAD);
    if (n_rec_pad) {
        const int32_t rc = svt_hip_ref_pad_batch_device(ctx, n_rec_pad, rec_pad, pad_x, pad_y);
        if (rc) return rc;
    }
    ED_STAGE(SVT_ENCDEC_STAGE_END);
    return SVT_HIP_OK;
}

/* Set-up of svt_hip_encdec_intra_device (encode) and svt_hip_decode_intra_device: every refusal, then the one-picture parameter block and
 * the q index's tables sent.  own_refusal: what the entry itself found wrong with its own arguments (null: nothing), reported behind
 * "bad argument".  lf: the picture will be deblocked (d_lfm is needed).  Of the picture, src and d_dqcoeff are looked at for the encode
 * entry only.  Everything is checked before the first enqueue: a refusal leaves every buffer as it was. */
struct ed_intra_setup {
    ed_batch_dev        hb;
    const ed_batch_dev *dB;
    const uint32_t     *iscan_off;
    svt_yuv_planes      rec;
    const svt_lf_mask  *lfm;
    int32_t             lfm_stride, mi_rows, mi_cols;
};
int32_t ed_intra_prepare(svt_hip_ctx *ctx, svt_encdec_work *w, const svt_encdec_picture *pic, int32_t width, int32_t height, int32_t mi_stride, int32_t q_index,
                         const bool lf, const bool encode, const char *who, const char *own_refusal, ed_intra_setup &S) {
    if (!ctx || !w || !pic || width != w->width || height != w->height || mi_stride < (width >> 3)) return ed_bad(who, "bad argument");
    if (own_refusal) return ed_bad(who, own_refusal);
    const svt_encdec_picture &p = *pic;
    if (!p.d_lf_mi || (encode && (!p.src.y || !p.src.u || !p.src.v)) || !p.recon.y || !p.recon.u || !p.recon.v || !p.d_qcoeff || !p.d_eob_map || !p.d_nz || (lf && !p.d_lfm))
        return ed_bad(who, "null picture field");
    if (((uintptr_t)p.d_qcoeff | (encode ? (uintptr_t)p.d_dqcoeff : 0)) & 15)
        return ed_bad(who, encode ? "coefficient arrays must be 16-byte aligned" : "the coefficient array must be 16-byte aligned");
    if (p.recon.y_stride > 65535 || ((p.recon.y_stride | p.recon.uv_stride) & 3) || (((uintptr_t)p.recon.y | (uintptr_t)p.recon.u | (uintptr_t)p.recon.v) & 3) ||
        (encode && (((p.src.y_stride | p.src.uv_stride) & 3) || (((uintptr_t)p.src.y | (uintptr_t)p.src.u | (uintptr_t)p.src.v) & 3))) ||
        (p.pred.y && (((uintptr_t)p.pred.y | (uintptr_t)p.pred.u | (uintptr_t)p.pred.v | (uintptr_t)p.pred.y_stride | (uintptr_t)p.pred.uv_stride) & 3)))
        return ed_bad(who, "planes and strides must be 4-byte aligned");
    if (p.pred.y && (!p.pred.u || !p.pred.v)) return ed_bad(who, "prediction planes");
    svt_quant_tables qt[2];
    if (svt_hip_quant_tables_for_qindex(q_index, qt) != SVT_HIP_OK) return ed_bad(who, "q index");
    HIP_TRY(hipSetDevice(ctx->device));
    ed_batch_dev &hb = S.hb;
    memset(&hb, 0, sizeof hb);
    fill_dims(hb, 1, width, height, mi_stride);
    (void)svt_hip_vp9_iscan_tables(&S.iscan_off, nullptr);
    hb.pic[0].lf_mi = p.d_lf_mi; hb.pic[0].nz = p.d_nz; hb.pic[0].eob_map = p.d_eob_map; hb.pic[0].lfm = p.d_lfm;
    if (stage_batch(ctx, hb, &S.dB)) return ed_bad(who, "descriptor buffers", SVT_HIP_ERR_NO_RESOURCES);
    if (const int32_t e = ed_send_qtabs(ctx, w, qt, who)) return e;
    /* what ed_tail takes: arrays of length 1 */
    S.rec = p.recon; S.rec.width = width; S.rec.height = height;
    S.lfm = p.d_lfm; S.lfm_stride = hb.sb_cols; S.mi_rows = hb.mi_rows; S.mi_cols = hb.mi_cols;
    return SVT_HIP_OK;
}

/* Argument checking and descriptor set-up of svt_hip_encdec_batch_device and svt_hip_decode_batch_device: everything in front of the
 * first launch, the parameter block and the q index's tables sent.  decode: the pictures' src and d_dqcoeff are not looked at (the source
 * offsets of the geometry records read 0) and a picture with has_intra is refused unless allow_intra (svt_hip_decode_mixed_batch_device:
 * such a picture's planes and strides must then be 4-byte aligned, what the wavefront kernel's dword accesses need). */
int32_t ed_prepare(svt_hip_ctx *ctx, svt_encdec_work *w, int32_t n_pics, const svt_encdec_picture *pics, int32_t width, int32_t height, int32_t mi_stride,
                   int32_t q_index, const svt_encdec_flags *flags, const svt_lf_thresh *thr, const bool decode, const bool allow_intra, ed_setup &S) {
    const char *const who = decode ? "decode" : "encdec";
    if (!ctx || !w || !pics || !flags || n_pics < 1 || n_pics > w->max_pics || width != w->width || height != w->height || mi_stride < (width >> 3))
        return ed_bad(who, "bad argument");
    if (flags->apply_loop_filter && !thr) return ed_bad(who, "loop filter without thresholds");
    if (decode && !allow_intra)
        for (int i = 0; i < n_pics; i++)
            if (pics[i].has_intra) return svt_set_error(SVT_HIP_ERR_UNSUPPORTED, "decode: pictures with intra blocks are not reconstructed by this entry");
    HIP_TRY(hipSetDevice(ctx->device));
    /* one 32-bit offset space for the source planes and one for the prediction planes of the batch */
    uintptr_t src_lo = UINTPTR_MAX, src_hi = 0, pred_lo = UINTPTR_MAX, pred_hi = 0;
    for (int i = 0; i < n_pics; i++) {
        const svt_encdec_picture &p = pics[i];
        if (!p.d_mc_mi || !p.d_lf_mi || (!decode && (!p.src.y || !p.src.u || !p.src.v)) || !p.pred.y || !p.pred.u || !p.pred.v || !p.recon.y || !p.recon.u || !p.recon.v ||
            !p.d_qcoeff || !p.d_eob_map || !p.d_nz || (flags->apply_loop_filter && !p.d_lfm))
            return ed_bad(who, "null picture field");
        if (!decode && !p.d_dqcoeff != !pics[0].d_dqcoeff) return ed_bad(who, "d_dqcoeff must be given for every picture of a batch or for none");
        if (((uintptr_t)p.d_qcoeff | (decode ? 0 : (uintptr_t)p.d_dqcoeff)) & 15) return ed_bad(who, "coefficient arrays must be 16-byte aligned");
        if (decode && p.has_intra &&
            (((uintptr_t)p.pred.y | (uintptr_t)p.pred.u | (uintptr_t)p.pred.v | (uintptr_t)p.recon.y | (uintptr_t)p.recon.u | (uintptr_t)p.recon.v |
              (uintptr_t)p.pred.y_stride | (uintptr_t)p.pred.uv_stride | (uintptr_t)p.recon.y_stride | (uintptr_t)p.recon.uv_stride) & 3))
            return ed_bad(who, "planes and strides of a picture with intra blocks must be 4-byte aligned");
        const uint8_t *s3[3] = {p.src.y, p.src.u, p.src.v}, *p3[3] = {p.pred.y, p.pred.u, p.pred.v};
        for (int k = 0; k < 3; k++) {
            if (!decode) { src_lo = (uintptr_t)s3[k] < src_lo ? (uintptr_t)s3[k] : src_lo; src_hi = (uintptr_t)s3[k] > src_hi ? (uintptr_t)s3[k] : src_hi; }
            pred_lo = (uintptr_t)p3[k] < pred_lo ? (uintptr_t)p3[k] : pred_lo; pred_hi = (uintptr_t)p3[k] > pred_hi ? (uintptr_t)p3[k] : pred_hi;
        }
    }
    if (decode) src_lo = src_hi = 0;
    /* bytes from a plane's first sample to its last row's end: the largest stride x rows among the planes the 32-bit block offsets
       address (a reference buffer's stride is width + 160; a caller's stride can exceed 2 x width on narrow pictures) */
    uint64_t plane_span = 0;
    for (int i = 0; i < n_pics; i++) {
        const svt_yuv_planes *pl[3] = {&pics[i].src, &pics[i].pred, &pics[i].recon};
        for (int k = decode ? 1 : 0; k < 3; k++) {
            const uint64_t a = (uint64_t)(pl[k]->y_stride > 0 ? pl[k]->y_stride : 0) * (uint64_t)height, b = (uint64_t)(pl[k]->uv_stride > 0 ? pl[k]->uv_stride : 0) * (uint64_t)(height / 2);
            plane_span = a > plane_span ? a : plane_span;
            plane_span = b > plane_span ? b : plane_span;
        }
    }
    if ((uint64_t)(src_hi - src_lo) + plane_span >= (1ull << 32) || (uint64_t)(pred_hi - pred_lo) + plane_span >= (1ull << 32))
        return ed_bad(who, "the batch's source / prediction planes must lie within 4 GB");
    /* coefficient arrays: one base for the batch as well (element offsets are 32 bit) */
    uintptr_t q_lo = UINTPTR_MAX, dq_lo = UINTPTR_MAX;
    for (int i = 0; i < n_pics; i++) {
        q_lo = (uintptr_t)pics[i].d_qcoeff < q_lo ? (uintptr_t)pics[i].d_qcoeff : q_lo;
        if (!decode) dq_lo = (uintptr_t)pics[i].d_dqcoeff < dq_lo ? (uintptr_t)pics[i].d_dqcoeff : dq_lo;
    }
    if (decode) dq_lo = 0;
    ed_batch_dev &hb = S.hb;
    memset(&hb, 0, sizeof hb);
    fill_dims(hb, n_pics, width, height, mi_stride);
    {
        const uint32_t *offs = nullptr;
        (void)svt_hip_vp9_iscan_tables(&offs, nullptr);
        for (int i = 0; i < 16; i++) hb.iscan_off[i] = offs[i];
    }
    /* reconstruction bases: at most ED_MAX_SETS pointers, each serving every picture whose planes lie within 4 GB above it.  Chosen
       from the pictures' lowest plane addresses in ascending order, so that the result does not depend on the order the pictures
       arrive in (separately allocated buffers in descending address order once opened a base each) */
    uint8_t      **recon_set = S.recon_set;
    int            n_sets = 0;
    {
        uintptr_t lo[ED_MAX_PICS], hi[ED_MAX_PICS];
        int       order[ED_MAX_PICS];
        for (int i = 0; i < n_pics; i++) {
            const uint8_t *r3[3] = {pics[i].recon.y, pics[i].recon.u, pics[i].recon.v};
            lo[i] = UINTPTR_MAX; hi[i] = 0; order[i] = i;
            for (int k = 0; k < 3; k++) { lo[i] = (uintptr_t)r3[k] < lo[i] ? (uintptr_t)r3[k] : lo[i]; hi[i] = (uintptr_t)r3[k] > hi[i] ? (uintptr_t)r3[k] : hi[i]; }
        }
        for (int a = 1; a < n_pics; a++) /* insertion sort by lowest address (n_pics <= 32) */
            for (int b = a; b > 0 && lo[order[b]] < lo[order[b - 1]]; b--) { const int t_ = order[b]; order[b] = order[b - 1]; order[b - 1] = t_; }
        for (int a = 0; a < n_pics; a++) {
            const int i = order[a];
            if (n_sets && (uint64_t)(hi[i] - (uintptr_t)recon_set[n_sets - 1]) + plane_span < (1ull << 32)) continue; /* (sorted: lo[i] >= the last base) */
            if (n_sets == ED_MAX_SETS || (uint64_t)(hi[i] - lo[i]) + plane_span >= (1ull << 32))
                return ed_bad(who, "the batch's reconstruction buffers span more than 8 regions of 4 GB");
            recon_set[n_sets++] = (uint8_t *)lo[i];
        }
    }
    svt_mc_picture *mcp = S.mcp;
    svt_yuv_planes *rec = S.rec, *rec_pad = S.rec_pad;
    int            n_rec_pad = 0;
    const svt_lf_mask **lfm = S.lfm;
    int32_t       *lfm_stride = S.lfm_stride, *mi_rows_a = S.mi_rows_a, *mi_cols_a = S.mi_cols_a;
    for (int i = 0; i < n_pics; i++) {
        const svt_encdec_picture &p = pics[i];
        ed_pic_dev &P = hb.pic[i];
        P.mc_mi = (svt_mc_mode_info *)p.d_mc_mi; P.lf_mi = p.d_lf_mi; P.nz = p.d_nz; P.eob_map = p.d_eob_map; P.lfm = p.d_lfm;
        const uintptr_t q_off = ((uintptr_t)p.d_qcoeff - q_lo) / sizeof(int16_t), dq_off = decode ? q_off : ((uintptr_t)p.d_dqcoeff - dq_lo) / sizeof(int16_t);
        if ((!decode && p.d_dqcoeff && q_off != dq_off) || q_off + (uint64_t)hb.n_sb * SVT_SB_COEFFS >= (1ull << 32))
            return ed_bad(who, "qcoeff / dqcoeff of the batch must be laid out alike, within 2^32 elements");
        /* the picture's reconstruction planes: 32-bit offsets from one of at most ED_MAX_SETS base pointers (a base serves every
           picture whose planes lie within 4 GB above it: buffers carved out of one slab share one) */
        const uint8_t *r3[3] = {p.recon.y, p.recon.u, p.recon.v};
        uintptr_t r_lo = UINTPTR_MAX, r_hi = 0;
        for (int k = 0; k < 3; k++) { r_lo = (uintptr_t)r3[k] < r_lo ? (uintptr_t)r3[k] : r_lo; r_hi = (uintptr_t)r3[k] > r_hi ? (uintptr_t)r3[k] : r_hi; }
        int set = -1;
        for (int k = n_sets - 1; k >= 0 && set < 0; k--) /* the highest base at or below the picture: the one chosen for it above */
            if (r_lo >= (uintptr_t)recon_set[k] && (uint64_t)(r_hi - (uintptr_t)recon_set[k]) + plane_span < (1ull << 32)) set = k;
        if (set < 0) return ed_bad(who, "the batch's reconstruction buffers span more than 8 regions of 4 GB");
        svt_tq_pic_geom &g = P.g;
        const uint8_t *s3[3] = {p.src.y, p.src.u, p.src.v}, *p3[3] = {p.pred.y, p.pred.u, p.pred.v};
        for (int k = 0; k < 3; k++) {
            g.src_off[k] = decode ? 0u : (uint32_t)((uintptr_t)s3[k] - src_lo); g.pred_off[k] = (uint32_t)((uintptr_t)p3[k] - pred_lo);
            g.recon_off[k] = (uint32_t)((uintptr_t)r3[k] - (uintptr_t)recon_set[set]);
        }
        if ((!decode && p.src.y_stride > 65535) || p.pred.y_stride > 65535 || p.recon.y_stride > 65535) return ed_bad(who, "stride");
        g.src_stride[0] = decode ? 0 : (uint16_t)p.src.y_stride; g.src_stride[1] = decode ? 0 : (uint16_t)p.src.uv_stride;
        g.pred_stride[0] = (uint16_t)p.pred.y_stride; g.pred_stride[1] = (uint16_t)p.pred.uv_stride;
        g.recon_stride[0] = (uint16_t)p.recon.y_stride; g.recon_stride[1] = (uint16_t)p.recon.uv_stride;
        g.coeff_base = (uint32_t)q_off; g.width = width; g.height = height; g.recon_set = (uint8_t)set; g.pic = (uint8_t)i; g.do_recon = flags->do_recon ? 1 : 0;
        mcp[i].d_mi = p.d_mc_mi; mcp[i].mi_stride = mi_stride; mcp[i].mi_rows = hb.mi_rows; mcp[i].mi_cols = hb.mi_cols;
        mcp[i].ref[0] = p.ref[0]; mcp[i].ref[1] = p.ref[1]; mcp[i].pred = p.pred; mcp[i].use_subpel = p.use_subpel;
        rec[i] = p.recon; rec[i].width = width; rec[i].height = height;
        if (!p.no_pad) rec_pad[n_rec_pad++] = rec[i];
        lfm[i] = p.d_lfm; lfm_stride[i] = hb.sb_cols; mi_rows_a[i] = hb.mi_rows; mi_cols_a[i] = hb.mi_cols;
    }
    const ed_batch_dev *dB = nullptr;
    if (stage_batch(ctx, hb, &dB)) return ed_bad(who, "descriptor buffers", SVT_HIP_ERR_NO_RESOURCES);
    /* quantiser tables of the q index */
    svt_quant_tables qt[2];
    if (svt_hip_quant_tables_for_qindex(q_index, qt) != SVT_HIP_OK) return ed_bad(who, "q index");
    if (const int32_t e = ed_send_qtabs(ctx, w, qt, who)) return e;
    S.dB = dB; S.src_lo = src_lo; S.pred_lo = pred_lo; S.q_lo = q_lo; S.dq_lo = dq_lo; S.n_sets = n_sets; S.n_rec_pad = n_rec_pad;
    return SVT_HIP_OK;
}

} // namespace

extern "C" int32_t svt_hip_encdec_batch_device(svt_hip_ctx *ctx, svt_encdec_work *w, int32_t n_pics, const svt_encdec_picture *pics, int32_t width,
                                               int32_t height, int32_t mi_stride, int32_t q_index, const svt_encdec_flags *flags, const svt_lf_thresh *thr,
                                               int32_t pad_x, int32_t pad_y) {
    ed_setup S;
    if (const int32_t e = ed_prepare(ctx, w, n_pics, pics, width, height, mi_stride, q_index, flags, thr, false, false, S)) return e;
    const ed_batch_dev &hb = S.hb;
    const ed_batch_dev *dB = S.dB;
    const uintptr_t     src_lo = S.src_lo, pred_lo = S.pred_lo, q_lo = S.q_lo, dq_lo = S.dq_lo;
    uint8_t *const     *recon_set = S.recon_set;
    const int           n_sets = S.n_sets;
    /* 1. inter prediction of the whole batch */
    ED_STAGE(SVT_ENCDEC_STAGE_MC);
    int32_t rc = svt_hip_inter_pred_batch_device(ctx, n_pics, S.mcp);
    if (rc) return rc;
    /* 2. transform blocks from the grids */
    ED_STAGE(SVT_ENCDEC_STAGE_LISTS);
    rc = ed_lists(ctx, w, hb, dB);
    if (rc) return rc;
    /* 3. residual -> transform -> quantisation (-> inverse -> reconstruction) */
    ED_STAGE(SVT_ENCDEC_STAGE_TQ);
    int32_t cap[4];
    ed_block_caps(hb, cap);
    rc = svt_tq_launch_device_lists(ctx, (const uint8_t *)src_lo, (const uint8_t *)pred_lo, recon_set, n_sets, nullptr, cap, w->d_off_cnt, w->d_qtabs, w->d_iscan,
                                    (int16_t *)q_lo, (int16_t *)dq_lo, w->d_eob, nullptr, w->d_pos, &dB->pic[0].g, (int)sizeof(ed_pic_dev), dB->iscan_off, hb.sb_cols);
    if (rc) return rc;
    /* 4. eob map + skip flags (entries of the map that are not the origin of a transform block of THIS picture read 0) */
    ED_STAGE(SVT_ENCDEC_STAGE_SKIP);
    {
        const size_t map_bytes = (size_t)(width / 4) * (height / 4) * 3 / 2 * sizeof(uint16_t);
        uintptr_t    low = map_bytes;
        for (int i = 0; i < n_pics; i++) low |= (uintptr_t)pics[i].d_eob_map;
        if (!(low & 15))
            hipLaunchKernelGGL(svt_eob_map_clear_kernel, dim3(64, n_pics), dim3(256), 0, ctx->stream, dB, (int)(map_bytes / 16));
        else
            for (int i = 0; i < n_pics; i++) HIP_TRY(hipMemsetAsync(pics[i].d_eob_map, 0, map_bytes, ctx->stream));
    }
    /* 3b. intra blocks of inter pictures: their inter neighbours are reconstructed now; the wavefront kernel codes them, one picture
           after the other (it writes their eob-map entries and coefficient flags itself) */
    for (int i = 0; i < n_pics; i++)
        if (pics[i].has_intra) {
            if (!flags->do_recon) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "encdec: intra blocks need the reconstruction (do_recon)");
            rc = svt_intra_launch(ctx, &pics[i], width, height, mi_stride, w->d_qtabs, w->d_iscan, hb.iscan_off, w->d_intra_sync, w->d_status, 1);
            if (rc) return rc;
        }
    rc = ed_skip(ctx, w, hb, dB, true);
    if (rc) return rc;
    /* 5. deblocking, 6. the reconstruction becomes a reference picture */
    return ed_tail(ctx, w, hb, dB, S.rec, S.lfm, S.lfm_stride, S.mi_rows_a, S.mi_cols_a, flags->apply_loop_filter ? thr : nullptr, flags->pad_reference ? S.n_rec_pad : 0,
                   S.rec_pad, pad_x, pad_y);
}

namespace {
/* the lists of the decode pass hold inter leaves only: a unit inside the picture whose record says is_inter = 0 is reported (its blocks are
 * in no list) unless its picture's bit of intra_mask is set (has_intra: the wavefront kernel reconstructs them) */
__global__ __launch_bounds__(256) void svt_dec_intra_check_kernel(const ed_batch_dev *__restrict__ B, int32_t *__restrict__ status, const uint32_t intra_mask) {
    const int units = B->mi_rows * B->mi_cols;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= units * B->n_pics) return;
    const int pic = i / units, u = i % units;
    if ((intra_mask >> pic) & 1) return;
    if (!B->pic[pic].lf_mi[(u / B->mi_cols) * B->mi_stride + u % B->mi_cols].is_inter) atomicOr(status, 1);
}
/* The decode pass: a batch of inter pictures rebuilt from what a frame reader returned (include/svtvp9_hip.h).  The stages and their
 * order are the encode pass's, with svt_rc_kernel (recon_kernel.hip) in the place of the forward transform: the eob maps are inputs here
 * (not cleared), the reconstruction kernel leaves every block's eob in list order, and svt_tq_skip_kernel + svt_skip_update_kernel then
 * state exactly the decoder's rule -- an inter leaf of 8x8 or larger with no coefficient in any of its transform blocks is skipped for
 * the loop filter (vp9_decodeframe.c: decode_block resets mi->skip of such a leaf only when eobtotal is 0 and the leaf is >= 8x8; the
 * lists hold nothing below 8x8 that is inter).  svt_tq_skip_kernel's rewrite of the eob map entries stores the values it was read from. */
int32_t decode_batch(svt_hip_ctx *ctx, svt_encdec_work *w, int32_t n_pics, const svt_encdec_picture *pics, int32_t width, int32_t height, int32_t mi_stride,
                     int32_t q_index, const svt_lf_thresh *thr, int32_t pad_x, int32_t pad_y, int32_t *d_status, const bool allow_intra) {
    if (!d_status) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "decode: null status");
    svt_encdec_flags flags;
    memset(&flags, 0, sizeof flags);
    flags.do_recon = 1; flags.apply_loop_filter = thr ? 1 : 0; flags.pad_reference = 1;
    ed_setup S;
    if (const int32_t e = ed_prepare(ctx, w, n_pics, pics, width, height, mi_stride, q_index, &flags, thr, true, allow_intra, S)) return e;
    const ed_batch_dev &hb = S.hb;
    const ed_batch_dev *dB = S.dB;
    uint32_t intra_mask = 0; /* (ED_MAX_PICS = 32 pictures: one bit each) */
    for (int i = 0; i < n_pics; i++) intra_mask |= pics[i].has_intra ? 1u << i : 0u;
    HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(int32_t), ctx->stream));
    /* 1. inter prediction of the whole batch */
    ED_STAGE(SVT_ENCDEC_STAGE_MC);
    int32_t rc = svt_hip_inter_pred_batch_device(ctx, n_pics, S.mcp);
    if (rc) return rc;
    /* 2. transform blocks from the grids */
    ED_STAGE(SVT_ENCDEC_STAGE_LISTS);
    rc = ed_lists(ctx, w, hb, dB);
    if (rc) return rc;
    hipLaunchKernelGGL(svt_dec_intra_check_kernel, dim3((n_pics * hb.mi_rows * hb.mi_cols + 255) / 256), dim3(256), 0, ctx->stream, dB, w->d_status, intra_mask);
    HIP_TRY(hipGetLastError());
    /* 3. coefficients -> dequantisation -> inverse transform -> reconstruction; d_status[0] = coefficients that overflowed 16 bits */
    ED_STAGE(SVT_ENCDEC_STAGE_TQ);
    int32_t cap[4];
    ed_block_caps(hb, cap);
    rc = svt_rc_launch_device_lists(ctx, (const uint8_t *)S.pred_lo, S.recon_set, S.n_sets, cap, w->d_off_cnt, w->d_qtabs, (const int16_t *)S.q_lo, w->d_eob, w->d_pos,
                                    &dB->pic[0].g, &dB->pic[0].eob_map, (int)sizeof(ed_pic_dev), dB->iscan_off, hb.sb_cols, (uint32_t *)d_status);
    if (rc) return rc;
    /* 3b. intra blocks of inter pictures: their inter neighbours are reconstructed now; the coefficient-driven wavefront kernel rebuilds them,
           one picture after the other (it marks their units' coefficient flags itself; the eob map is its input) */
    for (int i = 0; i < n_pics; i++)
        if (pics[i].has_intra) {
            rc = svt_intra_rc_launch(ctx, &pics[i], width, height, mi_stride, w->d_qtabs, hb.iscan_off, w->d_intra_sync, w->d_status, (uint32_t *)d_status, 1);
            if (rc) return rc;
        }
    /* 4. skip flags from the eobs (above) */
    ED_STAGE(SVT_ENCDEC_STAGE_SKIP);
    rc = ed_skip(ctx, w, hb, dB, true);
    if (rc) return rc;
    /* 5. deblocking (thr = NULL: the header's filter level is 0), 6. the reconstruction becomes a reference picture */
    return ed_tail(ctx, w, hb, dB, S.rec, S.lfm, S.lfm_stride, S.mi_rows_a, S.mi_cols_a, thr, S.n_rec_pad, S.rec_pad, pad_x, pad_y);
}
} // namespace

extern "C" int32_t svt_hip_decode_batch_device(svt_hip_ctx *ctx, svt_encdec_work *w, int32_t n_pics, const svt_encdec_picture *pics, int32_t width,
                                               int32_t height, int32_t mi_stride, int32_t q_index, const svt_lf_thresh *thr, int32_t pad_x, int32_t pad_y,
                                               int32_t *d_status) {
    return decode_batch(ctx, w, n_pics, pics, width, height, mi_stride, q_index, thr, pad_x, pad_y, d_status, false);
}

/* the same pass for batches whose pictures may carry has_intra: step 3b runs for them (include/svtvp9_hip.h) */
extern "C" int32_t svt_hip_decode_mixed_batch_device(svt_hip_ctx *ctx, svt_encdec_work *w, int32_t n_pics, const svt_encdec_picture *pics, int32_t width,
                                                     int32_t height, int32_t mi_stride, int32_t q_index, const svt_lf_thresh *thr, int32_t pad_x, int32_t pad_y,
                                                     int32_t *d_status) {
    return decode_batch(ctx, w, n_pics, pics, width, height, mi_stride, q_index, thr, pad_x, pad_y, d_status, true);
}

/* The decode twin of svt_hip_encdec_intra_device below: an intra picture rebuilt from its grid, coefficients and eob map by the
 * coefficient-driven wavefront kernel (intra_recon_kernel.hip), then the same tail.  The eob map is an input (not cleared); d_nz is cleared
 * and the kernel marks the units that hold coefficients, so svt_skip_update_kernel states the encode pass's rule (and a decoder's: a block
 * whose transform blocks are all empty is skipped for the loop filter).  Everything is checked before the first enqueue: a refusal leaves
 * every buffer as it was. */
extern "C" int32_t svt_hip_decode_intra_device(svt_hip_ctx *ctx, svt_encdec_work *w, const svt_encdec_picture *pic, int32_t width, int32_t height, int32_t mi_stride,
                                               int32_t q_index, const svt_lf_thresh *thr, int32_t pad_x, int32_t pad_y, int32_t *d_status) {
    ed_intra_setup S;
    if (const int32_t e = ed_intra_prepare(ctx, w, pic, width, height, mi_stride, q_index, thr != nullptr, false, "decode_intra", d_status ? nullptr : "null status", S)) return e;
    HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(int32_t), ctx->stream));
    ED_STAGE(SVT_ENCDEC_STAGE_TQ);
    HIP_TRY(hipMemsetAsync(pic->d_nz, 0, (size_t)mi_stride * S.hb.mi_rows, ctx->stream));
    int32_t rc = svt_intra_rc_launch(ctx, pic, width, height, mi_stride, w->d_qtabs, S.iscan_off, w->d_intra_sync, w->d_status, (uint32_t *)d_status, 0);
    if (rc) return rc;
    ED_STAGE(SVT_ENCDEC_STAGE_SKIP);
    rc = ed_skip(ctx, w, S.hb, S.dB, false);
    if (rc) return rc;
    return ed_tail(ctx, w, S.hb, S.dB, &S.rec, &S.lfm, &S.lfm_stride, &S.mi_rows, &S.mi_cols, thr, pic->no_pad ? 0 : 1, &S.rec, pad_x, pad_y);
}

/* An intra picture: prediction + transform + reconstruction by the wavefront kernel (intra_kernel.hip), then the same tail as a batch of
 * inter pictures -- skip flags, loop-filter masks, deblocking, border. */
extern "C" int32_t svt_hip_encdec_intra_device(svt_hip_ctx *ctx, svt_encdec_work *w, const svt_encdec_picture *pic, int32_t width, int32_t height, int32_t mi_stride,
                                               int32_t q_index, const svt_encdec_flags *flags, const svt_lf_thresh *thr, int32_t pad_x, int32_t pad_y) {
    const char *const own = !flags ? "bad argument" : !flags->do_recon ? "intra prediction needs the reconstruction (do_recon)" :
                            flags->apply_loop_filter && !thr ? "loop filter without thresholds" : nullptr;
    ed_intra_setup S;
    if (const int32_t e = ed_intra_prepare(ctx, w, pic, width, height, mi_stride, q_index, flags && flags->apply_loop_filter, true, "encdec_intra", own, S)) return e;
    ED_STAGE(SVT_ENCDEC_STAGE_TQ);
    HIP_TRY(hipMemsetAsync(pic->d_eob_map, 0, (size_t)(width / 4) * (height / 4) * 3 / 2 * sizeof(uint16_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(pic->d_nz, 0, (size_t)mi_stride * S.hb.mi_rows, ctx->stream));
    int32_t rc = svt_intra_launch(ctx, pic, width, height, mi_stride, w->d_qtabs, w->d_iscan, S.iscan_off, w->d_intra_sync, w->d_status, 0);
    if (rc) return rc;
    ED_STAGE(SVT_ENCDEC_STAGE_SKIP);
    rc = ed_skip(ctx, w, S.hb, S.dB, false);
    if (rc) return rc;
    return ed_tail(ctx, w, S.hb, S.dB, &S.rec, &S.lfm, &S.lfm_stride, &S.mi_rows, &S.mi_cols, flags->apply_loop_filter ? thr : nullptr,
                   flags->pad_reference && !pic->no_pad ? 1 : 0, &S.rec, pad_x, pad_y);
}

extern "C" int32_t svt_hip_md_intra_default_device(svt_hip_ctx *ctx, int32_t width, int32_t height, int32_t filter_level, svt_lf_mode_info *d_lf_mi, int32_t mi_stride) {
    if (!ctx || !d_lf_mi || width < 8 || height < 8 || (width & 7) || (height & 7) || mi_stride < (width >> 3))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_intra_default: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    return svt_md_intra_default_launch(ctx, d_lf_mi, mi_stride, height >> 3, width >> 3, filter_level);
}

extern "C" void svt_hip_encdec_work_set_stage_hook(svt_encdec_work *w, svt_encdec_stage_hook hook, void *user) {
    if (!w) return;
    w->hook = hook;
    w->hook_user = user;
}

extern "C" int32_t svt_hip_encdec_work_status(svt_hip_ctx *ctx, svt_encdec_work *w, int32_t counts[8]) {
    if (!ctx || !w) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "encdec_status: null");
    HIP_TRY(hipSetDevice(ctx->device));
    int32_t h[9];
    HIP_TRY(hipMemcpyAsync(h, w->d_off_cnt, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (counts) memcpy(counts, h, 8 * sizeof(int32_t));
    if (h[8]) {
        HIP_TRY(hipMemsetAsync(w->d_status, 0, sizeof(int32_t), ctx->stream));
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "encdec: malformed mode-info grid (block outside the picture, misaligned, or transform larger than its block)");
    }
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_encdec_work_download(svt_hip_ctx *ctx, svt_encdec_work *w, svt_tq_block *blocks, uint32_t *pos, uint16_t *eob, int32_t capacity) {
    int32_t c[8];
    const int32_t rc = svt_hip_encdec_work_status(ctx, w, c);
    if (rc) return rc;
    const int32_t total = c[3] + c[7];
    if (total > capacity) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "encdec_download: capacity");
    if (total > 0) {
        if (blocks) {
            if (!w->last_hb) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "encdec_download: no batch yet");
            if (!w->d_blocks && hipMalloc((void **)&w->d_blocks, w->cap_per_pic * (size_t)w->max_pics * sizeof(svt_tq_block)) != hipSuccess) {
                w->d_blocks = nullptr;
                return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "encdec_download: device memory");
            }
            const ed_batch_dev *dB = nullptr;
            if (stage_batch(ctx, *(const ed_batch_dev *)w->last_hb, &dB)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "encdec_download: descriptor buffers");
            hipLaunchKernelGGL(svt_tq_expand_kernel, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, dB, (const int32_t *)w->d_off_cnt, (const uint32_t *)w->d_pos, w->d_blocks);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(blocks, w->d_blocks, (size_t)total * sizeof(svt_tq_block), hipMemcpyDeviceToHost, ctx->stream));
        }
        if (pos) HIP_TRY(hipMemcpyAsync(pos, w->d_pos, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (eob) HIP_TRY(hipMemcpyAsync(eob, w->d_eob, (size_t)total * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return total;
}

extern "C" int32_t svt_hip_md_default_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_me_pu_result *const *d_results, int32_t width, int32_t height,
                                                   uint32_t lambda, int32_t filter_level, svt_mc_mode_info *const *d_mc_mi, svt_lf_mode_info *const *d_lf_mi,
                                                   int32_t mi_stride) {
    if (!ctx || n_pics < 1 || !d_results || !d_mc_mi || !d_lf_mi || width < 8 || height < 8 || (width & 7) || (height & 7) || mi_stride < (width >> 3))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_default: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    for (int first = 0; first < n_pics; first += ED_MAX_PICS) {
        const int n = n_pics - first < ED_MAX_PICS ? n_pics - first : ED_MAX_PICS;
        ed_batch_dev hb;
        memset(&hb, 0, sizeof hb);
        fill_dims(hb, n, width, height, mi_stride);
        hb.lambda = lambda; hb.filter_level = filter_level;
        for (int i = 0; i < n; i++) {
            if (!d_results[first + i] || !d_mc_mi[first + i] || !d_lf_mi[first + i]) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_default: null picture");
            hb.pic[i].res = d_results[first + i]; hb.pic[i].mc_mi = d_mc_mi[first + i]; hb.pic[i].lf_mi = d_lf_mi[first + i];
        }
        const ed_batch_dev *dB = nullptr;
        if (stage_batch(ctx, hb, &dB)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "md_default: descriptor buffers");
        hipLaunchKernelGGL(svt_md_default_kernel, dim3(n * hb.n_sb), dim3(64), 0, ctx->stream, dB);
        HIP_TRY(hipGetLastError());
    }
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_lf_build_masks_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_lf_mode_info *const *d_lf_mi, int32_t mi_stride, int32_t mi_rows,
                                                 int32_t mi_cols, svt_lf_mask *const *d_lfm) {
    if (!ctx || n_pics < 1 || !d_lf_mi || !d_lfm || mi_rows < 1 || mi_cols < 1 || mi_stride < mi_cols) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "lf_masks: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    for (int first = 0; first < n_pics; first += ED_MAX_PICS) {
        const int n = n_pics - first < ED_MAX_PICS ? n_pics - first : ED_MAX_PICS;
        ed_batch_dev hb;
        memset(&hb, 0, sizeof hb);
        fill_dims(hb, n, mi_cols * 8, mi_rows * 8, mi_stride);
        for (int i = 0; i < n; i++) {
            if (!d_lf_mi[first + i] || !d_lfm[first + i]) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "lf_masks: null picture");
            hb.pic[i].lf_mi = (svt_lf_mode_info *)d_lf_mi[first + i]; hb.pic[i].lfm = d_lfm[first + i];
        }
        const ed_batch_dev *dB = nullptr;
        if (stage_batch(ctx, hb, &dB)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "lf_masks: descriptor buffers");
        if (const int32_t e = ed_lf_masks(ctx, dB, n, hb.n_sb, nullptr)) return e;
    }
    return SVT_HIP_OK;
}

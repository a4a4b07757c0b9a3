/*
 * coef_update.hip -- the forward coefficient-probability update over batches of pictures (gfx950): token records and coef_counts -> the
 * coefficient section of the compressed header as bool records, and the probabilities the tile is coded with.
 *
 * Replaces update_coef_probs (Source/Lib/VPX/vp9_bitstream.c:669-687) over build_tree_distribution (:511-531), the TWO_LOOP form of
 * update_coef_probs_common (:542-612) and VPX/vp9_subexp.c; the rules are stated once in coef_update_core.h:
 *   count    CU_ITEMS records per workgroup and pass, grid-stride over a picture (grid.y = the picture, the total read on the device):
 *            which records code node 0, into a 576-bin LDS histogram; every workgroup writes its histogram to the context's buffer --
 *            no global atomics, and the bins are 32-bit
 *   decide   one workgroup per (picture, transform size): 144 lanes sum the partial histograms (eob_branch); lane l takes entries 2 l and
 *            2 l + 1 of the size's 396 and runs their searches (up to 254 candidates; nine cost terms each for the pivot node) on a copy
 *            of the cost table in LDS; update count and savings are reduced over the workgroup, the records of an entry are a function
 *            of (u, newp, oldp) alone, so their places are a scan; the size's records go to its own range of the context's buffer, its
 *            432 probabilities and its part of the result record to the picture's outputs
 *   join     one workgroup per picture: prefix || the four sections || suffix into d_hdr_bools, their number, the segment, the result's
 *            totals.  A third launch and not the last-arriving workgroup of decide: stream order is the only dependence, nothing waits
 *            on another workgroup and nothing needs a counter that has to be cleared between calls
 * The pictures of a batch are independent: each is measured against its own d_old_probs (or the context's table).
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"
#include "coef_update_core.h"
#include "wave_ops.h"

#define CU_ITEMS 1024    /* records per workgroup and pass: 256 lanes x 4 */
#define CU_MAX_WGS 64    /* workgroups of a picture in the count kernel */
#define CU_SECT_STRIDE 4760 /* records of a size's range: 1 + SVT_CU_ENTRIES * SVT_CU_MAX_PER_ENTRY = 4753, rounded up to 16 bytes */

extern "C" int32_t svt_cu_check_picture(const svt_cu_picture *p);

namespace {

static_assert(CU_SECT_STRIDE >= 1 + SVT_CU_ENTRIES * SVT_CU_MAX_PER_ENTRY && CU_SECT_STRIDE % 8 == 0, "a size's range holds its section");
static_assert(2 * 256 >= SVT_CU_ENTRIES, "two entries a lane");

struct cu_pic_dev {
    svt_cu_picture p;
    const uint8_t *old;     /* p.d_old_probs or the context's table */
    uint32_t      *part;    /* wgs x 576 partial histograms */
    uint16_t      *sect;    /* 4 x CU_SECT_STRIDE records */
    uint32_t      *sect_n;  /* 4: records of each section */
};
struct cu_batch_dev {
    uint16_t   cost[256];
    uint32_t   wgs, pad_[3];
    cu_pic_dev s[SVT_CU_MAX_PICS];
};

__device__ __forceinline__ uint32_t pic_tokens(const svt_cu_picture &p) {
    const uint32_t n = p.d_n_tokens ? *p.d_n_tokens : p.n_tokens;
    return n < p.max_tokens ? n : p.max_tokens;
}

__global__ __launch_bounds__(256) void svt_cu_count_kernel(const cu_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_h[SVT_CU_ROWS];
    const cu_pic_dev &P = B->s[blockIdx.y];
    const uint32_t    tid = threadIdx.x, n = pic_tokens(P.p), stride = B->wgs * CU_ITEMS;
    for (uint32_t i = tid; i < SVT_CU_ROWS; i += 256) s_h[i] = 0;
    __syncthreads();
    const uint32_t *tok = P.p.d_tokens;
    for (uint64_t base = (uint64_t)blockIdx.x * CU_ITEMS; base < n; base += stride) /* (64-bit: base + stride may pass 2^32) */
        _Pragma("unroll") for (int j = 0; j < 4; j++) {
            const uint64_t i = base + (uint32_t)j * 256 + tid;
            if (i >= n) continue;
            const uint32_t rec = tok[i], row = SVT_TOK_PROB_ROW(rec);
            if (row < SVT_CU_ROWS && svt_cu_node0_coded(rec, i > 0, i > 0 ? tok[i - 1] : 0u)) atomicAdd(&s_h[row], 1u);
        }
    __syncthreads();
    for (uint32_t i = tid; i < SVT_CU_ROWS; i += 256) P.part[(size_t)blockIdx.x * SVT_CU_ROWS + i] = s_h[i];
}

__global__ __launch_bounds__(256) void svt_cu_decide_kernel(const cu_batch_dev *__restrict__ B, const svt_bool_tables *__restrict__ tables) {
    __shared__ uint16_t  s_cost[256];
    __shared__ uint32_t  s_eob[144];
    __shared__ uint8_t   s_probs[432];
    __shared__ uint32_t  s_wu[4], s_wn[4];
    __shared__ long long s_ws[4];
    const cu_pic_dev &P = B->s[blockIdx.y];
    const int         t = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    s_cost[tid] = B->cost[tid];
    for (int i = tid; i < 432; i += 256) s_probs[i] = P.old[432 * t + i];
    if (tid < 144) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < B->wgs; w++) sum += P.part[(size_t)w * SVT_CU_ROWS + 144 * t + tid];
        s_eob[tid] = sum;
        P.p.d_eob_branch[144 * t + tid] = sum;
    }
    __syncthreads();
    const bool searched = svt_cu_tx_total(s_eob) > SVT_CU_TX_TOTAL_MIN;
    int        u[2] = {0, 0}, newp[2] = {0, 0}, oldp[2] = {0, 0}, at[2] = {0, 0};
    long long  sav = 0;
    uint32_t   upd = 0;
    if (searched)
        _Pragma("unroll") for (int k = 0; k < 2; k++) {
            const int e = 2 * tid + k;
            if (e >= SVT_CU_ENTRIES) continue;
            int       node;
            const int row = svt_cu_entry(e, &node);
            int64_t   s;
            at[k] = 3 * row + node;
            oldp[k] = svt_cu_old(s_probs[at[k]]);
            u[k] = svt_cu_entry_decide(P.p.d_counts + 12 * (size_t)(144 * t + row), s_eob[row], node, oldp[k], s_cost, tables->pareto, &newp[k], &s);
            sav += svt_cu_entry_savings(u[k], s, s_cost);
            upd += (uint32_t)u[k];
        }
    const uint32_t  wu = wave_sum(upd);
    const long long ws = wave_sum(sav);
    if (lane == 0) { s_wu[wv] = wu; s_ws[wv] = ws; }
    __syncthreads();
    const uint32_t updates = s_wu[0] + s_wu[1] + s_wu[2] + s_wu[3];
    const int64_t  savings = s_ws[0] + s_ws[1] + s_ws[2] + s_ws[3];
    const bool     send = searched && svt_cu_send(updates, savings);
    uint32_t       cnt = 0;
    if (send)
        _Pragma("unroll") for (int k = 0; k < 2; k++)
            if (2 * tid + k < SVT_CU_ENTRIES) cnt += (uint32_t)svt_cu_entry_records(u[k], newp[k], oldp[k]);
    const uint32_t ex = wave_excl_prefix(cnt, lane);
    if (lane == 63) s_wn[wv] = ex + cnt;
    __syncthreads();
    uint32_t off = 1 + ex;
    for (int i = 0; i < wv; i++) off += s_wn[i];
    uint16_t *sect = P.sect + (size_t)t * CU_SECT_STRIDE;
    if (send)
        _Pragma("unroll") for (int k = 0; k < 2; k++) {
            if (2 * tid + k >= SVT_CU_ENTRIES) continue;
            off += (uint32_t)svt_cu_emit(u[k], newp[k], oldp[k], sect + off);
            if (u[k]) s_probs[at[k]] = (uint8_t)newp[k];
        }
    if (tid == 0) {
        sect[0] = SVT_BOOL_RECORD(send ? 1 : 0, 128);
        P.sect_n[t] = 1 + s_wn[0] + s_wn[1] + s_wn[2] + s_wn[3];
        P.p.d_result->updated[t] = updates;
        P.p.d_result->sent[t] = send;
        P.p.d_result->savings[t] = savings;
    }
    __syncthreads();
    for (int i = tid; i < 432; i += 256) P.p.d_probs[432 * t + i] = s_probs[i];
}

__global__ __launch_bounds__(256) void svt_cu_join_kernel(const cu_batch_dev *__restrict__ B) {
    const cu_pic_dev &P = B->s[blockIdx.x];
    const uint32_t    tid = threadIdx.x;
    uint16_t         *out = P.p.d_hdr_bools;
    uint32_t          n = P.p.n_prefix;
    for (uint32_t i = tid; i < P.p.n_prefix; i += 256) out[i] = P.p.prefix[i];
    for (int t = 0; t < 4; t++) {
        const uint32_t  most = 1 + SVT_CU_ENTRIES * SVT_CU_MAX_PER_ENTRY, m = P.sect_n[t] < most ? P.sect_n[t] : most; /* (never more: the capacity's proof) */
        const uint16_t *src = P.sect + (size_t)t * CU_SECT_STRIDE;
        for (uint32_t i = tid; i < m; i += 256) out[n + i] = src[i];
        n += m;
    }
    for (uint32_t i = tid; i < P.p.n_suffix; i += 256) out[n + i] = P.p.suffix[i];
    n += P.p.n_suffix;
    if (tid == 0) {
        *P.p.d_n_hdr_bools = n;
        P.p.d_segment->first = 0; P.p.d_segment->count = n; P.p.d_segment->kind = 1;
        P.p.d_result->hdr_bools = n;
        P.p.d_result->tokens = pic_tokens(P.p);
    }
}

size_t cu_align16(size_t v) { return (v + 15) & ~(size_t)15; }

} // namespace

extern "C" void svt_hip_coef_update_geometry(int32_t *records_per_pass, int32_t *max_workgroups) {
    if (records_per_pass) *records_per_pass = CU_ITEMS;
    if (max_workgroups) *max_workgroups = CU_MAX_WGS;
}

extern "C" int32_t svt_hip_coef_update_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_cu_picture *pics) {
    if (!ctx || !pics || n_pics < 1 || n_pics > SVT_CU_MAX_PICS) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "coef_update: bad argument");
    uint32_t wgs = 1;
    for (int i = 0; i < n_pics; i++) {
        if (svt_cu_check_picture(&pics[i])) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "coef_update: null picture field or too many header records");
        const uint32_t w = (uint32_t)(((uint64_t)pics[i].max_tokens + CU_ITEMS - 1) / CU_ITEMS);
        wgs = w > wgs ? w : wgs;
    }
    wgs = wgs > CU_MAX_WGS ? CU_MAX_WGS : wgs;
    if (!ctx->slot_bytes[SVT_SLOT_BC_TABLES]) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "coef_update: svt_hip_boolcode_set_tables has not been called");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t per_pic = cu_align16(sizeof(uint32_t) * (size_t)wgs * SVT_CU_ROWS) + cu_align16(sizeof(uint16_t) * 4 * CU_SECT_STRIDE) + 16;
    uint8_t     *scratch = (uint8_t *)svt_ctx_slot(ctx, SVT_SLOT_CU_SCRATCH, per_pic * (size_t)n_pics);
    if (!scratch) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "coef_update: scratch");
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof(cu_batch_dev), &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "coef_update: descriptor buffers");
    const svt_bool_tables *dT = (const svt_bool_tables *)ctx->slot[SVT_SLOT_BC_TABLES];
    svt_ctx_timer          timer(ctx);
    HIP_TRY(timer.begin());
    cu_batch_dev *hb = (cu_batch_dev *)h;
    memset(hb, 0, sizeof *hb);
    memcpy(hb->cost, svt_hip_coef_update_cost_table(), sizeof hb->cost);
    hb->wgs = wgs;
    for (int i = 0; i < n_pics; i++) {
        cu_pic_dev &P = hb->s[i];
        P.p = pics[i];
        P.old = pics[i].d_old_probs ? pics[i].d_old_probs : dT->coef_probs;
        P.part = (uint32_t *)scratch; scratch += cu_align16(sizeof(uint32_t) * (size_t)wgs * SVT_CU_ROWS);
        P.sect = (uint16_t *)scratch; scratch += cu_align16(sizeof(uint16_t) * 4 * CU_SECT_STRIDE);
        P.sect_n = (uint32_t *)scratch; scratch += 16;
    }
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof(cu_batch_dev)));
    const cu_batch_dev *dB = (const cu_batch_dev *)d;
    hipLaunchKernelGGL(svt_cu_count_kernel, dim3(wgs, n_pics), dim3(256), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_cu_decide_kernel, dim3(4, n_pics), dim3(256), 0, ctx->stream, dB, dT);
    hipLaunchKernelGGL(svt_cu_join_kernel, dim3(n_pics), dim3(256), 0, ctx->stream, dB);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}

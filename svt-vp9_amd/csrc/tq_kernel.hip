/*
 * tq_kernel.hip -- residual -> forward DCT/ADST -> quantise/dequantise -> inverse transform + reconstruction
 * for batches of VP9 transform blocks (gfx950).
 *
 * Replaces the per-block body of perform_coding_loop (Source/Lib/Codec/EbEncDecProcess.c:365-587):
 *   eb_vp9_residual_kernel (C_DEFAULT/EbPictureOperators_C.c:204) -> eb_vp9_fdct32x32 / eb_vpx_partial_fdct32x32 /
 *   eb_vp9_fht16x16 / fht8x8 / fht4x4 / eb_vpx_fdct4x4 (VPX/fwd_txfm.c, VPX/vp9_dct.c) -> eb_vp9_quantize_b[_32x32]
 *   (VPX/quantize.c:112-254) -> pic_copy + eb_vp9_idct*_add / eb_vp9_iht*_add (VPX/vp9_idct.c:111-189, VPX/inv_txfm.c).
 *
 * Mapping: one N-point 1-D transform per lane, N lanes per NxN block, 64/N blocks per wave64 and 256/N per
 * workgroup; the column pass keeps a whole column in VGPRs, the transposition between the passes goes through a
 * padded (N+1 dwords per row) LDS tile so both passes are bank-conflict free; the eob is a max-reduction of
 * iscan positions over the block's N lanes (DPP/shuffle).  Integer butterflies on VALU -- no MFMA (these are
 * 32-bit integer rotations with data-dependent rounding/truncation, not dense contractions).
 * Source, prediction and reconstruction move as dword rows (lane i owns row i); the row <-> column changes go through the
 * same LDS tile; coefficient rows leave as 8/16-byte vectors (coeff_off and the two coefficient arrays must be 16-byte
 * aligned: every block starts on a multiple of 8 coefficients).  Global traffic per block: N*N source + N*N prediction bytes in, 2*N*N int16 (qcoeff, dqcoeff) + N*N recon out.
 *
 * The walks.  Every launch is persistent: a workgroup walks groups of blocks (256 4x4 blocks, 256 / N blocks otherwise) of its XCD's
 * eighth of the list (tq_walk_of).  An iteration needs the block's position code (or descriptor), from it the picture's geometry
 * record, from that the 2 N rows of source and prediction: three dependent round trips, two of them to lines nobody has touched, in
 * front of ~500 (4x4) / ~700 (8x8) vector instructions.  The 4x4 and 8x8 instances without the fused rate pass walk software-pipelined
 * (tq_pipelined): after a prologue that fetches the first group, an iteration
 *     loads both descriptors -- its own group's, whole, and the address fields of the next group's -- and waits for them (lines the
 *         previous iteration has just read: one short round trip),
 *     issues the row loads of group gj + step and the position-code load of group gj + 2 step, waits for neither,
 *     runs the body of group gj on the rows the previous iteration fetched (tq_block_body / tq_lane_block take them as arguments),
 *     and moves the fetched registers down.
 * The prefetch is predicated like the loop: no load is issued for a group at or beyond n_blocks (the list's tail need not be readable),
 * and the idle slots of a partly filled last group work on block 0 and store nothing, as before.  The wait in the first step is
 * explicit (tq_loads_landed): loads return in order, so a wait that the compiler places behind the far loads for one of the near ones
 * would wait for the far ones too.  What it costs: 14 - 16 registers (4x4: 63 -> 77, 8x8: 62 -> 78; both were in the 64-register
 * class, both are now in the 80-register one), no scratch.  The 16x16 instance would need 108 (> 96: one wave per SIMD less) and the
 * 32x32 one sits at 128 with scalar spills: both keep the serial walk, as do the instances with the fused rate pass (the 4x4 one: 129
 * registers pipelined instead of 113, a wave per SIMD less).
 *
 * The grids.  In the encode pass the launches run beside motion estimation, whose five workgroups per CU leave 112 registers per SIMD
 * and 3 LDS granules: a CU on which more than that moves in loses ME workgroups for as long as it stays.  The mode-decision
 * entry points keep six workgroups per CU (TQ_PER_2CU); svt_tq_launch_device_lists launches TQ_PER_2CU_ENC per size, chosen from a sweep
 * of the bench step (profiles/tq_prefetch.md):
 *     4x4: one workgroup on every other CU (128 on this part).  One wave of 80 registers and no LDS per SIMD is the only form of this
 *         stage that fits beside FIVE ME workgroups, and the step is fastest there: 6 465 frames/s for the parent, 6 740 at 128
 *         workgroups, 6 610 - 6 735 at 192 - 384, 6 515 at 1 536; below 128 the launch itself becomes the chain's long pole (64: 6 665,
 *         32: 5 640).  The same grid under the serial loop gives 6 690: most of the gain is the grid, the prefetch adds what lets
 *         so few waves keep up.
 *     8x8, 16x16, 32x32: two workgroups per CU.  Their LDS tiles (8 / 14 / 27 granules) cost a CU one ME workgroup whatever the
 *         count; between one and six per CU the step moves by less than its run-to-run spread, except 32x32 at one on every other CU
 *         (-1.3 %) and all three at six per CU together (-1.7 %).
 */
#include <hip/hip_runtime.h>
#include <type_traits>
#include "tq_core.h"

namespace {

/* The pipelined walks put this between the loads of the descriptors and the loads they send ahead for later groups.  Loads return in
 * order: a wait for an older load that the compiler places AFTER the younger, far ones have been issued waits for those too -- and where
 * two paths meet it has to place the wait that is safe on both.  With the descriptors landed here, the first thing a block body waits for
 * is a table load of its own, two transform passes later. */
__device__ __forceinline__ void tq_loads_landed() { __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0); expcnt, lgkmcnt untouched */ }

/* which instances walk their list software-pipelined (file comment) */
template <int N, bool RATE, bool DIST> constexpr bool tq_pipelined() { return N < 16 && !RATE; }

/* 32x32: 54 KB of LDS per 256-thread workgroup (eight blocks + the rate tables) allow three workgroups = 12 waves per CU */
template <int N, bool RATE, bool DIST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(N == 32 ? (RATE ? 3 : 4) : 1))) void svt_tq_kernel(const uint8_t *__restrict__ src, const uint8_t *__restrict__ pred,
                                                     uint8_t *__restrict__ recon, const svt_tq_block *__restrict__ blocks,
                                                     int n_blocks, const svt_quant_tables *__restrict__ qtabs,
                                                     const int16_t *__restrict__ iscan_all, int16_t *__restrict__ qcoeff,
                                                     int16_t *__restrict__ dqcoeff, uint16_t *__restrict__ eob_out,
                                                     uint64_t *__restrict__ dist_out, tq_rate_args ra, const uint8_t *const *__restrict__ recon_set, tq_dev_count dc) {
    {   /* device-built list: where this size's blocks start and how many there are */
        const int o = dc.first_block(n_blocks);
        blocks += o; eob_out += o;
        if (dist_out) dist_out += 2 * o;
        if constexpr (RATE) ra.bits += o;
    }
    constexpr int BPW = TQ_THREADS / N;   /* blocks per workgroup */
    constexpr int LS  = N + 1;            /* padded LDS row stride in dwords */
    __shared__ int32_t tile[BPW][N * LS];
    /* RATE: the four token-cost slices [plane_type][is_inter] of this transform size, copied once per (persistent) workgroup */
    __shared__ uint32_t s_tc[RATE ? 4 * RATE_SLICE : 1];
    /* ... and the {scan, neighbours} tables of this size (all four transform types; one for 32x32): the walk's three table
     * reads per position then cost an LDS access instead of a dependent global round trip */
    /* (the two entries that close a table -- the neighbours of position n -- are never read: a walk ends at position eob <= n - 1 or,
     * for a full block, without an EOB token; leaving them out of the single 32x32 table keeps that instance at 53 760 bytes = 42 LDS
     * granules, three workgroups per CU instead of two) */
    constexpr int SCAN_T = 3 * N * N + 2, SCAN_N = N == 32 ? 3 * N * N : 4 * SCAN_T;
    __shared__ int16_t s_scan[RATE ? SCAN_N : 2];
    if constexpr (RATE) {
        const uint32_t *g = &ra.T->token_costs[txcfg<N>::size][0][0][0][0][0][0];
        for (int j = threadIdx.x; j < 4 * RATE_SLICE; j += TQ_THREADS) s_tc[j] = g[j];
        const uint32_t *gs = (const uint32_t *)(ra.scan + rate_scan_offset(txcfg<N>::size, 0)); /* 4-byte aligned, even count */
        for (int j = threadIdx.x; j < SCAN_N / 2; j += TQ_THREADS) ((uint32_t *)s_scan)[j] = gs[j];
        __syncthreads();
    }
    const int lb  = threadIdx.x / N;      /* block slot inside the workgroup */
    const int i   = threadIdx.x % N;      /* column (pass 1) / row (pass 2) owned by this lane */
    const tq_walk wk = tq_walk_of((n_blocks + BPW - 1) / BPW);
    /* group gj of this workgroup's walk exists (uniform: depends on the workgroup only; once false it stays false) */
    auto in_walk = [&](int gj) { return gj < wk.per_xcd && (wk.base + gj) * BPW < n_blocks; };
    /* the lane's block of group gj; the idle slots of a partly filled last group work on block 0 and store nothing */
    auto code_of = [&](int gj) { const int blk = (wk.base + gj) * BPW + lb; return dc.pos[blk < n_blocks ? blk : 0]; };
    /* POS (dc.pos != null): the list holds position codes and the descriptor is rebuilt in registers */
    auto block_of = [&](auto POS, int gj, uint32_t pc, svt_tq_block &k) {
        const int blk = (wk.base + gj) * BPW + lb;
        if constexpr (decltype(POS)::value)
            tq_block_of_pos<N>(dc, pc, &k);
        else k = blocks[blk < n_blocks ? blk : 0];
    };
    /* lane i fetches ROW i of source and prediction as dwords (coalesced: the N lanes of a block read N consecutive rows of N bytes);
     * of the descriptor only the address fields are used */
    auto rows_of = [&](int gj, const svt_tq_block &k, uint32_t (&srow)[N / 4], uint32_t (&prow)[N / 4]) {
        _Pragma("unroll") for (int q = 0; q < N / 4; q++) { srow[q] = 0u; prow[q] = 0u; }
        if ((wk.base + gj) * BPW + lb >= n_blocks) return;
        const uint8_t *sp = src + k.src_off + (size_t)i * k.src_stride;
        const uint8_t *pp = pred + k.pred_off + (size_t)i * k.pred_stride;
        constexpr uintptr_t AM = N >= 16 ? 15 : N - 1;
        row_load<N>(sp, ((uintptr_t)sp & AM) == 0, srow); row_load<N>(pp, ((uintptr_t)pp & AM) == 0, prow);
    };
    auto body_of = [&](int gj, const svt_tq_block &k, const uint32_t (&srow)[N / 4], const uint32_t (&prow)[N / 4]) {
        const int  blk = (wk.base + gj) * BPW + lb;
        const bool active = blk < n_blocks;
        /* a batch may reconstruct into several buffers (reference pictures of different mini-GOPs): pad_[0] bits 4-6 name the one */
        int32_t *bits_slot = nullptr;
        if constexpr (RATE) bits_slot = ra.bits + blk;
        tq_block_body<N, RATE, DIST>(k, active, i, tile[lb], srow, prow, qtabs, iscan_all, qcoeff, dqcoeff, eob_out + blk, dist_out ? dist_out + 2 * blk : nullptr, bits_slot,
                                     ra.T, s_tc, s_scan, recon_set ? (uint8_t *)recon_set[(k.pad_[0] >> 4) & 7] : recon);
        tq_block_sync(); /* the block's tile is rewritten by its lanes' next block */
    };
    int gj = wk.first;
    if constexpr (!tq_pipelined<N, RATE, DIST>()) { /* the serial walk: fetch, then compute (spelled out: written with the helpers above the
                                                     * 32x32 instance gets a vector spill) */
        for (; gj < wk.per_xcd; gj += wk.step) {
            const int grp = wk.base + gj;
            if (grp * BPW >= n_blocks) break;     /* uniform: depends on the workgroup only */
            const int blk = grp * BPW + lb;
            const bool active = blk < n_blocks;
            svt_tq_block k;
            if (dc.pos) { /* (uniform) the list holds position codes: the descriptor is rebuilt in registers */
                const uint32_t pc = dc.pos[active ? blk : 0];
                tq_block_of_pos<N>(dc, pc, &k);
            } else if (active) k = blocks[blk];
            else { k = blocks[0]; }
            int32_t *t = tile[lb];
            uint32_t srow[N / 4], prow[N / 4];
            {
                const uint8_t *sp = src + k.src_off + (size_t)i * k.src_stride;
                const uint8_t *pp = pred + k.pred_off + (size_t)i * k.pred_stride;
                constexpr uintptr_t AM = N >= 16 ? 15 : N - 1;
                _Pragma("unroll") for (int q = 0; q < N / 4; q++) { srow[q] = 0u; prow[q] = 0u; }
                if (active) { row_load<N>(sp, ((uintptr_t)sp & AM) == 0, srow); row_load<N>(pp, ((uintptr_t)pp & AM) == 0, prow); }
            }
            int32_t *bits_slot = nullptr;
            if constexpr (RATE) bits_slot = ra.bits + blk;
            tq_block_body<N, RATE, DIST>(k, active, i, t, srow, prow, qtabs, iscan_all, qcoeff, dqcoeff, eob_out + blk, dist_out ? dist_out + 2 * blk : nullptr, bits_slot,
                                         ra.T, s_tc, s_scan, recon_set ? (uint8_t *)recon_set[(k.pad_[0] >> 4) & 7] : recon);
            tq_block_sync(); /* the block's tile is rewritten by its lanes' next block */
        }
    } else {
        /* software-pipelined walk (file comment): while group gj computes, the rows of group gj + step and the position codes of
         * group gj + 2 step are in flight.  Nothing is loaded for a group that is not in the walk.  One copy of the loop per list form,
         * so that the loads of an iteration's descriptors sit in one basic block and are waited for once. */
        auto walk = [&](auto POS) {
            constexpr bool P = decltype(POS)::value;
            bool     have0 = in_walk(gj), have1 = have0 && in_walk(gj + wk.step);
            uint32_t pc0 = 0u, pc1 = 0u, s0[N / 4], p0[N / 4];
            if constexpr (P) { if (have0) pc0 = code_of(gj); if (have1) pc1 = code_of(gj + wk.step); }
            if (have0) { svt_tq_block k; block_of(POS, gj, pc0, k); rows_of(gj, k, s0, p0); }
            while (have0) {
                const int  g1 = gj + wk.step, g2 = g1 + wk.step;
                const bool have2 = have1 && in_walk(g2);
                uint32_t   pc2 = 0u, s1[N / 4], p1[N / 4];
                /* both descriptors first: this group's, whole, and the address fields of the next one's (this group's again when
                 * there is no next) -- lines that the previous iteration or a neighbour has just read */
                svt_tq_block k, kn;
                block_of(POS, gj, pc0, k);
                block_of(POS, have1 ? g1 : gj, have1 ? pc1 : pc0, kn);
                tq_loads_landed();
                if (have1) rows_of(g1, kn, s1, p1);
                else { _Pragma("unroll") for (int q = 0; q < N / 4; q++) { s1[q] = 0u; p1[q] = 0u; } }
                if constexpr (P) { if (have2) pc2 = code_of(g2); }
                body_of(gj, k, s0, p0);
                _Pragma("unroll") for (int q = 0; q < N / 4; q++) { s0[q] = s1[q]; p0[q] = p1[q]; }
                pc0 = pc1; pc1 = pc2; gj = g1; have0 = have1; have1 = have2;
            }
        };
        if (dc.pos) walk(std::true_type{}); else walk(std::false_type{});
    }
}


/* ---- coefficient rate of a 4x4 block inside the lane that owns it ----
 * The three 4x4 scan orders of VP9 (VPX/vp9_scan.c: default_scan_4x4 for DCT_DCT and ADST_ADST, row_scan_4x4 for ADST_DCT,
 * col_scan_4x4 for DCT_ADST) with their neighbour pairs are compile-time tables here, so that the unrolled walk over the
 * scan positions addresses the lane's 16 token / energy registers with constant indices: no LDS staging of the coefficients,
 * no cross-lane step.  svt_hip_rate_scan4x4_table exposes them; tests/test_rate.py checks them against the reference's tables
 * (the scan array the caller passes must hold the same ones -- they are normative).  */
struct scan4_tab { uint8_t scan[16], nb[32]; };
constexpr scan4_tab SCAN4[3] = {
    {{0, 4, 1, 5, 8, 2, 12, 9, 3, 6, 13, 10, 7, 14, 11, 15},
     {0, 0, 0, 0, 0, 0, 1, 4, 4, 4, 1, 1, 8, 8, 5, 8, 2, 2, 2, 5, 9, 12, 6, 9, 3, 6, 10, 13, 7, 10, 11, 14}},
    {{0, 1, 4, 2, 5, 3, 6, 8, 9, 7, 12, 10, 13, 11, 14, 15},
     {0, 0, 0, 0, 0, 0, 1, 1, 4, 4, 2, 2, 5, 5, 4, 4, 8, 8, 6, 6, 8, 8, 9, 9, 12, 12, 10, 10, 13, 13, 14, 14}},
    {{0, 4, 8, 1, 12, 5, 9, 2, 13, 6, 10, 3, 7, 14, 11, 15},
     {0, 0, 0, 0, 4, 4, 0, 0, 8, 8, 1, 1, 5, 5, 1, 1, 9, 9, 2, 2, 6, 6, 2, 2, 3, 3, 10, 10, 7, 7, 11, 11}}};
constexpr uint8_t BAND4[16] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 5};
__host__ __device__ constexpr int scan4_kind(int tx_type) { return tx_type == SVT_ADST_DCT ? 1 : tx_type == SVT_DCT_ADST ? 2 : 0; }

/* tok[r] / en[r]: token and energy class of raster coefficient r; tc: the block's cost slice in LDS.  Position c contributes
 * tc[band][previous token == ZERO][ctx][token] while c < eob and the EOB token at c == eob (< 16); the position-independent
 * value costs are added by the caller.  The loop is unrolled; it leaves as soon as no lane of the wave has c <= eob. */
template <int K>
__device__ __forceinline__ int rate_walk4(const int (&tok)[16], const int (&en)[16], const uint32_t *tc, int eob, int ctx0) {
    int sum = (int)tc[ctx0 * 12 + (eob == 0 ? 11 : tok[0])];
    _Pragma("unroll") for (int c = 1; c < 16; c++) {
        if (!__any(c <= eob)) break;
        const int  pt = (1 + en[SCAN4[K].nb[2 * c]] + en[SCAN4[K].nb[2 * c + 1]]) >> 1;
        const bool in = c < eob;
        const int  pz = in && tok[SCAN4[K].scan[c - 1]] == 0, tk = in ? tok[SCAN4[K].scan[c]] : 11;
        const int  v  = (int)tc[((BAND4[c] * 2 + pz) * 6 + pt) * 12 + tk];
        sum += c <= eob ? v : 0;
    }
    return sum;
}

/* 4x4 blocks: one block per lane (why not 8x8 too: launch_tq).  With N lanes per block the small transforms are a sliver of the instruction
 * stream (descriptor decode and table loads repeated in every lane, LDS transposes, shuffles for eob and distortion: ~125
 * VALU lane-operations per sample, as many as a 32x32 block); a lane that owns the whole block keeps its samples in
 * registers from the residual to the reconstruction, needs no LDS, no barrier and no cross-lane step.  Same arithmetic as
 * svt_tq_kernel<N>: the fwd_txfm.c and vp9_dct.c forms of the DCT coincide (the int16 casts are no-ops at this size).  The inverse
 * always runs all rows (the reference's reduced variants are shortcuts with identical results).  Memory instructions per
 * block are unchanged (a lane issues the four row loads its four lanes issued). */
/* the four rows of source and prediction of a block, packed, into the calling lane */
__device__ __forceinline__ void tq_lane_rows(const svt_tq_block &k, const uint8_t *__restrict__ src, const uint8_t *__restrict__ pred, uint32_t (&srow)[4], uint32_t (&prow)[4]) {
    _Pragma("unroll") for (int r = 0; r < 4; r++) {
        srow[r] = *(const uint32_t *)(src + k.src_off + (size_t)r * k.src_stride);
        prow[r] = *(const uint32_t *)(pred + k.pred_off + (size_t)r * k.pred_stride);
    }
}

/* one 4x4 block, whole, in the calling lane: the body of svt_tq_lane_kernel.  srow / prow: its rows (tq_lane_rows) */
template <bool RATE, bool DIST>
__device__ __forceinline__ void tq_lane_block(const svt_tq_block &k, const int blk, const uint32_t (&srow)[4], const uint32_t (&prow)[4], uint8_t *__restrict__ recon,
                                              const svt_quant_tables *__restrict__ qtabs, const int16_t *__restrict__ iscan_all, int16_t *__restrict__ qcoeff,
                                              int16_t *__restrict__ dqcoeff, uint16_t *__restrict__ eob_out, uint64_t *__restrict__ dist_out, const tq_rate_args &ra,
                                              const uint32_t *s_tc, const int32_t *s_vc, const uint8_t *const *__restrict__ recon_set) {
    constexpr int N = 4;
    const bool col_adst = k.tx_type == SVT_ADST_DCT || k.tx_type == SVT_ADST_ADST;
    const bool row_adst = k.tx_type == SVT_DCT_ADST || k.tx_type == SVT_ADST_ADST;
    int32_t    m[N][N]; /* after the column pass: m[kk][cc] = vertical frequency kk of column cc */
    {
        _Pragma("unroll") for (int cc = 0; cc < N; cc++) {
            int32_t v[N], o[N];
            _Pragma("unroll") for (int r = 0; r < N; r++) v[r] = ((int)((srow[r] >> (8 * cc)) & 0xff) - (int)((prow[r] >> (8 * cc)) & 0xff)) * 16;
            if (cc == 0 && v[0]) ++v[0];
            if (col_adst) tx_fadst4(v, o); else tx_fdct4(v, o);
            _Pragma("unroll") for (int kk = 0; kk < N; kk++) m[kk][cc] = (int16_t)o[kk];
        }
    }
    /* quantiser tables of the block (lanes of one table read the same addresses) */
    const svt_quant_tables q = tq_load_qtab(qtabs, k.qtab);
    /* ---- row pass, quantisation, distortion, eob; each row of coefficients leaves as one 8-byte vector ---- */
    int32_t  dq[N][N];
    uint32_t rdist = 0, pdist = 0;
    int      eob = 0;
    int      tok[RATE ? 16 : 1], en[RATE ? 16 : 1], vsum = 0, nnz = 0; /* RATE: per raster coefficient */
    const uint32_t *ip = (const uint32_t *)(iscan_all + k.iscan_off);
    _Pragma("unroll") for (int i = 0; i < N; i++) {
        int32_t  o[N];
        uint32_t isw[N / 2], qw[N / 2], dqw[N / 2];
        _Pragma("unroll") for (int j = 0; j < N / 2; j++) isw[j] = ip[i * (N / 2) + j];
        if (row_adst) tx_fadst4(m[i], o);
        else { tx_fdct4(m[i], o); _Pragma("unroll") for (int kk = 0; kk < N; kk++) o[kk] = (int16_t)o[kk]; }
        _Pragma("unroll") for (int kk = 0; kk < N; kk++) {
            const int cv = (int16_t)((o[kk] + 1) >> 2);
            int       level, qv, dv;
            tq_quant_coeff<false>(q, (i | kk) != 0, cv, level, qv, dv);
            dq[i][kk] = dv;
            if constexpr (DIST) {
                const int dd = (int16_t)(cv - dv);
                rdist += (uint32_t)(dd * dd);
                pdist += (uint32_t)(cv * cv);
            }
            if (kk & 1) { qw[kk >> 1] |= (uint32_t)(uint16_t)qv << 16; dqw[kk >> 1] |= (uint32_t)(uint16_t)dv << 16; }
            else { qw[kk >> 1] = (uint16_t)qv; dqw[kk >> 1] = (uint16_t)dv; }
            if (level) { const int pos = (int)((isw[kk >> 1] >> (16 * (kk & 1))) & 0xffff) + 1; eob = pos > eob ? pos : eob; }
            if constexpr (RATE) {
                /* token, energy class and value cost of this coefficient; skipped when it is zero in every lane of the wave */
                tok[i * N + kk] = 0; en[i * N + kk] = 0;
                if (__any(level != 0)) {
                    const int al = qv < 0 ? -qv : qv; /* |level| as the reference sees it (the int16 qcoeff) */
                    tok[i * N + kk] = token_of(qv);
                    en[i * N + kk]  = energy_of_value(qv);
                    nnz += qv != 0;
                    int vc = s_vc[66 + (al < 67 ? qv : 0)];
                    if (__any(al >= 67)) { /* CAT6: vp9_get_token_cost, VPX/vp9_tokenize.h:118-127 */
                        const int extra = al >= 67 ? al - 67 : 0;
                        const int c6 = ra.T->cat6_low_cost[extra & 0xff] + ra.T->cat6_high_cost[extra >> 8];
                        vc = al >= 67 ? c6 : vc;
                    }
                    vsum += qv != 0 ? vc : 0;
                }
            }
        }
        int16_t *qo = qcoeff + k.coeff_off + i * N, *dqo = dqcoeff + k.coeff_off + i * N;
        *(uint2 *)qo = make_uint2(qw[0], qw[1]);
        if (dqcoeff) *(uint2 *)dqo = make_uint2(dqw[0], dqw[1]);
    }
    eob_out[blk] = (uint16_t)eob;
    if constexpr (DIST) if (dist_out) { dist_out[2 * blk] = rdist; dist_out[2 * blk + 1] = pdist; }
    if constexpr (RATE) {
        const int       rinfo = k.pad_[0], ptype = (rinfo >> 2) & 1, inter = (rinfo >> 3) & 1, ctx0 = rinfo & 3;
        const uint32_t *tc = s_tc + (ptype * 2 + inter) * RATE_SLICE;
        const int       kind = scan4_kind(k.tx_type);
        int             bits = 0;
        if (kind == 0) bits = rate_walk4<0>(tok, en, tc, eob, ctx0);
        if (kind == 1) bits = rate_walk4<1>(tok, en, tc, eob, ctx0);
        if (kind == 2) bits = rate_walk4<2>(tok, en, tc, eob, ctx0);
        /* value costs: every position before eob pays the cost of its value; the zeros among them pay value_cost[0 + 66] */
        ra.bits[blk] = bits + vsum + (eob - nnz) * s_vc[66];
    }
    if (!k.do_recon) return;
    /* ---- reconstruction: rows first, then columns (vp9_idct.c:111-189, inv_txfm.c); a column's four results go straight
     * into the packed output rows ---- */
    constexpr int SH = txcfg<N>::shift;
    uint32_t      rw[N] = {0, 0, 0, 0};
    const bool dc_only = k.tx_type == SVT_DCT_DCT && eob <= 1;
    if (eob != 0 && !dc_only) {
        int32_t t[N][N];
        _Pragma("unroll") for (int i = 0; i < N; i++) {
            int32_t o[N];
            inv1d<N>(dq[i], o, row_adst);
            _Pragma("unroll") for (int kk = 0; kk < N; kk++) t[i][kk] = (int16_t)o[kk];
        }
        _Pragma("unroll") for (int cc = 0; cc < N; cc++) {
            int32_t v[N], o[N];
            _Pragma("unroll") for (int r = 0; r < N; r++) v[r] = t[r][cc];
            inv1d<N>(v, o, col_adst);
            _Pragma("unroll") for (int r = 0; r < N; r++) {
                const int res = ((int16_t)o[r] + (1 << (SH - 1))) >> SH;
                rw[r] |= (uint32_t)clip_add((int)((prow[r] >> (8 * cc)) & 0xff), res) << (8 * cc);
            }
        }
    } else {
        int32_t a1 = 0;
        if (eob != 0) { /* eb_vp9_idct4x4_1_add_c, inv_txfm.c:174 */
            int32_t d = tx_rsw((int16_t)dq[0][0] * TX_C16);
            d = tx_rsw(d * TX_C16);
            a1 = (d + (1 << (SH - 1))) >> SH;
        }
        _Pragma("unroll") for (int r = 0; r < N; r++) {
            _Pragma("unroll") for (int cc = 0; cc < N; cc++) rw[r] |= (uint32_t)clip_add((int)((prow[r] >> (8 * cc)) & 0xff), a1) << (8 * cc);
        }
    }
    uint8_t *const rbase = recon_set ? (uint8_t *)recon_set[(k.pad_[0] >> 4) & 7] : recon;
    if (!rbase) return; /* a set index beyond the caller's n_set: nowhere to reconstruct to (never buffer 0 by default) */
    _Pragma("unroll") for (int r = 0; r < N; r++) *(uint32_t *)(rbase + k.recon_off + (size_t)r * k.recon_stride) = rw[r];
}

template <int N, bool RATE, bool DIST>
__global__ __launch_bounds__(256) void svt_tq_lane_kernel(const uint8_t *__restrict__ src, const uint8_t *__restrict__ pred,
                                                          uint8_t *__restrict__ recon, const svt_tq_block *__restrict__ blocks,
                                                          int n_blocks, const svt_quant_tables *__restrict__ qtabs,
                                                          const int16_t *__restrict__ iscan_all, int16_t *__restrict__ qcoeff,
                                                          int16_t *__restrict__ dqcoeff, uint16_t *__restrict__ eob_out,
                                                          uint64_t *__restrict__ dist_out, tq_rate_args ra, const uint8_t *const *__restrict__ recon_set, tq_dev_count dc) {
    static_assert(N == 4, "block-per-lane form: 4x4 only (launch_tq)");
    {   /* device-built list (svt_tq_kernel) */
        const int o = dc.first_block(n_blocks);
        blocks += o; eob_out += o;
        if (dist_out) dist_out += 2 * o;
        if constexpr (RATE) ra.bits += o;
    }
    /* RATE: the four 4x4 token-cost slices [plane_type][is_inter] and the value-cost table, copied once per workgroup */
    __shared__ uint32_t s_tc[RATE ? 4 * RATE_SLICE : 1];
    __shared__ int32_t  s_vc[RATE ? 136 : 1];
    if constexpr (RATE) {
        const uint32_t *g = &ra.T->token_costs[0][0][0][0][0][0][0];
        for (int j = threadIdx.x; j < 4 * RATE_SLICE; j += 256) s_tc[j] = g[j];
        if (threadIdx.x < 133) s_vc[threadIdx.x] = ra.T->value_cost[threadIdx.x];
        __syncthreads();
    }
    const tq_walk wk = tq_walk_of((n_blocks + 255) / 256);
    /* Software-pipelined walk (file comment), per lane: while the lane's block of group gj computes, the rows of its block of group
     * gj + step and the position code of its block of group gj + 2 step are in flight.  A lane loads nothing for a block at or beyond
     * n_blocks (once a lane is past the end it stays there); no barrier inside the loop. */
    auto blk_of = [&](int gj) { return (wk.base + gj) * 256 + (int)threadIdx.x; };
    auto in_walk = [&](int gj) { return gj < wk.per_xcd && blk_of(gj) < n_blocks; };
    auto block_of = [&](auto POS, int gj, uint32_t pc, svt_tq_block &k) {
        if constexpr (decltype(POS)::value) tq_block_of_pos<N>(dc, pc, &k);
        else k = blocks[blk_of(gj)];
    };
    if constexpr (!tq_pipelined<N, RATE, DIST>()) { /* the serial walk: fetch, then compute */
      for (int gj = wk.first; gj < wk.per_xcd; gj += wk.step) {
        const int blk = (wk.base + gj) * 256 + (int)threadIdx.x;
        if (blk >= n_blocks) continue; /* no barrier inside the loop */
        svt_tq_block k;
        if (dc.pos) {
            const uint32_t pc = dc.pos[blk];
            tq_block_of_pos<N>(dc, pc, &k);
        } else k = blocks[blk];
        uint32_t srow[4], prow[4];
        tq_lane_rows(k, src, pred, srow, prow);
        tq_lane_block<RATE, DIST>(k, blk, srow, prow, recon, qtabs, iscan_all, qcoeff, dqcoeff, eob_out, dist_out, ra, s_tc, s_vc, recon_set);
      }
      return;
    }
    auto walk = [&](auto POS) { /* one copy per list form (svt_tq_kernel) */
        constexpr bool P = decltype(POS)::value;
        int      gj = wk.first;
        bool     have0 = in_walk(gj), have1 = have0 && in_walk(gj + wk.step);
        uint32_t pc0 = 0u, pc1 = 0u, s0[4] = {}, p0[4] = {};
        if constexpr (P) { if (have0) pc0 = dc.pos[blk_of(gj)]; if (have1) pc1 = dc.pos[blk_of(gj + wk.step)]; }
        if (have0) { svt_tq_block k; block_of(POS, gj, pc0, k); tq_lane_rows(k, src, pred, s0, p0); }
        while (have0) {
            const int  g1 = gj + wk.step, g2 = g1 + wk.step;
            const bool have2 = have1 && in_walk(g2);
            uint32_t   pc2 = 0u, s1[4] = {}, p1[4] = {};
            svt_tq_block k, kn; /* this block's descriptor, whole, and the address fields of the lane's next (svt_tq_kernel) */
            block_of(POS, gj, pc0, k);
            block_of(POS, have1 ? g1 : gj, have1 ? pc1 : pc0, kn);
            tq_loads_landed();
            if (have1) tq_lane_rows(kn, src, pred, s1, p1);
            if constexpr (P) { if (have2) pc2 = dc.pos[blk_of(g2)]; }
            tq_lane_block<RATE, DIST>(k, blk_of(gj), s0, p0, recon, qtabs, iscan_all, qcoeff, dqcoeff, eob_out, dist_out, ra, s_tc, s_vc, recon_set);
            _Pragma("unroll") for (int r = 0; r < 4; r++) { s0[r] = s1[r]; p0[r] = p1[r]; }
            pc0 = pc1; pc1 = pc2; gj = g1; have0 = have1; have1 = have2;
        }
    };
    if (dc.pos) walk(std::true_type{}); else walk(std::false_type{});
}

/* persistent grid: a multiple of 8 workgroups (one walk per XCD, tq_walk_of), at most `per_2cu` per pair of compute units.
 * SVT_HIP_TQ_GRID=a,b,c,d (an experiment aid, read once): the largest grid of a 4x4 / 8x8 / 16x16 / 32x32 launch in workgroups, rounded up
 * to a multiple of 8; 0 or absent = the built-in cap.  It is how the caps below were swept, and how a small batch gets long walks. */
int tq_grid(svt_hip_ctx *ctx, int ngroups, int per_2cu, int size) {
    static const struct grid_env { int v[4]; } env = [] {
        grid_env g = {{0, 0, 0, 0}};
        if (const char *e = getenv("SVT_HIP_TQ_GRID")) sscanf(e, "%d,%d,%d,%d", &g.v[0], &g.v[1], &g.v[2], &g.v[3]);
        return g;
    }();
    const int per_xcd = (ngroups + 7) / 8, cap = env.v[size] > 0 ? (env.v[size] + 7) / 8 : (ctx->cu_count * per_2cu + 15) / 16;
    return 8 * (per_xcd < cap ? per_xcd : cap);
}

/* workgroups per two CUs of a mode-decision launch (svt_hip_tq_*batch*: six per CU; nothing is known about what runs beside it) */
constexpr int TQ_PER_2CU = 12;
/* ... and of an encode-pass launch (svt_tq_launch_device_lists) per size: one 4x4 workgroup on every other CU, two per CU of the others
 * (file comment, profiles/tq_prefetch.md) */
constexpr int TQ_PER_2CU_ENC[4] = {1, 4, 4, 4};

template <int N, bool RATE, bool DIST = true>
hipError_t launch_tq(svt_hip_ctx *ctx, const uint8_t *src, const uint8_t *pred, uint8_t *recon, const svt_tq_block *blocks, int n,
                     const svt_quant_tables *q, const int16_t *iscan, int16_t *qc, int16_t *dqc, uint16_t *eob, uint64_t *dist, tq_rate_args ra,
                     const uint8_t *const *recon_set, tq_dev_count dc = {nullptr, 0, nullptr, nullptr, 0, nullptr, 0}, int per_2cu = TQ_PER_2CU) {
    if (n <= 0) return hipSuccess;
    /* block per lane for 4x4 only: the 8x8 instance is bit-exact too but needs 201 VGPRs (64 samples + the transposed
     * intermediate live in one lane; 87 spills when held to 128) -- two waves per SIMD, and each displaces two ME waves:
     * the overlapped step went from 3.27 to 3.77 ms with it, so 8x8 stays on the N-lanes-per-block kernel */
    if constexpr (N == 4) {
        hipLaunchKernelGGL((svt_tq_lane_kernel<N, RATE, DIST>), dim3(tq_grid(ctx, (n + 255) / 256, per_2cu, 0)), dim3(256), 0, ctx->stream, src, pred, recon, blocks, n, q,
                           iscan, qc, dqc, eob, dist, ra, recon_set, dc);
        return hipGetLastError();
    } else {
        constexpr int BPW = TQ_THREADS / N;
        hipLaunchKernelGGL((svt_tq_kernel<N, RATE, DIST>), dim3(tq_grid(ctx, (n + BPW - 1) / BPW, per_2cu, txcfg<N>::size)), dim3(TQ_THREADS), 0, ctx->stream, src, pred, recon, blocks, n, q,
                           iscan, qc, dqc, eob, dist, ra, recon_set, dc);
        return hipGetLastError();
    }
}

template <bool RATE>
int32_t tq_launch_all(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *d_recon, const svt_tq_block *d_blocks,
                      const int32_t size_count[4], const svt_quant_tables *d_qtabs, const int16_t *d_iscan, int16_t *d_qcoeff,
                      int16_t *d_dqcoeff, uint16_t *d_eob, uint64_t *d_dist, tq_rate_args ra, uint8_t *const *recon_set = nullptr, int n_set = 0) {
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *const *d_set = nullptr;
    if (recon_set)
        if (const int32_t e = tq_stage_recon_set(ctx, recon_set, n_set, &d_set)) return e;
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    int        off = 0;
    hipError_t rc = hipSuccess;
    auto at = [&](int o) { tq_rate_args r = ra; if (r.bits) r.bits += o; return r; };
    rc = launch_tq<4, RATE>(ctx, d_src, d_pred, d_recon, d_blocks + off, size_count[0], d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob + off, d_dist ? d_dist + 2 * off : nullptr, at(off), d_set);
    off += size_count[0];
    if (rc == hipSuccess) rc = launch_tq<8, RATE>(ctx, d_src, d_pred, d_recon, d_blocks + off, size_count[1], d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob + off, d_dist ? d_dist + 2 * off : nullptr, at(off), d_set);
    off += size_count[1];
    if (rc == hipSuccess) rc = launch_tq<16, RATE>(ctx, d_src, d_pred, d_recon, d_blocks + off, size_count[2], d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob + off, d_dist ? d_dist + 2 * off : nullptr, at(off), d_set);
    off += size_count[2];
    if (rc == hipSuccess) rc = launch_tq<32, RATE>(ctx, d_src, d_pred, d_recon, d_blocks + off, size_count[3], d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob + off, d_dist ? d_dist + 2 * off : nullptr, at(off), d_set);
    HIP_TRY(rc);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}
} // namespace

/* several reconstruction buffers: their base pointers go to the device through the descriptor ring.  Internal to the library (declared in
 * svt_ctx.h; recon_kernel.hip stages its set with it too). */
int32_t tq_stage_recon_set(svt_hip_ctx *ctx, uint8_t *const *recon_set, int n_set, const uint8_t *const **d_set) {
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, 8 * sizeof(void *), &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "tq: descriptor buffers");
    for (int i = 0; i < 8; i++) ((uint8_t **)h)[i] = i < n_set ? recon_set[i] : nullptr; /* a block that names a set >= n_set is not reconstructed anywhere */
    HIP_TRY(svt_ctx_stage_send(ctx, 8 * sizeof(void *)));
    *d_set = (const uint8_t *const *)d;
    return SVT_HIP_OK;
}

/* Transform stage over block lists that were built ON THE DEVICE (csrc/encdec.hip): d_off_cnt[s] / d_off_cnt[4 + s] = first block and
 * number of blocks of size s inside d_blocks / d_eob; cap[s] = an upper bound known to the host, which only sizes the persistent
 * grids.  No rate, optional distortion.  d_pos != null: the lists are position codes (d_blocks is not read): tq_dev_count.  Internal to the
 * library (declared in svt_ctx.h). */
int32_t svt_tq_launch_device_lists(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *const *recon_set, int n_set,
                                   const svt_tq_block *d_blocks, const int32_t cap[4], const int32_t *d_off_cnt, const svt_quant_tables *d_qtabs,
                                   const int16_t *d_iscan, int16_t *d_qcoeff, int16_t *d_dqcoeff, uint16_t *d_eob, uint64_t *d_dist,
                                   const uint32_t *d_pos, const void *d_geom, int geom_stride, const uint32_t *d_iscan_off, int sb_cols) {
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *const *d_set = nullptr;
    if (const int32_t e = tq_stage_recon_set(ctx, recon_set, n_set, &d_set)) return e;
    const tq_rate_args none = {nullptr, nullptr, nullptr};
    hipError_t rc = hipSuccess;
#define TQ_DEV(N, S, D) launch_tq<N, false, D>(ctx, d_src, d_pred, nullptr, d_blocks, cap[S], d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob, d_dist, none, d_set, tq_dev_count{d_off_cnt, S, d_pos, (const uint8_t *)d_geom, geom_stride, d_iscan_off, sb_cols}, TQ_PER_2CU_ENC[S])
    if (d_dist) { /* with the coefficient-domain distortion pair */
        rc = TQ_DEV(4, 0, true);
        if (rc == hipSuccess) rc = TQ_DEV(8, 1, true);
        if (rc == hipSuccess) rc = TQ_DEV(16, 2, true);
        if (rc == hipSuccess) rc = TQ_DEV(32, 3, true);
    } else {      /* the encode pass: no distortion sums (instances without that arithmetic) */
        rc = TQ_DEV(4, 0, false);
        if (rc == hipSuccess) rc = TQ_DEV(8, 1, false);
        if (rc == hipSuccess) rc = TQ_DEV(16, 2, false);
        if (rc == hipSuccess) rc = TQ_DEV(32, 3, false);
    }
#undef TQ_DEV
    HIP_TRY(rc);
    return SVT_HIP_OK;
}

/* Blocks must be grouped by transform size: size_count[s] blocks of SVT_TX_<s>, in the order 4x4, 8x8, 16x16,
 * 32x32, and within a size all blocks must share the same do_recon flag (the encode pass reconstructs every
 * block; mode decision none) -- the kernel keeps its barriers workgroup-uniform that way. */
extern "C" int32_t svt_hip_tq_batch_device(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *d_recon,
                                           const svt_tq_block *d_blocks, const int32_t size_count[4],
                                           const svt_quant_tables *d_qtabs, const int16_t *d_iscan, int16_t *d_qcoeff,
                                           int16_t *d_dqcoeff, uint16_t *d_eob) {
    return svt_hip_tq_batch_dist_device(ctx, d_src, d_pred, d_recon, d_blocks, size_count, d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob,
                                        nullptr);
}

/* as svt_hip_tq_batch_device, plus d_dist[2*b], d_dist[2*b+1] = full_distortion_kernel32bit's result pair of block b
 * (residual distortion, prediction distortion); d_dist may be NULL */
extern "C" int32_t svt_hip_tq_batch_dist_device(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *d_recon,
                                                const svt_tq_block *d_blocks, const int32_t size_count[4],
                                                const svt_quant_tables *d_qtabs, const int16_t *d_iscan, int16_t *d_qcoeff,
                                                int16_t *d_dqcoeff, uint16_t *d_eob, uint64_t *d_dist) {
    if (!ctx || !d_src || !d_pred || !d_blocks || !size_count || !d_qtabs || !d_iscan || !d_qcoeff || !d_dqcoeff || !d_eob)
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq: null argument");
    if (((uintptr_t)d_qcoeff | (uintptr_t)d_dqcoeff) & 15) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq: coefficient arrays must be 16-byte aligned");
    tq_rate_args none = {nullptr, nullptr, nullptr};
    return tq_launch_all<false>(ctx, d_src, d_pred, d_recon, d_blocks, size_count, d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob, d_dist, none);
}

/* as svt_hip_tq_batch_dist_device, plus d_bits[b] = coeff_rate_estimate of block b computed behind the quantiser (no second
 * pass over the coefficients): the rate inputs of a block travel in svt_tq_block.pad_[0] (SVT_TQ_RATE_INFO) */
extern "C" int32_t svt_hip_tq_rd_batch_device(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *d_recon,
                                              const svt_tq_block *d_blocks, const int32_t size_count[4],
                                              const svt_quant_tables *d_qtabs, const int16_t *d_iscan, int16_t *d_qcoeff,
                                              int16_t *d_dqcoeff, uint16_t *d_eob, uint64_t *d_dist,
                                              const svt_rate_tables *d_tables, const int16_t *d_scan, int32_t *d_bits) {
    if (!ctx || !d_src || !d_pred || !d_blocks || !size_count || !d_qtabs || !d_iscan || !d_qcoeff || !d_dqcoeff || !d_eob || !d_tables ||
        !d_scan || !d_bits)
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq_rd: null argument");
    if (((uintptr_t)d_qcoeff | (uintptr_t)d_dqcoeff) & 15) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq_rd: coefficient arrays must be 16-byte aligned");
    if ((uintptr_t)d_scan & 3) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq_rd: scan array must be 4-byte aligned");
    tq_rate_args ra = {d_tables, d_scan, d_bits};
    return tq_launch_all<true>(ctx, d_src, d_pred, d_recon, d_blocks, size_count, d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob, d_dist, ra);
}

/* svt_hip_tq_rd_batch_device for a batch whose blocks reconstruct into up to 8 different buffers: block b writes into
 * recon_set[(pad_[0] >> 4) & 7] + recon_off.  One launch per transform size then serves pictures whose reference buffers lie further
 * apart than a 32-bit offset reaches, or in separate allocations -- e.g. the pictures of five consecutive mini-GOPs that one step of
 * a picture-level pipeline codes (bench.py's diagonal schedule). */
extern "C" int32_t svt_hip_tq_rd_batch_multi_device(svt_hip_ctx *ctx, const uint8_t *d_src, const uint8_t *d_pred, uint8_t *const *recon_set, int32_t n_set,
                                                    const svt_tq_block *d_blocks, const int32_t size_count[4], const svt_quant_tables *d_qtabs,
                                                    const int16_t *d_iscan, int16_t *d_qcoeff, int16_t *d_dqcoeff, uint16_t *d_eob, uint64_t *d_dist,
                                                    const svt_rate_tables *d_tables, const int16_t *d_scan, int32_t *d_bits) {
    if (!ctx || !d_src || !d_pred || !recon_set || n_set < 1 || n_set > 8 || !d_blocks || !size_count || !d_qtabs || !d_iscan || !d_qcoeff || !d_dqcoeff || !d_eob)
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq_multi: bad argument");
    if (((uintptr_t)d_qcoeff | (uintptr_t)d_dqcoeff) & 15) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq_multi: coefficient arrays must be 16-byte aligned");
    if (d_bits) {
        if (!d_tables || !d_scan || ((uintptr_t)d_scan & 3)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq_multi: rate tables / scan array");
        tq_rate_args ra = {d_tables, d_scan, d_bits};
        return tq_launch_all<true>(ctx, d_src, d_pred, nullptr, d_blocks, size_count, d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob, d_dist, ra, recon_set, n_set);
    }
    tq_rate_args none = {nullptr, nullptr, nullptr};
    return tq_launch_all<false>(ctx, d_src, d_pred, nullptr, d_blocks, size_count, d_qtabs, d_iscan, d_qcoeff, d_dqcoeff, d_eob, d_dist, none, recon_set, n_set);
}

/* the compiled-in 4x4 scan orders of the in-lane rate pass: out[0..15] = scan, out[16..47] = the neighbour pairs of positions 0..15 */
extern "C" int32_t svt_hip_rate_scan4x4_table(int32_t tx_type, int16_t out[48]) {
    if (tx_type < 0 || tx_type > 3 || !out) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "scan4x4: bad argument");
    const scan4_tab &t = SCAN4[scan4_kind(tx_type)];
    for (int i = 0; i < 16; i++) out[i] = t.scan[i];
    for (int i = 0; i < 32; i++) out[16 + i] = t.nb[i];
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_tq_batch(svt_hip_ctx *ctx, const uint8_t *src, const uint8_t *pred, uint8_t *recon, size_t plane_bytes,
                                    const svt_tq_block *blocks, int32_t n_blocks, const svt_quant_tables *qtabs, int32_t n_qtabs,
                                    const int16_t *iscan, size_t iscan_count, int16_t *qcoeff, int16_t *dqcoeff,
                                    size_t coeff_count, uint16_t *eob) {
    if (!ctx || !src || !pred || !recon || !blocks || n_blocks < 1 || !qtabs || !iscan || !qcoeff || !dqcoeff || !eob)
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq: null argument");
    int32_t cnt[4] = {0, 0, 0, 0};
    for (int i = 0; i < n_blocks; i++) {
        if (blocks[i].tx_size > 3 || blocks[i].qtab >= n_qtabs) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq: bad block");
        if (blocks[i].coeff_off & 7) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq: coeff_off must be a multiple of 8 coefficients");
        if (i && blocks[i].tx_size < blocks[i - 1].tx_size) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq: blocks not grouped by tx_size");
        if (i && blocks[i].tx_size == blocks[i - 1].tx_size && (blocks[i].do_recon != 0) != (blocks[i - 1].do_recon != 0))
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "tq: do_recon must be uniform within a tx_size group");
        cnt[blocks[i].tx_size]++;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    uint8_t *ds = (uint8_t *)svt_ctx_slot(ctx, SVT_SLOT_TQ_SRC, plane_bytes + 64), *dp = (uint8_t *)svt_ctx_slot(ctx, SVT_SLOT_TQ_PRED, plane_bytes + 64);
    uint8_t *dr = (uint8_t *)svt_ctx_slot(ctx, SVT_SLOT_TQ_RECON, plane_bytes + 64);
    svt_tq_block *db = (svt_tq_block *)svt_ctx_slot(ctx, SVT_SLOT_TQ_BLOCKS, sizeof(svt_tq_block) * (size_t)n_blocks);
    svt_quant_tables *dqt = (svt_quant_tables *)svt_ctx_slot(ctx, SVT_SLOT_TQ_QTABS, sizeof(svt_quant_tables) * (size_t)n_qtabs);
    int16_t *dis = (int16_t *)svt_ctx_slot(ctx, SVT_SLOT_TQ_ISCAN, sizeof(int16_t) * iscan_count);
    int16_t *dq = (int16_t *)svt_ctx_slot(ctx, SVT_SLOT_TQ_QCOEFF, sizeof(int16_t) * coeff_count), *ddq = (int16_t *)svt_ctx_slot(ctx, SVT_SLOT_TQ_DQCOEFF, sizeof(int16_t) * coeff_count);
    uint16_t *de = (uint16_t *)svt_ctx_slot(ctx, SVT_SLOT_TQ_EOB, sizeof(uint16_t) * (size_t)n_blocks);
    if (!ds || !dp || !dr || !db || !dqt || !dis || !dq || !ddq || !de) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "tq: device buffers");
    HIP_TRY(hipMemcpyAsync(ds, src, plane_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dp, pred, plane_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dr, recon, plane_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(db, blocks, sizeof(svt_tq_block) * (size_t)n_blocks, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dqt, qtabs, sizeof(svt_quant_tables) * (size_t)n_qtabs, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dis, iscan, sizeof(int16_t) * iscan_count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(dq, 0, sizeof(int16_t) * coeff_count, ctx->stream));
    HIP_TRY(hipMemsetAsync(ddq, 0, sizeof(int16_t) * coeff_count, ctx->stream));
    int32_t rc = svt_hip_tq_batch_device(ctx, ds, dp, dr, db, cnt, dqt, dis, dq, ddq, de);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(recon, dr, plane_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(qcoeff, dq, sizeof(int16_t) * coeff_count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dqcoeff, ddq, sizeof(int16_t) * coeff_count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(eob, de, sizeof(uint16_t) * (size_t)n_blocks, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SVT_HIP_OK;
}

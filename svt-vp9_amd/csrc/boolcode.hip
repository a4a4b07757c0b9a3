/*
 * boolcode.hip -- the VP9 bool coder over batches of streams (gfx950): token records and raw bools -> arithmetic-coded bytes.
 *
 * Replaces pack_mb_tokens over vpx_write between eb_vp9_start_encode and eb_vp9_stop_encode (Source/Lib/VPX/vp9_bitstream.c:98-162,
 * VPX/bitwriter.h:34-84, VPX/bitwriter.c).  The reference codes one tile per picture, so a picture is one chain of range updates;
 * here the chain is cut into chunks of BC_K bools and only the composition of the chunks' maps is serial (boolcode_core.h states the
 * arithmetic):
 *   segscan   one workgroup per stream: first item of every segment (an item = a token record or a raw bool), items of the stream
 *   count     one workgroup per 1024 items: bools of every item (a function of the token and of "node 0 left out"), their sum
 *   tilescan  one workgroup per stream: first bool of every 1024 items, bools of the stream n, M = n + 33 symbols, the framing bools
 *   expand    one workgroup per 1024 items: the bool records, 2 bytes a bool, into scratch
 *   maps      one wave per chunk, two start states per lane (the 128 ranges 128 .. 255): the chunk's bools are wave-uniform loads;
 *             result per start state: end state | shifts summed << 8
 *   chain     one workgroup per stream: the maps are staged through LDS BC_TILE chunks at a time and one lane walks a tile: every
 *             chunk's true start state and bit position, the total shift S, the bytes nb = (S - 16) / 8
 *   clear     zeroes the words of the accumulator the stream reaches
 *   code      one lane per chunk re-runs it from its true start state; split << position goes to 64-bit sums of 32-bit output
 *             words (a bit position can receive 127 contributions of up to 255): two running sums in registers, one integer atomic
 *             per touched word
 *   carry     one workgroup per stream, word tiles from the far end: high halves folded into the next word, then a
 *             generate / propagate scan; big-endian bytes, the marker byte, the size
 * Integer atomics only: the bytes do not depend on the order.  No lane walks the bools of a stream: the serial loops are over segment
 * tiles, item tiles (the two scans), chunks (chain) and word tiles (carry).
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"
#include "boolcode_core.h"
#include "wave_ops.h"

#define BC_K 256          /* bools per chunk */
#define BC_TILE 32        /* chunks per LDS tile of the chain kernel */
#define BC_ITEMS 1024     /* items per workgroup of count / expand: 256 lanes x 4 consecutive items */

extern "C" int32_t svt_boolcode_check_segments(uint32_t n_tokens, uint32_t n_bools, const svt_bool_segment *segments, uint32_t n_segments, uint64_t *items);

namespace {

enum { ST_ITEMS, ST_M, ST_CHUNKS, ST_S, ST_NB, ST_OVER, ST_WORDS = 16 };

struct bc_stream_dev {
    const uint32_t         *tokens;
    const uint16_t         *in_bools;
    const svt_bool_segment *segs;
    const uint32_t         *d_n_tokens;
    uint8_t                *bytes;
    uint32_t               *d_size;
    uint32_t               *state, *seg_pre, *tile_sum;
    uint16_t               *bools;
    uint32_t               *maps, *start;
    unsigned long long     *acc;
    uint32_t                n_segments, n_tokens, max_bools, capacity;
};
struct bc_batch_dev {
    bc_stream_dev s[SVT_BOOL_MAX_STREAMS];
};

/* exclusive prefix of v over the 256 lanes of the workgroup, *total = the sum; s_w: 4 entries of LDS, free again on return */
template <typename T> __device__ __forceinline__ T block_excl_scan(T v, T *s_w, T *total) {
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const T   ex = wave_excl_prefix(v, lane);
    if (lane == 63) s_w[wv] = ex + v;
    __syncthreads();
    T base = 0;
    for (int i = 0; i < wv; i++) base += s_w[i];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return base + ex;
}

__global__ __launch_bounds__(256) void svt_bc_segscan_kernel(const bc_batch_dev *__restrict__ B) {
    __shared__ unsigned long long s_w[4];
    __shared__ uint32_t           s_bad;
    const bc_stream_dev &P = B->s[blockIdx.x];
    const uint32_t       tid = threadIdx.x;
    unsigned long long   run = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    if (!P.segs) run = P.d_n_tokens ? *P.d_n_tokens : P.n_tokens;
    else {
        for (uint32_t base = 0; base < P.n_segments; base += 256) {
            const uint32_t     s = base + tid;
            unsigned long long tot;
            /* a segment of an unknown kind, or one whose buffer the stream does not have: the stream is not coded */
            if (s < P.n_segments && P.segs[s].count && (P.segs[s].kind > 1 || (P.segs[s].kind ? !P.in_bools : !P.tokens))) s_bad = 1;
            const unsigned long long ex = block_excl_scan<unsigned long long>(s < P.n_segments ? P.segs[s].count : 0u, s_w, &tot);
            if (s < P.n_segments) P.seg_pre[s] = run + ex > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(run + ex);
            run += tot;
        }
        if (tid == 0) P.seg_pre[P.n_segments] = run > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)run;
    }
    __syncthreads();
    if (tid == 0) { /* every item is at least one bool */
        const bool over = run > P.max_bools || s_bad;
        P.state[ST_ITEMS] = over ? 0u : (uint32_t)run;
        P.state[ST_OVER] = over;
    }
}

/* the four consecutive items i0 .. i0 + 3 of a lane: record (a token's or a raw bool's), bools, node 0 left out */
struct bc_items {
    uint32_t rec[4];
    int      cnt[4], skip[4], raw[4];
};
__device__ __forceinline__ void load_items(const bc_stream_dev &P, uint32_t n_items, uint32_t i0, bc_items &it) {
    uint32_t seg = 0, k = i0, first = 0, count = n_items, kind = 0;
    if (P.segs && i0 < n_items) {
        uint32_t lo = 0, hi = P.n_segments; /* the last segment that starts at or in front of i0: seg_pre[n_segments] = n_items > i0 */
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (P.seg_pre[mid] <= i0) lo = mid; else hi = mid;
        }
        seg = lo; k = i0 - P.seg_pre[lo];
        first = P.segs[seg].first; count = P.segs[seg].count; kind = P.segs[seg].kind;
    }
    _Pragma("unroll") for (int j = 0; j < 4; j++) {
        it.rec[j] = 0; it.cnt[j] = 0; it.skip[j] = 0; it.raw[j] = 0;
        if (i0 + j >= n_items) continue;
        while (k >= count) { /* (ends: the item exists, so a later segment holds it) */
            k -= count; seg++;
            first = P.segs[seg].first; count = P.segs[seg].count; kind = P.segs[seg].kind;
        }
        if (kind) { it.rec[j] = P.in_bools[first + k]; it.cnt[j] = 1; it.raw[j] = 1; }
        else {
            const uint32_t rec = P.tokens[first + k];
            it.rec[j] = rec;
            it.skip[j] = svt_bool_skip0(rec, k > 0, k > 0 ? P.tokens[first + k - 1] : 0u);
            it.cnt[j] = svt_bool_count((int)SVT_TOK_TOKEN(rec), it.skip[j]);
        }
        k++;
    }
}

__global__ __launch_bounds__(256) void svt_bc_count_kernel(const bc_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_w[4];
    const bc_stream_dev &P = B->s[blockIdx.y];
    const uint32_t       n_items = P.state[ST_ITEMS];
    if (blockIdx.x * BC_ITEMS >= n_items) return;
    bc_items it;
    load_items(P, n_items, blockIdx.x * BC_ITEMS + threadIdx.x * 4, it);
    uint32_t total;
    (void)block_excl_scan<uint32_t>((uint32_t)(it.cnt[0] + it.cnt[1] + it.cnt[2] + it.cnt[3]), s_w, &total);
    if (threadIdx.x == 0) P.tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void svt_bc_tilescan_kernel(const bc_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_w[4];
    const bc_stream_dev &P = B->s[blockIdx.x];
    const uint32_t       tid = threadIdx.x, n_tiles = (P.state[ST_ITEMS] + BC_ITEMS - 1) / BC_ITEMS;
    unsigned long long   run = 0;
    for (uint32_t base = 0; base < n_tiles; base += 256) {
        const uint32_t t = base + tid, v = t < n_tiles ? P.tile_sum[t] : 0u;
        uint32_t       tot;
        const uint32_t ex = block_excl_scan<uint32_t>(v, s_w, &tot);
        if (t < n_tiles) P.tile_sum[t] = (uint32_t)(run + ex);
        run += tot;
    }
    const bool     over = P.state[ST_OVER] || run > P.max_bools;
    const uint32_t n = (uint32_t)run, M = over ? 0u : n + 1 + SVT_BOOL_FRAME_TAIL;
    if (!over) { /* what eb_vp9_start_encode and eb_vp9_stop_encode add */
        if (tid == 0) P.bools[0] = SVT_BOOL_RECORD(0, 128);
        if (tid < SVT_BOOL_FRAME_TAIL) P.bools[1 + n + tid] = SVT_BOOL_RECORD(0, 128);
    }
    if (tid == 0) {
        P.state[ST_M] = M;
        P.state[ST_CHUNKS] = (M + BC_K - 1) / BC_K;
        P.state[ST_OVER] = over;
    }
}

/* The expand kernel's text, instantiated twice on "coefficient probabilities per stream".  The table's only reader.  A macro and not a
 * template: through a templated device function the plain instance compiles to the code it always was but for three commuted adds, and
 * svt_hip_boolcode_batch_device is to run the code object it ran before the second instance existed, instruction for instruction. */
#define BC_EXPAND_BODY(EXPAND)                                                                                                                          \
    __shared__ uint32_t s_w[4];                                                                                                                         \
    const bc_stream_dev &P = B->s[blockIdx.y];                                                                                                          \
    const uint32_t       n_items = P.state[ST_ITEMS];                                                                                                   \
    if (P.state[ST_OVER] || blockIdx.x * BC_ITEMS >= n_items) return;                                                                                   \
    bc_items it;                                                                                                                                        \
    load_items(P, n_items, blockIdx.x * BC_ITEMS + threadIdx.x * 4, it);                                                                                \
    uint32_t total;                                                                                                                                     \
    uint32_t off = 1 + P.tile_sum[blockIdx.x] + block_excl_scan<uint32_t>((uint32_t)(it.cnt[0] + it.cnt[1] + it.cnt[2] + it.cnt[3]), s_w, &total);      \
    _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                                                     \
        if (!it.cnt[j]) continue;                                                                                                                       \
        if (it.raw[j]) P.bools[off] = (uint16_t)it.rec[j];                                                                                              \
        else (void)EXPAND;                                                                                                                              \
        off += (uint32_t)it.cnt[j];                                                                                                                     \
    }
__global__ __launch_bounds__(256) void svt_bc_expand_kernel(const bc_batch_dev *__restrict__ B, const svt_bool_tables *__restrict__ tables) {
    BC_EXPAND_BODY(svt_bool_expand(it.rec[j], it.skip[j], tables, P.bools + off))
}
/* coef[stream] when it is set, the context's coefficient probabilities otherwise */
__global__ __launch_bounds__(256) void svt_bc_expand_tables_kernel(const bc_batch_dev *__restrict__ B, const svt_bool_tables *__restrict__ tables,
                                                                    const uint8_t *const *__restrict__ coef) {
    BC_EXPAND_BODY(svt_bool_expand_probs(it.rec[j], it.skip[j], coef[blockIdx.y] ? coef[blockIdx.y] : tables->coef_probs, tables, P.bools + off))
}
#undef BC_EXPAND_BODY

/* the j-th (0 .. 7) bool record of a 16-byte group */
__device__ __forceinline__ uint32_t bool_of(const uint4 &q, int j) {
    const uint32_t w = (j >> 1) == 0 ? q.x : (j >> 1) == 1 ? q.y : (j >> 1) == 2 ? q.z : q.w;
    return (w >> (16 * (j & 1))) & 0xffffu;
}

__global__ __launch_bounds__(256) void svt_bc_maps_kernel(const bc_batch_dev *__restrict__ B) {
    const bc_stream_dev &P = B->s[blockIdx.y];
    const uint32_t       lane = threadIdx.x & 63, c = blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t       M = (uint32_t)__builtin_amdgcn_readfirstlane((int)P.state[ST_M]); /* (wave-uniform: the loop's bounds stay scalar) */
    if (c >= (uint32_t)__builtin_amdgcn_readfirstlane((int)P.state[ST_CHUNKS])) return;
    const uint32_t cnt = M - c * BC_K < BC_K ? M - c * BC_K : BC_K;
    const uint4   *src = (const uint4 *)(P.bools + (size_t)c * BC_K);
    uint32_t       r0 = 128 + lane, r1 = 192 + lane, s0 = 0, s1 = 0, split;
    for (uint32_t g = 0; g * 8 < cnt; g++) {
        const uint4 q = src[g];
        _Pragma("unroll") for (int j = 0; j < 8; j++) {
            if (g * 8 + j >= cnt) break;
            const uint32_t rec = bool_of(q, j);
            const uint32_t n0 = svt_bool_step(r0, rec, &split), n1 = svt_bool_step(r1, rec, &split);
            r0 = n0 & 255u; s0 += n0 >> 8;
            r1 = n1 & 255u; s1 += n1 >> 8;
        }
    }
    P.maps[(size_t)c * 128 + lane] = r0 | s0 << 8;
    P.maps[(size_t)c * 128 + 64 + lane] = r1 | s1 << 8;
}

__global__ __launch_bounds__(256) void svt_bc_chain_kernel(const bc_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_map[BC_TILE * 128];
    __shared__ uint32_t s_start[BC_TILE * 2];
    const bc_stream_dev &P = B->s[blockIdx.x];
    const uint32_t       tid = threadIdx.x, n_chunks = P.state[ST_CHUNKS];
    uint32_t             r = 255, S = 0; /* lane 0's */
    for (uint32_t t0 = 0; t0 < n_chunks; t0 += BC_TILE) {
        const uint32_t n = n_chunks - t0 < BC_TILE ? n_chunks - t0 : BC_TILE;
        for (uint32_t i = tid; i < n * 128; i += 256) s_map[i] = P.maps[(size_t)t0 * 128 + i];
        __syncthreads();
        if (tid == 0)
            for (uint32_t c = 0; c < n; c++) {
                s_start[2 * c] = r; s_start[2 * c + 1] = S;
                const uint32_t m = s_map[c * 128 + r - 128];
                r = m & 255u; S += m >> 8;
            }
        __syncthreads();
        if (tid < 2 * n) P.start[(size_t)t0 * 2 + tid] = s_start[tid];
        __syncthreads();
    }
    if (tid == 0) {
        P.state[ST_S] = S;
        P.state[ST_NB] = n_chunks ? (S - 16) / 8 : 0u;
        P.state[ST_WORDS] = n_chunks ? (S + 8 + 31) / 32 + 1 : 0u; /* words the carry kernel reads; one more is cleared */
    }
}

__global__ __launch_bounds__(256) void svt_bc_clear_kernel(const bc_batch_dev *__restrict__ B) {
    const bc_stream_dev &P = B->s[blockIdx.y];
    const uint32_t       n = P.state[ST_WORDS] + 1;
    for (uint32_t i = blockIdx.x * 1024 + threadIdx.x; i < n && i < (blockIdx.x + 1) * 1024; i += 256) P.acc[i] = 0;
}

__global__ __launch_bounds__(64) void svt_bc_code_kernel(const bc_batch_dev *__restrict__ B) {
    const bc_stream_dev &P = B->s[blockIdx.y];
    const uint32_t       c = blockIdx.x * 64 + threadIdx.x, M = P.state[ST_M];
    if (c >= P.state[ST_CHUNKS]) return;
    const uint32_t cnt = M - c * BC_K < BC_K ? M - c * BC_K : BC_K;
    const uint4   *src = (const uint4 *)(P.bools + (size_t)c * BC_K);
    uint32_t       r = P.start[2 * (size_t)c], pos = P.start[2 * (size_t)c + 1], wcur = pos >> 5;
    unsigned long long a0 = 0, a1 = 0; /* sums of words wcur, wcur + 1 */
    for (uint32_t g = 0; g * 8 < cnt; g++) {
        const uint4 q = src[g];
        _Pragma("unroll") for (int j = 0; j < 8; j++) {
            if (g * 8 + j >= cnt) break;
            const uint32_t rec = bool_of(q, j);
            uint32_t       split;
            const uint32_t next = svt_bool_step(r, rec, &split);
            if (rec & 0x100u) {
                const uint32_t w = pos >> 5;
                if (w != wcur) {
                    if (a0) atomicAdd(&P.acc[wcur], a0);
                    if (w == wcur + 1) a0 = a1;
                    else { if (a1) atomicAdd(&P.acc[wcur + 1], a1); a0 = 0; }
                    a1 = 0; wcur = w;
                }
                const unsigned long long t = (unsigned long long)split << (56 - (pos & 31u)); /* split's 8 bits at [pos, pos + 8) of the 64 bits of two words */
                a0 += t >> 32; a1 += t & 0xFFFFFFFFull;
            }
            r = next & 255u; pos += next >> 8;
        }
    }
    if (a0) atomicAdd(&P.acc[wcur], a0);
    if (a1) atomicAdd(&P.acc[wcur + 1], a1);
}

__global__ __launch_bounds__(256) void svt_bc_carry_kernel(const bc_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_gp[256];
    const bc_stream_dev &P = B->s[blockIdx.x];
    const uint32_t       tid = threadIdx.x;
    if (P.state[ST_OVER]) {
        if (tid == 0) *P.d_size = SVT_BOOL_SIZE_OVERFLOW;
        return;
    }
    const uint32_t W = P.state[ST_WORDS], nb = P.state[ST_NB], cap = P.capacity;
    uint32_t       cin = 0;
    for (uint32_t tile = (W + 255) / 256; tile-- > 0;) {
        const uint32_t k = tile * 256 + 255 - tid; /* lane 0 holds the word furthest from the front: carries travel with the lane index */
        uint32_t       l = 0, g = 0, p = 0;
        if (k < W) {
            const unsigned long long v = (P.acc[k] & 0xFFFFFFFFull) + (P.acc[k + 1] >> 32); /* (word k + 1 is cleared even when k + 1 == W) */
            l = (uint32_t)v; g = (uint32_t)(v >> 32); p = l == 0xFFFFFFFFu;
        }
        s_gp[tid] = g | p << 1;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            const uint32_t o = tid >= d ? s_gp[tid - d] : 2u, m = s_gp[tid];
            __syncthreads();
            s_gp[tid] = ((m | ((m >> 1) & o)) & 1u) | (m & o & 2u);
            __syncthreads();
        }
        const uint32_t before = tid ? s_gp[tid - 1] : 2u, last = s_gp[255];
        const uint32_t c_in = (before | ((before >> 1) & cin)) & 1u;
        cin = (last | ((last >> 1) & cin)) & 1u;
        if (k < W) {
            const uint32_t f = l + c_in;
            _Pragma("unroll") for (uint32_t b = 0; b < 4; b++)
                if (4 * k + b < nb && 4 * k + b < cap) P.bytes[4 * k + b] = (uint8_t)(f >> (24 - 8 * b));
            if (nb && (nb - 1) >> 2 == k) { /* no ambiguity with a superframe index: eb_vp9_stop_encode's trailing byte */
                const uint32_t extra = ((f >> (24 - 8 * ((nb - 1) & 3u))) & 0xe0u) == 0xc0u;
                if (extra && nb < cap) P.bytes[nb] = 0;
                *P.d_size = nb + extra;
            }
        }
        __syncthreads();
    }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

} // namespace

extern "C" void svt_hip_boolcode_geometry(int32_t *bools_per_chunk, int32_t *chunks_per_tile) {
    if (bools_per_chunk) *bools_per_chunk = BC_K;
    if (chunks_per_tile) *chunks_per_tile = BC_TILE;
}

extern "C" int32_t svt_hip_boolcode_set_tables(svt_hip_ctx *ctx, const svt_bool_tables *tables) {
    return svt_ctx_set_tables(ctx, SVT_SLOT_BC_TABLES, tables, sizeof(svt_bool_tables), "boolcode");
}

/* both batch entries: d_coef_probs null = the context's table for every stream (the plain expand kernel, the descriptor alone is staged) */
static int32_t bc_batch(svt_hip_ctx *ctx, int32_t n_streams, const svt_bool_stream *streams, const uint8_t *const *d_coef_probs) {
    if (!ctx || !streams || n_streams < 1 || n_streams > SVT_BOOL_MAX_STREAMS) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "boolcode: bad argument");
    size_t   total = 0;
    uint32_t max_tiles = 1, max_chunks = 1, max_words = 1;
    for (int i = 0; i < n_streams; i++) {
        const svt_bool_stream &s = streams[i];
        if (!s.d_size || (!s.d_bytes && s.capacity) || (!s.d_segments && s.n_segments) || (!s.d_segments && !s.d_tokens && (s.n_tokens || s.d_n_tokens)))
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "boolcode: null stream field");
        if (7ull * ((unsigned long long)s.max_bools + 1 + SVT_BOOL_FRAME_TAIL) >= 0x100000000ull)
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "boolcode: stream too long for 32-bit bit positions");
        const uint32_t tiles = (s.max_bools + BC_ITEMS - 1) / BC_ITEMS, chunks = (s.max_bools + 1 + SVT_BOOL_FRAME_TAIL + BC_K - 1) / BC_K;
        const uint32_t words = (uint32_t)((7ull * (s.max_bools + 1 + SVT_BOOL_FRAME_TAIL) + 8 + 31) / 32) + 4;
        total += align16(sizeof(uint32_t) * 32) + align16(sizeof(uint32_t) * ((size_t)s.n_segments + 1)) + align16(sizeof(uint32_t) * ((size_t)tiles + 1)) +
                 align16(sizeof(uint16_t) * (size_t)chunks * BC_K) + align16(sizeof(uint32_t) * (size_t)chunks * 128) + align16(sizeof(uint32_t) * (size_t)chunks * 2) +
                 align16(sizeof(unsigned long long) * (size_t)words);
        max_tiles = tiles > max_tiles ? tiles : max_tiles;
        max_chunks = chunks > max_chunks ? chunks : max_chunks;
        max_words = words > max_words ? words : max_words;
    }
    if (!ctx->slot_bytes[SVT_SLOT_BC_TABLES]) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "boolcode: svt_hip_boolcode_set_tables has not been called");
    HIP_TRY(hipSetDevice(ctx->device));
    uint8_t *scratch = (uint8_t *)svt_ctx_slot(ctx, SVT_SLOT_BC_SCRATCH, total);
    if (!scratch) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "boolcode: scratch");
    bc_batch_dev hb;
    memset(&hb, 0, sizeof hb);
    for (int i = 0; i < n_streams; i++) {
        const svt_bool_stream &s = streams[i];
        bc_stream_dev         &P = hb.s[i];
        const uint32_t tiles = (s.max_bools + BC_ITEMS - 1) / BC_ITEMS, chunks = (s.max_bools + 1 + SVT_BOOL_FRAME_TAIL + BC_K - 1) / BC_K;
        const uint32_t words = (uint32_t)((7ull * (s.max_bools + 1 + SVT_BOOL_FRAME_TAIL) + 8 + 31) / 32) + 4;
        P.tokens = s.d_tokens; P.in_bools = s.d_bools; P.segs = s.d_segments; P.d_n_tokens = s.d_n_tokens; P.bytes = s.d_bytes; P.d_size = s.d_size;
        P.n_segments = s.n_segments; P.n_tokens = s.n_tokens; P.max_bools = s.max_bools; P.capacity = s.capacity;
        P.state = (uint32_t *)scratch; scratch += align16(sizeof(uint32_t) * 32);
        P.seg_pre = (uint32_t *)scratch; scratch += align16(sizeof(uint32_t) * ((size_t)s.n_segments + 1));
        P.tile_sum = (uint32_t *)scratch; scratch += align16(sizeof(uint32_t) * ((size_t)tiles + 1));
        P.bools = (uint16_t *)scratch; scratch += align16(sizeof(uint16_t) * (size_t)chunks * BC_K);
        P.maps = (uint32_t *)scratch; scratch += align16(sizeof(uint32_t) * (size_t)chunks * 128);
        P.start = (uint32_t *)scratch; scratch += align16(sizeof(uint32_t) * (size_t)chunks * 2);
        P.acc = (unsigned long long *)scratch; scratch += align16(sizeof(unsigned long long) * (size_t)words);
    }
    void        *h = nullptr, *d = nullptr;
    const size_t staged = sizeof hb + (d_coef_probs ? sizeof(const uint8_t *) * SVT_BOOL_MAX_STREAMS : 0);
    if (svt_ctx_stage(ctx, staged, &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "boolcode: descriptor buffers");
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    memcpy(h, &hb, sizeof hb);
    if (d_coef_probs) {
        const uint8_t **hc = (const uint8_t **)((uint8_t *)h + sizeof hb);
        for (int i = 0; i < SVT_BOOL_MAX_STREAMS; i++) hc[i] = i < n_streams ? d_coef_probs[i] : nullptr;
    }
    HIP_TRY(svt_ctx_stage_send(ctx, staged));
    const bc_batch_dev    *dB = (const bc_batch_dev *)d;
    const svt_bool_tables *dT = (const svt_bool_tables *)ctx->slot[SVT_SLOT_BC_TABLES];
    const dim3             ns((unsigned)n_streams);
    hipLaunchKernelGGL(svt_bc_segscan_kernel, ns, dim3(256), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_bc_count_kernel, dim3(max_tiles, n_streams), dim3(256), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_bc_tilescan_kernel, ns, dim3(256), 0, ctx->stream, dB);
    if (d_coef_probs)
        hipLaunchKernelGGL(svt_bc_expand_tables_kernel, dim3(max_tiles, n_streams), dim3(256), 0, ctx->stream, dB, dT, (const uint8_t *const *)((const uint8_t *)d + sizeof hb));
    else hipLaunchKernelGGL(svt_bc_expand_kernel, dim3(max_tiles, n_streams), dim3(256), 0, ctx->stream, dB, dT);
    hipLaunchKernelGGL(svt_bc_maps_kernel, dim3((max_chunks + 3) / 4, n_streams), dim3(256), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_bc_chain_kernel, ns, dim3(256), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_bc_clear_kernel, dim3((max_words + 1023) / 1024, n_streams), dim3(256), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_bc_code_kernel, dim3((max_chunks + 63) / 64, n_streams), dim3(64), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_bc_carry_kernel, ns, dim3(256), 0, ctx->stream, dB);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_boolcode_batch_device(svt_hip_ctx *ctx, int32_t n_streams, const svt_bool_stream *streams) {
    return bc_batch(ctx, n_streams, streams, nullptr);
}
extern "C" int32_t svt_hip_boolcode_batch_tables_device(svt_hip_ctx *ctx, int32_t n_streams, const svt_bool_stream *streams, const uint8_t *const *d_coef_probs) {
    return bc_batch(ctx, n_streams, streams, d_coef_probs);
}

extern "C" int32_t svt_hip_boolcode(svt_hip_ctx *ctx, const uint32_t *tokens, uint32_t n_tokens, const uint16_t *bools, uint32_t n_bools,
                                    const svt_bool_segment *segments, uint32_t n_segments, uint8_t *bytes, uint32_t capacity, uint32_t *size) {
    if (!ctx || !size || (!bytes && capacity) || (!tokens && n_tokens) || (!bools && n_bools) || (!segments && n_segments))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "boolcode: null argument");
    uint64_t items = n_tokens, max_bools = (uint64_t)n_tokens * SVT_BOOL_MAX_PER_TOKEN;
    if (segments) {
        if (svt_boolcode_check_segments(n_tokens, n_bools, segments, n_segments, &items)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "boolcode: segment outside its buffer");
        max_bools = 0;
        for (uint32_t s = 0; s < n_segments; s++) max_bools += (uint64_t)segments[s].count * (segments[s].kind ? 1 : SVT_BOOL_MAX_PER_TOKEN);
    }
    if (7 * (max_bools + 1 + SVT_BOOL_FRAME_TAIL) >= 0x100000000ull) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "boolcode: stream too long for 32-bit bit positions");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t tb = align16(sizeof(uint32_t) * (size_t)n_tokens), bb = align16(sizeof(uint16_t) * (size_t)n_bools), sb = align16(sizeof(svt_bool_segment) * (size_t)n_segments);
    uint8_t     *din = (uint8_t *)svt_ctx_slot(ctx, SVT_SLOT_BC_IN, tb + bb + sb + 16);
    uint8_t     *dout = (uint8_t *)svt_ctx_slot(ctx, SVT_SLOT_BC_OUT, 16 + (size_t)capacity);
    if (!din || !dout) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "boolcode: device buffers");
    if (n_tokens) HIP_TRY(hipMemcpyAsync(din, tokens, sizeof(uint32_t) * (size_t)n_tokens, hipMemcpyHostToDevice, ctx->stream));
    if (n_bools) HIP_TRY(hipMemcpyAsync(din + tb, bools, sizeof(uint16_t) * (size_t)n_bools, hipMemcpyHostToDevice, ctx->stream));
    if (n_segments) HIP_TRY(hipMemcpyAsync(din + tb + bb, segments, sizeof(svt_bool_segment) * (size_t)n_segments, hipMemcpyHostToDevice, ctx->stream));
    svt_bool_stream s;
    memset(&s, 0, sizeof s);
    s.d_tokens = (const uint32_t *)din; s.d_bools = (const uint16_t *)(din + tb); s.d_segments = segments ? (const svt_bool_segment *)(din + tb + bb) : nullptr;
    s.n_segments = segments ? n_segments : 0; s.n_tokens = n_tokens; s.max_bools = (uint32_t)max_bools; s.capacity = capacity;
    s.d_bytes = dout + 16; s.d_size = (uint32_t *)dout;
    const int32_t rc = svt_hip_boolcode_batch_device(ctx, 1, &s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(size, dout, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t got = *size < capacity ? *size : capacity;
    if (got) {
        HIP_TRY(hipMemcpyAsync(bytes, dout + 16, got, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return SVT_HIP_OK;
}

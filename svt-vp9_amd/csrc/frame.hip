/*
 * frame.hip -- frame-packet assembly over a batch of pictures (gfx950): header || tile || trailer of every picture, densely, into one
 * arena, with an offset / size table beside it.
 *
 * Replaces the EB_MEMCPY of the entropy coder's tile bytes behind the two headers in eb_vp9_pack_bitstream
 * (Source/Lib/VPX/vp9_bitstream.c:1397-1411) and the append of the show-existing bytes (Codec/EbPacketizationProcess.c:374-453); the
 * headers themselves are host work (host/frame_host.c).  The tile's size is known only on the device and its slot is sized for a worst
 * case hundreds of times larger, so the gather runs on the device behind the bool coder:
 *   assemble   FR_WGS workgroups per picture (grid.y = picture).  Every workgroup reads the at most 32 tile sizes itself and sums the
 *              packet sizes in front of its picture (csrc/frame_core.h): no scan launch, no host value.  Workgroup 0 of a picture
 *              writes the table entry, the header, the trailer and the up to 15 bytes in front of and behind the 16-byte-aligned
 *              part of the destination as byte stores; all workgroups share that aligned part in a grid-stride loop over 16-byte
 *              vectors: two aligned 16-byte loads of the source (one when source and destination agree mod 16), a byte shift
 *              (__builtin_amdgcn_alignbyte over the eight dwords), one aligned 16-byte store.
 * Bounds: a load touches only 16-byte blocks that hold a source byte -- vector v reads the source bytes [s + 16 v, s + 16 v + 16), all
 * inside the tile, from the blocks that hold the first and the last of them; a store touches only [offset, offset + size) of its
 * picture, cut at arena_capacity (svt_frame_span), so neighbouring packets never interfere and nothing lies at or beyond the capacity.
 *   parts      the same for packets whose compressed header is a device stream too (a header with coefficient-probability updates):
 *              uncompressed header || compressed header || tile || trailer.  The shifted copy runs twice per picture, and the 16 bits of
 *              first_part_size -- the compressed header's size, a device value at an arbitrary bit position of the host's header bytes
 *              -- are filled in by the lanes that store those bytes.  No read-modify-write of the arena, no atomics.
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"
#include "frame_core.h"

#ifndef FR_WGS            /* (the CPU emulation of the tests builds with fewer) */
#define FR_WGS 16         /* workgroups per picture: with 256 lanes x 16 bytes, 64 KiB a pass of the grid-stride loop */
#endif
#define FR_LANES 256

extern "C" int32_t svt_frame_check_packets(int32_t n_pics, const svt_frame_packet *pk);
extern "C" int32_t svt_frame_check_parts(int32_t n_pics, const svt_frame_parts_packet *pk);

namespace {

struct fr_batch_dev {
    svt_frame_packet pk[SVT_FRAME_MAX_PICS];
    uint8_t         *arena;
    svt_frame_entry *table;
    uint32_t         arena_capacity;
    int32_t          n_pics;
};
struct fr_parts_dev {
    svt_frame_parts_packet pk[SVT_FRAME_MAX_PICS];
    uint8_t               *arena;
    svt_frame_entry       *table;
    uint32_t               arena_capacity;
    int32_t                n_pics;
};

/* dword j (0 .. 3) of the 16 bytes that start `sh` bytes (DS = sh >> 2 dwords, b = sh & 3 bytes) into the 32 bytes lo || hi */
template <int DS> __device__ __forceinline__ uint4 shift_bytes(const uint4 &lo, const uint4 &hi, uint32_t b) {
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint4          r;
    r.x = __builtin_amdgcn_alignbyte(w[DS + 1], w[DS + 0], b);
    r.y = __builtin_amdgcn_alignbyte(w[DS + 2], w[DS + 1], b);
    r.z = __builtin_amdgcn_alignbyte(w[DS + 3], w[DS + 2], b);
    r.w = __builtin_amdgcn_alignbyte(w[DS + 4], w[DS + 3], b);
    return r;
}

/* n_vec aligned 16-byte vectors at dst from the bytes at src, of any alignment, shared by the lanes of the picture's FR_WGS workgroups in a
 * grid-stride loop: two aligned loads (one when src is aligned too), a byte shift, one aligned store */
__device__ __forceinline__ void fr_copy_vectors(uint4 *const dst, const uint8_t *const src, const uint32_t n_vec) {
    if (!n_vec) return;
    const uint32_t  tid = threadIdx.x;
    const uintptr_t s0 = (uintptr_t)src;                                                  /* vector v = the source bytes s0 + 16 v .. + 15 */
    const uint4    *blk = (const uint4 *)(s0 & ~(uintptr_t)15);                           /* the block that holds the first of them */
    const uint32_t  sh = (uint32_t)__builtin_amdgcn_readfirstlane((int)(s0 & 15u)), b = sh & 3u;
    const uint32_t  stride = FR_WGS * FR_LANES;
    uint32_t        v = blockIdx.x * FR_LANES + tid;
    if (sh == 0) {
        for (; v < n_vec; v += stride) dst[v] = blk[v];
        return;
    }
    /* sh > 0: the bytes of vector v end sh bytes into block v + 1, which therefore holds source bytes too */
    switch (sh >> 2) {
    case 0: for (; v < n_vec; v += stride) dst[v] = shift_bytes<0>(blk[v], blk[v + 1], b); break;
    case 1: for (; v < n_vec; v += stride) dst[v] = shift_bytes<1>(blk[v], blk[v + 1], b); break;
    case 2: for (; v < n_vec; v += stride) dst[v] = shift_bytes<2>(blk[v], blk[v + 1], b); break;
    default: for (; v < n_vec; v += stride) dst[v] = shift_bytes<3>(blk[v], blk[v + 1], b); break;
    }
}

__global__ __launch_bounds__(FR_LANES) void svt_fr_assemble_kernel(const fr_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_size[SVT_FRAME_MAX_PICS];
    const uint32_t      tid = threadIdx.x;
    const int           pic = (int)blockIdx.y, n_pics = B->n_pics;
    if ((int)tid < n_pics) {
        const svt_frame_packet &q = B->pk[tid];
        s_size[tid] = svt_frame_packet_size(q.header_len, q.trailer_len, *q.d_tile_size, q.tile_capacity);
    }
    __syncthreads();
    const svt_frame_packet &P = B->pk[pic];
    const uint32_t          cap = B->arena_capacity, size = s_size[pic];
    uint32_t                none;
    const uint32_t          off = svt_frame_layout(s_size, pic, &none);
    uint8_t *const          arena = B->arena;
    if (blockIdx.x == 0 && tid == 0) {
        B->table[pic].offset = off;
        B->table[pic].size = size;
        if (pic == 0) {
            const uint32_t total = svt_frame_layout(s_size, n_pics, &none);
            B->table[n_pics].offset = total;
            B->table[n_pics].size = none;
        }
    }
    if (size == SVT_FRAME_SIZE_NONE) return;
    const uint32_t hl = P.header_len, tl = P.trailer_len, tile = size - hl - tl;
    const uint64_t at = (uint64_t)off + hl;                /* arena position of the tile's first byte */
    const uint32_t n = svt_frame_span(at, tile, cap);      /* tile bytes below the capacity */
    const uint8_t *src = P.d_tile;
    /* the destination's part in front of its first 16-byte boundary, its aligned vectors, the rest */
    const uint32_t mis = (uint32_t)(-(uintptr_t)(arena + at)) & 15u, head = mis < n ? mis : n;
    const uint32_t n_vec = (n - head) >> 4, tail = (n - head) & 15u;
    if (blockIdx.x == 0) { /* byte stores: lanes 0 .. 63 the header, 64 .. 79 the head, 80 .. 95 the tail, 96 .. 99 the trailer */
        if (tid < svt_frame_span(off, hl, cap)) arena[(uint64_t)off + tid] = P.header[tid];
        const uint32_t k = tid & 15u;
        if ((tid >> 4) == 4 && k < head) arena[at + k] = src[k];
        if ((tid >> 4) == 5 && k < tail) arena[at + head + 16ull * n_vec + k] = src[head + 16ull * n_vec + k];
        if ((tid >> 4) == 6 && k < svt_frame_span(at + tile, tl, cap)) arena[at + tile + k] = P.trailer[k];
    }
    fr_copy_vectors((uint4 *)(arena + at + head), src + head, n_vec);
}

/* One device part of a three-part packet: the n bytes (already cut at the capacity) at src, of any alignment, to arena + at.  Workgroup 0
 * stores the up to 15 bytes in front of and behind the 16-byte-aligned part of the destination as byte stores, lanes 16 g .. 16 g + 15 the
 * front and the 16 lanes behind them the rest; every workgroup takes its share of the aligned vectors */
__device__ __forceinline__ void fr_copy_part(uint8_t *const arena, const uint64_t at, const uint32_t n, const uint8_t *const src, const uint32_t g) {
    const uint32_t tid = threadIdx.x;
    const uint32_t mis = (uint32_t)(-(uintptr_t)(arena + at)) & 15u, head = mis < n ? mis : n;
    const uint32_t n_vec = (n - head) >> 4, tail = (n - head) & 15u;
    if (blockIdx.x == 0) {
        const uint32_t k = tid & 15u;
        if ((tid >> 4) == g && k < head) arena[at + k] = src[k];
        if ((tid >> 4) == g + 1 && k < tail) arena[at + head + 16ull * n_vec + k] = src[head + 16ull * n_vec + k];
    }
    fr_copy_vectors((uint4 *)(arena + at + head), src + head, n_vec);
}

/* uncompressed header || compressed header || tile || trailer (svt_frame_parts_packet): the kernel above with two device parts, the
 * copy run once for each, and first_part_size filled into the header bytes in the registers of the lanes that store them
 * (svt_frame_size_field_byte): the arena is never read.  Bounds as above, for each part */
__global__ __launch_bounds__(FR_LANES) void svt_fr_parts_kernel(const fr_parts_dev *__restrict__ B) {
    __shared__ uint32_t s_size[SVT_FRAME_MAX_PICS], s_comp[SVT_FRAME_MAX_PICS];
    const uint32_t      tid = threadIdx.x;
    const int           pic = (int)blockIdx.y, n_pics = B->n_pics;
    if ((int)tid < n_pics) {
        const svt_frame_parts_packet &q = B->pk[tid];
        const uint32_t                c = *q.d_compressed_size;
        s_comp[tid] = c;
        s_size[tid] = svt_frame_parts_size(q.header_len, q.trailer_len, c, q.compressed_capacity, *q.d_tile_size, q.tile_capacity);
    }
    __syncthreads();
    const svt_frame_parts_packet &P = B->pk[pic];
    const uint32_t                cap = B->arena_capacity, size = s_size[pic];
    uint32_t                      none;
    const uint32_t                off = svt_frame_layout(s_size, pic, &none);
    uint8_t *const                arena = B->arena;
    if (blockIdx.x == 0 && tid == 0) {
        B->table[pic].offset = off;
        B->table[pic].size = size;
        if (pic == 0) {
            const uint32_t total = svt_frame_layout(s_size, n_pics, &none);
            B->table[n_pics].offset = total;
            B->table[n_pics].size = none;
        }
    }
    if (size == SVT_FRAME_SIZE_NONE) return;
    const uint32_t hl = P.header_len, tl = P.trailer_len, comp = s_comp[pic], tile = size - hl - tl - comp;
    const uint64_t at_c = (uint64_t)off + hl, at_t = at_c + comp;     /* arena positions of the two device parts */
    if (blockIdx.x == 0) { /* byte stores: lanes 0 .. 31 the header, 32 .. 63 the compressed part's ends, 64 .. 95 the tile's, 96 .. 99 the trailer */
        if (tid < svt_frame_span(off, hl, cap)) arena[(uint64_t)off + tid] = svt_frame_size_field_byte(P.header[tid], tid, P.size_bit, comp);
        const uint32_t k = tid & 15u;
        if ((tid >> 4) == 6 && k < svt_frame_span(at_t + tile, tl, cap)) arena[at_t + tile + k] = P.trailer[k];
    }
    fr_copy_part(arena, at_c, svt_frame_span(at_c, comp, cap), P.d_compressed, 2);
    fr_copy_part(arena, at_t, svt_frame_span(at_t, tile, cap), P.d_tile, 4);
}

} // namespace

extern "C" void svt_hip_frame_geometry(int32_t *workgroups_per_picture, int32_t *bytes_per_pass) {
    if (workgroups_per_picture) *workgroups_per_picture = FR_WGS;
    if (bytes_per_pass) *bytes_per_pass = FR_WGS * FR_LANES * 16;
}

extern "C" int32_t svt_hip_frame_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_frame_packet *packets, uint8_t *d_arena, uint32_t arena_capacity,
                                              svt_frame_entry *d_table) {
    if (!ctx || !d_table || (!d_arena && arena_capacity) || svt_frame_check_packets(n_pics, packets))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "frame: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof(fr_batch_dev), &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "frame: descriptor buffers");
    fr_batch_dev *hb = (fr_batch_dev *)h;
    memset(hb, 0, sizeof *hb);
    memcpy(hb->pk, packets, sizeof(svt_frame_packet) * (size_t)n_pics);
    hb->arena = d_arena; hb->table = d_table; hb->arena_capacity = arena_capacity; hb->n_pics = n_pics;
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof(fr_batch_dev)));
    hipLaunchKernelGGL(svt_fr_assemble_kernel, dim3(FR_WGS, (unsigned)n_pics), dim3(FR_LANES), 0, ctx->stream, (const fr_batch_dev *)d);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_frame_parts_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_frame_parts_packet *packets, uint8_t *d_arena,
                                                    uint32_t arena_capacity, svt_frame_entry *d_table) {
    if (!ctx || !d_table || (!d_arena && arena_capacity) || svt_frame_check_parts(n_pics, packets))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "frame: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof(fr_parts_dev), &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "frame: descriptor buffers");
    fr_parts_dev *hb = (fr_parts_dev *)h;
    memset(hb, 0, sizeof *hb);
    memcpy(hb->pk, packets, sizeof(svt_frame_parts_packet) * (size_t)n_pics);
    hb->arena = d_arena; hb->table = d_table; hb->arena_capacity = arena_capacity; hb->n_pics = n_pics;
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof(fr_parts_dev)));
    hipLaunchKernelGGL(svt_fr_parts_kernel, dim3(FR_WGS, (unsigned)n_pics), dim3(FR_LANES), 0, ctx->stream, (const fr_parts_dev *)d);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}

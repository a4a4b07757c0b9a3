/*
 * frame_parts_emu.cpp -- the three-part assembly of csrc/frame.hip (svt_fr_parts_kernel and its entry point, included below) on the CPU
 * through the stand-in runtime of tests/emu/hip/hip_runtime.h: the batches tests/frame_parts_model.py makes (argv[1]) through
 * svt_hip_frame_parts_batch_device, compared byte for byte -- arena, guards, table -- with svt_hip_frame_assemble_parts_host.  Every
 * compressed header and every tile lives in an allocation of its own that is exactly the 16-byte blocks holding its bytes, so a build with
 * -fsanitize=address reports a load from a block that holds no source byte; the arena's guards show a store outside it, the size words and
 * the table are exactly their entries.
 *
 * file: int32 n_batches; per batch int32 n_pics, uint32 arena_capacity, int32 source_bytes, the source; per picture int32 comp_off,
 *       uint32 comp, comp_cap, int32 tile_off, uint32 tile, tile_cap, int32 header_len, size_bit, trailer_len, 27 header bytes, 4 trailer bytes
 */
#include "frame.hip"
#include "emu_harness.h"

#define GUARD 64
static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

/* the bytes [off, off + size) of the source in an allocation of exactly the 16-byte blocks that hold them, at the same address mod 16 */
static uint8_t *exact(std::vector<void *> &blocks, const std::vector<uint8_t> &source, int32_t off, uint32_t live) {
    const uint32_t mis = (uint32_t)off & 15u;
    uint8_t       *blk = (uint8_t *)aligned_alloc(16, ((size_t)mis + live + 15) / 16 * 16 + (live ? 0 : 16));
    blocks.push_back(blk);
    if (live) memcpy(blk + mis, source.data() + off, live);
    return blk + mis;
}

int main(int argc, char **argv) {
    static svt_hip_ctx ctx;
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    int32_t n_batches = 0;
    if (!f || !rd(f, &n_batches, 4)) return 2;
    int bad = 0;
    for (int b = 0; b < n_batches; b++) {
        int32_t n_pics, source_bytes; uint32_t cap;
        if (!rd(f, &n_pics, 4) || !rd(f, &cap, 4) || !rd(f, &source_bytes, 4) || n_pics < 1 || n_pics > SVT_FRAME_MAX_PICS) return 3;
        std::vector<uint8_t> source((size_t)source_bytes);
        if (!rd(f, source.data(), source.size())) return 3;
        svt_frame_parts_packet pk[SVT_FRAME_MAX_PICS];
        uint32_t sizes[2 * SVT_FRAME_MAX_PICS];
        std::vector<void *> blocks;
        memset(pk, 0, sizeof pk);
        for (int i = 0; i < n_pics; i++) {
            int32_t v[9];
            if (!rd(f, v, sizeof v) || !rd(f, pk[i].header, sizeof pk[i].header) || !rd(f, pk[i].trailer, sizeof pk[i].trailer)) return 3;
            const uint32_t comp = (uint32_t)v[1], comp_cap = (uint32_t)v[2], tile = (uint32_t)v[4], tile_cap = (uint32_t)v[5];
            const bool     ships = svt_frame_parts_size(0, 0, comp, comp_cap, tile, tile_cap) != SVT_FRAME_SIZE_NONE;
            pk[i].d_compressed = exact(blocks, source, v[0], ships ? comp : 0);
            pk[i].d_tile = exact(blocks, source, v[3], ships ? tile : 0);
            sizes[2 * i] = comp; sizes[2 * i + 1] = tile;
            pk[i].d_compressed_size = &sizes[2 * i]; pk[i].d_tile_size = &sizes[2 * i + 1];
            pk[i].compressed_capacity = comp_cap; pk[i].tile_capacity = tile_cap;
            pk[i].header_len = (uint8_t)v[6]; pk[i].size_bit = (uint16_t)v[7]; pk[i].trailer_len = (uint8_t)v[8];
        }
        const size_t room = GUARD + (size_t)cap + GUARD;
        uint8_t *a1 = (uint8_t *)aligned_alloc(16, (room + 15) / 16 * 16), *a2 = (uint8_t *)aligned_alloc(16, (room + 15) / 16 * 16);
        memset(a1, 0xA5, room); memset(a2, 0xA5, room);
        svt_frame_entry t1[SVT_FRAME_MAX_PICS + 1 + 4], t2[SVT_FRAME_MAX_PICS + 1 + 4];
        memset(t1, 0x5A, sizeof t1); memset(t2, 0x5A, sizeof t2);
        const int r1 = svt_hip_frame_parts_batch_device(&ctx, n_pics, pk, a1 + GUARD, cap, t1);
        const int r2 = svt_hip_frame_assemble_parts_host(n_pics, pk, a2 + GUARD, cap, t2);
        const bool ok = !r1 && !r2 && !memcmp(t1, t2, sizeof t1) && !memcmp(a1, a2, room);
        printf("batch %d pics %d capacity %u total %u none %u %s\n", b, n_pics, cap, t2[n_pics].offset, t2[n_pics].size, ok ? "ok" : "MISMATCH");
        bad += !ok;
        for (void *p : blocks) free(p);
        free(a1); free(a2);
    }
    fclose(f);
    printf("bad %d\n", bad);
    return bad;
}

/*
 * frame_emu.cpp -- csrc/frame.hip itself (kernel and entry point, included below) on the CPU through the stand-in runtime of
 * tests/emu/hip/hip_runtime.h: the packet batches tests/frame_model.py makes (argv[1], written by tests/test_frame.py) through
 * svt_hip_frame_batch_device, compared byte for byte -- arena, guards, table -- with svt_hip_frame_assemble_host.  Every tile lives in an
 * allocation of its own that is exactly the 16-byte blocks holding its bytes (its start at the batch's offset mod 16), so a build with
 * -fsanitize=address reports a load from a block that holds no source byte; the arena's guards show a store outside it.
 *
 * file: int32 n_batches; per batch int32 n_pics, uint32 arena_capacity, int32 source_bytes, the source; per picture int32 src_off,
 *       uint32 size, uint32 capacity, int32 header_len, trailer_len, 56 header bytes, 4 trailer bytes
 */
#include "frame.hip"
#include "emu_harness.h"

#define GUARD 64
static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

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
        svt_frame_packet pk[SVT_FRAME_MAX_PICS];
        uint32_t sizes[SVT_FRAME_MAX_PICS];
        std::vector<void *> blocks;
        memset(pk, 0, sizeof pk);
        for (int i = 0; i < n_pics; i++) {
            int32_t src_off, hl, tl; uint32_t size, capacity;
            if (!rd(f, &src_off, 4) || !rd(f, &size, 4) || !rd(f, &capacity, 4) || !rd(f, &hl, 4) || !rd(f, &tl, 4) || !rd(f, pk[i].header, sizeof pk[i].header) || !rd(f, pk[i].trailer, sizeof pk[i].trailer)) return 3;
            const uint32_t live = size == SVT_BOOL_SIZE_OVERFLOW || size > capacity ? 0 : size, mis = (uint32_t)src_off & 15u;
            uint8_t *blk = (uint8_t *)aligned_alloc(16, ((size_t)mis + live + 15) / 16 * 16 + (live ? 0 : 16));
            blocks.push_back(blk);
            if (live) memcpy(blk + mis, source.data() + src_off, live);
            sizes[i] = size;
            pk[i].d_tile = blk + mis; pk[i].d_tile_size = &sizes[i]; pk[i].tile_capacity = capacity;
            pk[i].header_len = (uint8_t)hl; pk[i].trailer_len = (uint8_t)tl;
        }
        uint8_t *a1 = (uint8_t *)aligned_alloc(16, GUARD + ((size_t)cap + 15) / 16 * 16 + GUARD), *a2 = (uint8_t *)aligned_alloc(16, GUARD + ((size_t)cap + 15) / 16 * 16 + GUARD);
        memset(a1, 0xA5, GUARD + (size_t)cap + GUARD); memset(a2, 0xA5, GUARD + (size_t)cap + GUARD);
        svt_frame_entry t1[SVT_FRAME_MAX_PICS + 1 + 4], t2[SVT_FRAME_MAX_PICS + 1 + 4];
        memset(t1, 0x5A, sizeof t1); memset(t2, 0x5A, sizeof t2);
        const int r1 = svt_hip_frame_batch_device(&ctx, n_pics, pk, a1 + GUARD, cap, t1);
        const int r2 = svt_hip_frame_assemble_host(n_pics, pk, a2 + GUARD, cap, t2);
        const uint32_t total = t2[n_pics].offset;
        /* beyond the total the contents are the fill of both; when the total exceeds the capacity the arena's contents are unspecified, but
           the two forms cut every run of bytes at the capacity the same way */
        const bool ok = !r1 && !r2 && !memcmp(t1, t2, sizeof t1) && !memcmp(a1, a2, GUARD + (size_t)cap + GUARD);
        printf("batch %d pics %d capacity %u total %u none %u %s\n", b, n_pics, cap, total, t2[n_pics].size, ok ? "ok" : "MISMATCH");
        bad += !ok;
        for (void *p : blocks) free(p);
        free(a1); free(a2);
    }
    fclose(f);
    printf("bad %d\n", bad);
    return bad;
}

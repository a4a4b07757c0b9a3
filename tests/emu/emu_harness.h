/*
 * emu_harness.h -- what every *_emu.cpp defines behind hip/hip_runtime.h and svt_ctx.h: the lane's indices, the barriers, the launch
 * (a thread per lane, the workgroups of the grid one after another) and the context's helpers.  Include it after the .hip under test.
 */
#pragma once
#include <stdio.h>
thread_local dim3 threadIdx, blockIdx, blockDim;
pthread_barrier_t *g_bar, *g_wave_bar;
unsigned long long g_shfl[1024];
void emu_launch(dim3 grid, dim3 block, std::function<void()> body) {
    pthread_barrier_t bar, wave[16];
    const unsigned n_waves = (block.x + 63) / 64;
    pthread_barrier_init(&bar, nullptr, block.x);
    for (unsigned w = 0; w < n_waves; w++) pthread_barrier_init(&wave[w], nullptr, block.x - 64 * w < 64 ? block.x - 64 * w : 64);
    g_bar = &bar; g_wave_bar = wave;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; t++) th.emplace_back([=] {
        blockDim = block; threadIdx = dim3(t);
        for (unsigned by = 0; by < grid.y; by++) for (unsigned bx = 0; bx < grid.x; bx++) { blockIdx = dim3(bx, by); body(); pthread_barrier_wait(g_bar); }
    });
    for (auto &t : th) t.join();
    pthread_barrier_destroy(&bar);
    for (unsigned w = 0; w < n_waves; w++) pthread_barrier_destroy(&wave[w]);
}
int32_t svt_set_error(int32_t c, const char *m) { fprintf(stderr, "error %d %s\n", c, m); return c; }
int32_t svt_set_hip_error(hipError_t e, const char *f, int l) { return -1; }
static char stage_h[65536], stage_d[65536];
int svt_ctx_stage(svt_hip_ctx *, size_t n, void **h, void **d) { *h = stage_h; *d = stage_d; return n > sizeof stage_h; }
void svt_ctx_stage_commit(svt_hip_ctx *) {}
void *svt_ctx_slot(svt_hip_ctx *c, int s, size_t bytes) {
    if (bytes > c->slot_bytes[s]) { free(c->slot[s]); hipMalloc(&c->slot[s], bytes); c->slot_bytes[s] = bytes; }
    return c->slot[s];
}

/*
 * A stand-in for <hip/hip_runtime.h> that lets the entropy-side stages (csrc/boolcode.hip, modeinfo.hip, modeinfo_inter.hip, mvrefs.hip,
 * frame.hip) compile as plain C++ and run on the CPU: one thread per lane of a workgroup, a pthread barrier for __syncthreads, wave
 * shuffles through a shared array behind a barrier of the wave's own 64 threads (the waves of a workgroup take their shuffles
 * independently of each other), __shared__ as a static (one workgroup runs at a time), device memory = host memory.  Only what those
 * files and svt_ctx.h use is here; emu_harness.h holds the definitions.
 */
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <vector>
#include <thread>
#include <functional>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { uint4 q = {x, y, z, w}; return q; }
extern thread_local dim3 threadIdx, blockIdx, blockDim;
extern pthread_barrier_t *g_bar, *g_wave_bar;
extern unsigned long long g_shfl[1024];
inline void __syncthreads() { pthread_barrier_wait(g_bar); }
inline void emu_wave_sync() { pthread_barrier_wait(&g_wave_bar[threadIdx.x >> 6]); }
template <typename T> inline T __shfl_up(T v, int d, int w) {
    g_shfl[threadIdx.x] = (unsigned long long)v;
    emu_wave_sync();
    T r = ((int)(threadIdx.x & 63) >= d) ? (T)g_shfl[threadIdx.x - d] : v;
    emu_wave_sync();
    return r;
}
template <typename T> inline T __shfl_xor(T v, int d, int w) {
    g_shfl[threadIdx.x] = (unsigned long long)v;
    emu_wave_sync();
    T r = (T)g_shfl[(threadIdx.x & ~63u) | ((threadIdx.x & 63u) ^ (unsigned)d)];
    emu_wave_sync();
    return r;
}
inline int __builtin_amdgcn_readfirstlane(int v) { return v; }
/* v_alignbyte_b32: the low 32 bits of (hi:lo) >> 8 * (bytes & 3) */
inline uint32_t __builtin_amdgcn_alignbyte(uint32_t hi, uint32_t lo, uint32_t bytes) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (bytes & 3u))); }
inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
typedef int hipError_t; typedef void *hipStream_t; typedef void *hipEvent_t;
enum { hipSuccess = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
inline hipError_t hipSetDevice(int) { return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return 0; }
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
inline hipError_t hipMalloc(void **p, size_t n) { *p = malloc(n + 64); memset(*p, 0xCD, n + 64); return 0; }
inline hipError_t hipFree(void *p) { free(p); return 0; }
void emu_launch(dim3 grid, dim3 block, std::function<void()> body);
#define hipLaunchKernelGGL(kernel, grid, block, shm, stream, ...) emu_launch(grid, block, [=] { kernel(__VA_ARGS__); })

/*
 * A stand-in for <hip/hip_runtime.h> that lets csrc/frame.hip compile as plain C++ and run on the CPU (tests/test_frame.py): one thread
 * per lane of a workgroup, a pthread barrier for __syncthreads, __shared__ as a static (one workgroup runs at a time), device memory =
 * host memory.  Only what frame.hip and svt_ctx.h use is here.
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
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { uint32_t x, y, z, w; };
extern thread_local dim3 threadIdx, blockIdx, blockDim;
extern pthread_barrier_t *g_bar;
inline void __syncthreads() { pthread_barrier_wait(g_bar); }
inline int __builtin_amdgcn_readfirstlane(int v) { return v; }
/* v_alignbyte_b32: the low 32 bits of (hi:lo) >> 8 * (bytes & 3) */
inline uint32_t __builtin_amdgcn_alignbyte(uint32_t hi, uint32_t lo, uint32_t bytes) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (bytes & 3u))); }
typedef int hipError_t; typedef void *hipStream_t; typedef void *hipEvent_t;
enum { hipSuccess = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
inline hipError_t hipSetDevice(int) { return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return 0; }
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
void emu_launch(dim3 grid, dim3 block, std::function<void()> body);
#define hipLaunchKernelGGL(kernel, grid, block, shm, stream, ...) emu_launch(grid, block, [=] { kernel(__VA_ARGS__); })

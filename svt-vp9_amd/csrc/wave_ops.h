/* wave_ops.h -- sums and prefixes over the 64 lanes of a wave, by shuffles: every lane of the wave takes the call.  Both are templates, so
 * a file that uses one of them needs only that one's shuffle of its runtime (the CPU stand-ins of tests/emu need not hold both). */
#ifndef SVT_WAVE_OPS_H
#define SVT_WAVE_OPS_H
#include <hip/hip_runtime.h>

/* the sum of v over the wave, in every lane */
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
    _Pragma("unroll") for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
/* the sum of v over the lanes below `lane` (= the caller's lane in its wave) */
template <typename T> __device__ __forceinline__ T wave_excl_prefix(T v, int lane) {
    T incl = v;
    _Pragma("unroll") for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    return incl - v;
}
#endif

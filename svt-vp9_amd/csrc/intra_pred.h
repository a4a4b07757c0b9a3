/*
 * intra_pred.h -- the ten VP9 intra predictors as device code, shared by the intra encode pass (intra_kernel.hip) and the open-loop
 * intra search (intra_search.hip): one row of an N x N prediction from the block's reference samples, and the transform type that
 * follows the luma mode.
 */
#ifndef SVT_INTRA_PRED_H
#define SVT_INTRA_PRED_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

/* eb_vp9_intra_mode_to_tx_type_lookup (VPX/vp9_reconintra.c:20-31): DC, V, H, D45, D135, D117, D153, D207, D63, TM */
__device__ __forceinline__ int intra_tx_type(int mode) { return (int)((0x3122130210ull >> (4 * mode)) & 3); }

#define AVG2(a, b) (((a) + (b) + 1) >> 1)
#define AVG3(a, b, c) (((a) + 2 * (b) + (c) + 2) >> 2)

/* Row r of the N x N prediction, packed.  e[k + 32] = B(k): B(0) the corner sample above[-1], B(k > 0) = above[k - 1] (2N samples:
 * the second N replicate above[N - 1], or are the true above-right samples), B(-k) = left[k - 1].  Closed forms of the procedures of
 * VPX/intrapred.c (d207 :22, d63 :43, d45 :59, d117 :75, d135 :99, d153 :120, v / h / tm :140-172, the four DC forms :174-236,
 * the 4x4 forms of d45 / d63 :349-416 which read the above-right samples). */
template <int N> __device__ __forceinline__ void intra_pred_row(const uint8_t *e, int mode, int r, int have_left, int have_top, uint32_t (&prow)[N / 4]) {
    auto B = [&](int k) -> int { return (int)e[k + 32]; };
    int dc = 128;
    if (mode == 0 && (have_left || have_top)) {
        int sum = 0, cnt = 0;
        if (have_top) { _Pragma("unroll") for (int j = 0; j < N; j++) sum += B(j + 1); cnt += N; }
        if (have_left) { _Pragma("unroll") for (int j = 0; j < N; j++) sum += B(-(j + 1)); cnt += N; }
        dc = (sum + (cnt >> 1)) / cnt;
    }
    _Pragma("unroll") for (int q = 0; q < N / 4; q++) prow[q] = 0;
    /* the mode is uniform over the wave: one branch, then N samples without control flow */
    auto fill = [&](auto f) {
        _Pragma("unroll") for (int c = 0; c < N; c++) prow[c >> 2] |= (uint32_t)(f(c) & 0xff) << (8 * (c & 3));
    };
    switch (mode) {
    case 0: fill([&](int) { return dc; }); break;
    case 1: fill([&](int c) { return B(c + 1); }); break;
    case 2: fill([&](int) { return B(-(r + 1)); }); break;
    case 3: /* D45 */
        fill([&](int c) {
            if (N == 4) return (r + c == 6) ? B(8) : AVG3(B(r + c + 1), B(r + c + 2), B(r + c + 3));
            return (r + c < N - 1) ? AVG3(B(r + c + 1), B(r + c + 2), B(r + c + 3)) : B(N);
        });
        break;
    case 4: fill([&](int c) { const int p = c - r; return AVG3(B(p - 1), B(p), B(p + 1)); }); break; /* D135 */
    case 5: /* D117 */
        fill([&](int c) {
            const int h = r >> 1;
            if (c >= h) { const int cc = c - h; return (r & 1) ? AVG3(B(cc - 1), B(cc), B(cc + 1)) : AVG2(B(cc), B(cc + 1)); }
            const int rr = r - 2 * c;
            return AVG3(B(-(rr - 2)), B(-(rr - 1)), B(-rr));
        });
        break;
    case 6: /* D153 */
        fill([&](int c) {
            const int h = c >> 1;
            if (r >= h) { const int rr = r - h; return (c & 1) ? AVG3(B(-rr + 1), B(-rr), B(-rr - 1)) : AVG2(B(-rr), B(-rr - 1)); }
            const int cc = c - 2 * r;
            return AVG3(B(cc - 2), B(cc - 1), B(cc));
        });
        break;
    case 7: /* D207: left[] clamped at N - 1 */
        fill([&](int c) {
            const int idx = r + (c >> 1);
            const int l0 = B(-(min(idx, N - 1) + 1)), l1 = B(-(min(idx + 1, N - 1) + 1)), l2 = B(-(min(idx + 2, N - 1) + 1));
            return (c & 1) ? AVG3(l0, l1, l2) : AVG2(l0, l1);
        });
        break;
    case 8: /* D63 */
        fill([&](int c) {
            const int h = r >> 1;
            if (N > 4 && r >= 2 && c >= N - 1 - h) return B(N);
            return (r & 1) ? AVG3(B(c + h + 1), B(c + h + 2), B(c + h + 3)) : AVG2(B(c + h + 1), B(c + h + 2));
        });
        break;
    default: /* TM */
        fill([&](int c) { const int v = B(-(r + 1)) + B(c + 1) - B(0); return v < 0 ? 0 : v > 255 ? 255 : v; });
        break;
    }
}

} // namespace

#endif /* SVT_INTRA_PRED_H */

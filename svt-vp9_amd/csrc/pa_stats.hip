/*
 * pa_stats.hip -- the per-picture statistics of the reference's picture-analysis process on gfx950: noise detection
 * (sb_flat_noise_array, pic_noise_class), the intensity histograms with their region / picture averages, and the chroma
 * block means.  Replaces picture_pre_processing_operations (Source/Lib/Codec/EbPictureAnalysisProcess.c:4191-4232 ->
 * detect_input_picture_noise :3512-3619, quarter_sample_detect_noise :3809-3928, sub_sample_detect_noise :3930-4055),
 * the two *_generate_pixel_intensity_histogram_bins + calculate_input_average_intensity of gathering_picture_statistics
 * (:4237-4432, :4839-4886) and compute_chroma_block_mean (:1828-2109).  Every kernel takes a batch of pictures.
 *
 * All three are plane passes that read their input once.  The weak-filtered and the noise samples of the noise kernel
 * live in registers; only flags, sums and (for tests) the two optional planes reach memory.
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"

#define PS_GLOBAL __attribute__((address_space(1)))
#define PS_AS_GLOBAL(T, p) ((T PS_GLOBAL *)(uintptr_t)(p))

namespace {
typedef uint32_t ps_u32x4 __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t ps_u32x2 __attribute__((ext_vector_type(2), aligned(1)));

/* ------------------------------------------------------------------------------------------------------------------ */
/* noise detection                                                                                                      */
/* ------------------------------------------------------------------------------------------------------------------ */
struct ps_noise_job {
    const uint8_t *src;   /* sample (0,0) of the analysed plane (full, 1/4 or 1/16 luma) */
    uint8_t       *flags; /* sb_flat_noise_array, pw * ph bytes */
    uint8_t       *den, *noise; /* optional w x h planes (stride w), or NULL */
    int32_t        stride, w, h;
    int32_t        tiles_x, tiles_y; /* 64x64 tiles launched for this picture: they cover every SB flag once */
    int32_t        vis_x, vis_y;     /* tiles the reference's loop visits */
    int32_t        pw, ph;           /* picture size in SBs */
    int32_t        tile0;            /* first workgroup of this job */
    uint32_t       sb_count;         /* tot_sb_count: the SBs the loop visits (known from the geometry) */
};

constexpr int PS_LDS_ROW = 18; /* dwords per staged row: sample x of the tile is byte 4 + x, the halo bytes 3 and 68 */

__device__ __forceinline__ uint32_t ps_byte(const uint32_t *w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }
__device__ __forceinline__ int      ps_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

/* the eleven-step ladder of detect_input_picture_noise (:3586-3615), the four-step one of sub_sample_detect_noise (:4033-4052)
 * and quarter_sample_detect_noise's (:3906-3925); PIC_NOISE_CLASS_1, 2, 3, 3_1, 4 .. 10 = 1, 2, 3, 4, 5 .. 11 */
__device__ uint32_t ps_noise_class(int method, uint64_t v, int luma_height) {
    if (method == 0) {
        const uint32_t th = luma_height <= 720 ? 25 : 0;
        uint32_t       c;
        if (v >= 80 + th) c = 11;
        else if (v >= 70 + th) c = 10;
        else if (v >= 60 + th) c = 9;
        else if (v >= 50 + th) c = 8;
        else if (v >= 40 + th) c = 7;
        else if (v >= 30 + th) c = 6;
        else if (v >= 20 + th) c = 5;
        else if (v >= 17 + th) c = 4;
        else if (v >= 10 + th) c = 3;
        else if (v >= 5 + th) c = 2;
        else c = 1;
        return c >= 5 ? 4 : c;
    }
    if (method == 1) {
        const uint32_t th = luma_height <= 720 ? 25 : luma_height <= 1080 ? 10 : 0;
        return v >= 55 + th ? 4 : v >= 10 + th ? 3 : v >= 5 + th ? 2 : 1;
    }
    return v > 60 ? 4 : v >= 10 ? 3 : v >= 5 ? 2 : 1;
}

/* One workgroup per 64x64 tile of the analysed plane; thread t filters 16 samples of row t >> 2.
 * M = 0: full precision, the tile is an SB and its 64x64 variance comes from 8x8 sums over rows 0, 2, 4, 6
 *        (compute_variance64x64 -> eb_vp9_compute_interm_var_four8x8_avx2_intrin / the SSE2 sub-sampled pair);
 * M = 1: half precision, 16 SBs per tile, 16x16 variances from full 8x8 means (compute_variance16x16);
 * M = 2: quarter precision, 4 SBs per tile, 32x32 variances (compute_variance32x32, with its pairing of 8x8 rows 0 + 2, 1 + 3).
 * In M = 1, 2 the noise variance of every SB row of the tile is taken from the tile's top SB row: the reference's noise picture
 * is one 64-row strip and noise_origin_index has no row term. */
/* part[tile]: the tile's sum of (noiseBlkVar >> 16), added up per picture by svt_pa_noise_class_kernel: one plain store per tile
 * (thousands of atomics on one address per picture cost more than the filter). */
template <int M>
__global__ __launch_bounds__(256) void svt_pa_noise_kernel(const ps_noise_job *__restrict__ jobs, int n_jobs, uint32_t noise_blk_th,
                                                           uint32_t *__restrict__ part) {
    __shared__ uint32_t s_w[66 * PS_LDS_ROW];
    __shared__ uint32_t s_blk[4][8][8]; /* den sum, den sum of squares, noise sum, noise sum of squares per 8x8 block */
    __shared__ uint64_t s_m16[2][16], s_q16[2][16];
    int j = 0;
    while (j + 1 < n_jobs && (int)blockIdx.x >= jobs[j + 1].tile0) j++;
    const ps_noise_job J = jobs[j];
    const int t = threadIdx.x, tile = (int)blockIdx.x - J.tile0, ty = tile / J.tiles_x, tx = tile - ty * J.tiles_x;
    const int x0 = tx * 64, y0 = ty * 64, W = J.w, H = J.h;
    constexpr int SBS = M == 0 ? 1 : M == 1 ? 4 : 2; /* SBs per tile side */
    const bool in_loop = tx < J.vis_x && ty < J.vis_y;
    const bool complete = x0 + 64 <= W && y0 + 64 <= H;
    const bool stats = in_loop && complete; /* M = 0: is_complete_sb; M = 1, 2: the loop visits whole tiles only */
    const bool planes = J.den != nullptr && in_loop;
    if (!stats) { /* these SBs keep the 0 the reference resets every flag to */
        if (t < SBS * SBS) {
            const int sby = ty * SBS + t / SBS, sbx = tx * SBS + t % SBS;
            if (sby < J.ph && sbx < J.pw) J.flags[sby * J.pw + sbx] = 0;
        }
        if (t == 0) part[blockIdx.x] = 0;
        if (!planes) return;
    }
    const uint8_t PS_GLOBAL *src = PS_AS_GLOBAL(const uint8_t, J.src);
    uint8_t *s_b = (uint8_t *)s_w;
    const int r = t >> 2, s = t & 3;
    if (complete) {
        const ps_u32x4 d = *(const ps_u32x4 PS_GLOBAL *)(src + (size_t)(y0 + r) * J.stride + x0 + 16 * s);
        uint32_t *o = s_w + (r + 1) * PS_LDS_ROW + 1 + 4 * s;
        o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = d.w;
    } else {
        for (int i = t; i < 4096; i += 256) {
            const int yy = i >> 6, xx = i & 63;
            s_b[(yy + 1) * (4 * PS_LDS_ROW) + 4 + xx] = src[(size_t)ps_clamp(y0 + yy, H - 1) * J.stride + ps_clamp(x0 + xx, W - 1)];
        }
    }
    for (int i = t; i < 260; i += 256) { /* the one-sample ring; coordinates outside the picture are clamped, those samples are never used */
        int yy, xx;
        if (i < 66) { yy = -1; xx = i - 1; }
        else if (i < 132) { yy = 64; xx = i - 67; }
        else if (i < 196) { yy = i - 132; xx = -1; }
        else { yy = i - 196; xx = 64; }
        s_b[(yy + 1) * (4 * PS_LDS_ROW) + 4 + xx] = src[(size_t)ps_clamp(y0 + yy, H - 1) * J.stride + ps_clamp(x0 + xx, W - 1)];
    }
    __syncthreads();

    uint32_t acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    const int gy = y0 + r;
    if (M != 0 || !(r & 1) || planes) {
        const uint32_t *cp = s_w + (r + 1) * PS_LDS_ROW + 4 * s;
        uint32_t cw[6], tw[4], bw[4];
        _Pragma("unroll") for (int k = 0; k < 6; k++) cw[k] = cp[k];
        _Pragma("unroll") for (int k = 0; k < 4; k++) { tw[k] = cp[k + 1 - PS_LDS_ROW]; bw[k] = cp[k + 1 + PS_LDS_ROW]; }
        const bool row_in = gy > 0 && gy < H - 1;
        uint32_t dw[4] = {0, 0, 0, 0}, nw[4] = {0, 0, 0, 0};
        _Pragma("unroll") for (int k = 0; k < 16; k++) {
            const int      gx = x0 + 16 * s + k;
            const uint32_t c = ps_byte(cw, k + 4);
            uint32_t       d = c, n = 0;
            if (row_in && gx > 0 && gx < W - 1) { /* picture-border samples are copied and their noise is 0 (:1686-1697) */
                d = (ps_byte(tw, k) + ps_byte(cw, k + 3) + 4 * c + ps_byte(cw, k + 5) + ps_byte(bw, k)) >> 3;
                n = c > d ? c - d : 0;
            }
            dw[k >> 2] |= d << (8 * (k & 3));
            nw[k >> 2] |= n << (8 * (k & 3));
            acc[k >> 3][0] += d; acc[k >> 3][1] += d * d; acc[k >> 3][2] += n; acc[k >> 3][3] += n * n;
        }
        if (planes && gy < H) {
            _Pragma("unroll") for (int k = 0; k < 16; k++) {
                const int gx = x0 + 16 * s + k;
                if (gx < W) {
                    J.den[(size_t)gy * W + gx]   = (uint8_t)(dw[k >> 2] >> (8 * (k & 3)));
                    J.noise[(size_t)gy * W + gx] = (uint8_t)(nw[k >> 2] >> (8 * (k & 3)));
                }
            }
        }
        if (M == 0 && (r & 1)) _Pragma("unroll") for (int k = 0; k < 8; k++) acc[k >> 2][k & 3] = 0;
    }
    if (!stats) return;
    /* the 8 rows of an 8x8 block are the lanes that differ in bits 2..4 */
    _Pragma("unroll") for (int k = 0; k < 8; k++) {
        uint32_t v = acc[k >> 2][k & 3];
        v += __shfl_xor(v, 4); v += __shfl_xor(v, 8); v += __shfl_xor(v, 16);
        acc[k >> 2][k & 3] = v;
    }
    if (!(t & 28)) _Pragma("unroll") for (int k = 0; k < 8; k++) s_blk[k & 3][r >> 3][2 * s + (k >> 2)] = acc[k >> 2][k & 3];
    __syncthreads();

    if (M == 0) {
        if (t < 32) { /* 16x16 level: >> 2 averages of the four 8x8 children, as every level above */
            const int wh = t >> 4, by = (t >> 2) & 3, bx = t & 3;
            uint64_t  m = 0, q = 0;
            _Pragma("unroll") for (int k = 0; k < 4; k++) {
                m += (uint64_t)s_blk[2 * wh][2 * by + (k >> 1)][2 * bx + (k & 1)] << 3;
                q += (uint64_t)s_blk[2 * wh + 1][2 * by + (k >> 1)][2 * bx + (k & 1)] << 11;
            }
            s_m16[wh][t & 15] = m >> 2; s_q16[wh][t & 15] = q >> 2;
        }
        __syncthreads();
        if (t == 0) {
            uint64_t var[2];
            for (int wh = 0; wh < 2; wh++) {
                uint64_t m64 = 0, q64 = 0;
                for (int b = 0; b < 4; b++) {
                    const int o = (b >> 1) * 8 + (b & 1) * 2;
                    m64 += (s_m16[wh][o] + s_m16[wh][o + 1] + s_m16[wh][o + 4] + s_m16[wh][o + 5]) >> 2;
                    q64 += (s_q16[wh][o] + s_q16[wh][o + 1] + s_q16[wh][o + 4] + s_q16[wh][o + 5]) >> 2;
                }
                m64 >>= 2; q64 >>= 2;
                var[wh] = q64 - m64 * m64;
            }
            /* noiseBlkVar is compared in 16.16 and accumulated >> 16 (:3565-3574) */
            J.flags[ty * J.pw + tx] = (var[0] >> 16) < 50 && var[1] > noise_blk_th;
            part[blockIdx.x] = (uint32_t)(var[1] >> 16);
        }
    } else if (t < 64) {
        unsigned long long add = 0;
        if (t < SBS * SBS) {
            const int vy = t / SBS, hx = t % SBS;
            uint64_t  var[2];
            _Pragma("unroll") for (int wh = 0; wh < 2; wh++) {
                const int by0 = wh ? 0 : vy * (8 / SBS), bx0 = hx * (8 / SBS); /* noise: always the strip's first SB row */
                uint64_t  m = 0, q = 0;
                if (M == 1) {
                    _Pragma("unroll") for (int k = 0; k < 4; k++) {
                        m += (uint64_t)s_blk[2 * wh][by0 + (k >> 1)][bx0 + (k & 1)] << 2;
                        q += (uint64_t)s_blk[2 * wh + 1][by0 + (k >> 1)][bx0 + (k & 1)] << 10;
                    }
                } else {
                    /* compute_variance32x32 numbers its 8x8 blocks row * 4 + col and then groups {0,1,8,9}, {2,3,10,11}, {4,5,12,13},
                     * {6,7,14,15} (:301-329): block rows 0 + 2 and 1 + 3 are paired */
                    _Pragma("unroll") for (int g = 0; g < 4; g++) {
                        uint64_t gm = 0, gq = 0;
                        _Pragma("unroll") for (int k = 0; k < 4; k++) {
                            const int rr = (g >> 1) + 2 * (k >> 1), cc = 2 * (g & 1) + (k & 1);
                            gm += (uint64_t)s_blk[2 * wh][(by0 + rr) & 7][(bx0 + cc) & 7] << 2;
                            gq += (uint64_t)s_blk[2 * wh + 1][(by0 + rr) & 7][(bx0 + cc) & 7] << 10;
                        }
                        m += gm >> 2; q += gq >> 2;
                    }
                }
                m >>= 2; q >>= 2;
                var[wh] = q - m * m;
            }
            const int sby = ty * SBS + vy, sbx = tx * SBS + hx;
            if (sby < J.ph && sbx < J.pw) J.flags[sby * J.pw + sbx] = (var[0] >> 16) < 50 && var[1] > noise_blk_th;
            add = var[1] >> 16;
        }
        _Pragma("unroll") for (int o = 1; o < SBS * SBS; o <<= 1) add += __shfl_xor(add, o);
        if (t == 0) part[blockIdx.x] = (uint32_t)add; /* at most 16 values below 2^16 */
    }
}

/* one workgroup per picture: the sum over its tiles, the integer division of :3577-3580 and the class */
__global__ __launch_bounds__(256) void svt_pa_noise_class_kernel(const ps_noise_job *__restrict__ jobs, const uint32_t *__restrict__ part,
                                                                 svt_pa_noise_result *__restrict__ res, int method, int luma_height) {
    __shared__ unsigned long long s_sum;
    const int i = blockIdx.x, tile0 = jobs[i].tile0, n_tiles = jobs[i].tiles_x * jobs[i].tiles_y;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    unsigned long long sum = 0;
    for (int k = threadIdx.x; k < n_tiles; k += 256) sum += part[tile0 + k];
    atomicAdd(&s_sum, sum);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n = jobs[i].sb_count;
        res[i].pic_noise_variance_sum = s_sum;
        res[i].sb_count = n;
        res[i].pic_noise_class = ps_noise_class(method, n ? s_sum / n : 0, luma_height);
    }
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* histograms and average intensity                                                                                     */
/* ------------------------------------------------------------------------------------------------------------------ */
struct ps_hist_job {
    const uint8_t *pl[3];    /* sample (0,0) of the 1/16 luma, of Cb and of Cr */
    const uint8_t *full_buf; /* first byte of the padded full luma buffer (scd_mode 0 only) */
    uint32_t      *hist;     /* [regions_w][regions_h][3][256] */
    uint8_t       *avg_region, *avg;
    int32_t        stride[3], full_stride;
    int32_t        w16, h16, W, H;
};

constexpr int PS_MEAN_WGS = 64; /* workgroups per picture of the scd_mode 0 luma mean */

/* One workgroup per (picture, region, component).  Private 256-bin histogram per wave in LDS, merged once. */
__global__ __launch_bounds__(256) void svt_pa_hist_kernel(const ps_hist_job *__restrict__ jobs, int rw_n, int rh_n, uint64_t *__restrict__ region_sum) {
    __shared__ uint32_t           s_h[4][256];
    __shared__ unsigned long long s_sum;
    const ps_hist_job &J = jobs[blockIdx.y]; /* a reference: the component index is dynamic */
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const int c = blockIdx.x % 3, reg = blockIdx.x / 3, ri = reg / rh_n, rj = reg - ri * rh_n; /* [width index][height index] */
    for (int i = t; i < 1024; i += 256) (&s_h[0][0])[i] = 0;
    if (t == 0) s_sum = 0;
    __syncthreads();
    /* region geometry in the units of the picture the reference passes: the 1/16 luma for Y, the source luma for Cb / Cr */
    const int pw = c ? J.W : J.w16, ph = c ? J.H : J.h16;
    const int rw = pw / rw_n, rh = ph / rh_n;
    const int rwo = rw + (ri == rw_n - 1 ? pw - rw_n * rw : 0), rho = rh + (rj == rh_n - 1 ? ph - rh_n * rh : 0); /* the last region takes the remainder */
    int bx = ri * rw, by = rj * rh, aw = rwo, ah = rho, step = 1;
    if (c) { bx >>= 1; by >>= 1; aw >>= 1; ah >>= 1; step = 4; } /* chroma: every 4th row and column (calculate_histogram, :128-150) */
    const int nx = (aw + step - 1) / step, ny = (ah + step - 1) / step;
    const uint8_t PS_GLOBAL *p = PS_AS_GLOBAL(const uint8_t, J.pl[c]) + (size_t)by * J.stride[c] + bx;
    uint32_t sum = 0;
    for (int yy = wv; yy < ny; yy += 4) {
        const uint8_t PS_GLOBAL *row = p + (size_t)(yy * step) * J.stride[c];
        for (int xx = lane; xx < nx; xx += 64) {
            const uint32_t v = row[xx * step];
            atomicAdd(&s_h[wv][v], 1u);
            sum += v;
        }
    }
    atomicAdd(&s_sum, (unsigned long long)sum);
    __syncthreads();
    /* bins start at 1 and end << 4 (eb_vp9_initialize_buffer_32bits(.., 64, 0, 1), :4261-4266; the shifts at :4300-4307, :4389-4396) */
    J.hist[(size_t)blockIdx.x * 256 + t] = (1u + s_h[0][t] + s_h[1][t] + s_h[2][t] + s_h[3][t]) << 4;
    if (t == 0) {
        const uint64_t sm = s_sum;
        const uint32_t area = (uint32_t)rwo * (uint32_t)rho;
        J.avg_region[blockIdx.x] = c ? (uint8_t)(((sm << 4) + (area >> 3)) / (area >> 2)) : (uint8_t)((sm + (area >> 1)) / area);
        region_sum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sm << 4;
    }
}

/* scd_mode 0: the sum of eb_vp9_compute_sub_mean8x8_sse2_intrin over the (W >> 3) x (H >> 3) blocks the reference addresses from
 * buffer_y[0], that is from the first byte of the padded buffer, not from sample (0,0) (:4853-4862) */
__global__ __launch_bounds__(256) void svt_pa_luma_mean_kernel(const ps_hist_job *__restrict__ jobs, uint64_t *__restrict__ part) {
    __shared__ unsigned long long s_sum;
    const ps_hist_job J = jobs[blockIdx.y];
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const int bw = J.W >> 3, n = bw * (J.H >> 3);
    const uint8_t PS_GLOBAL *p = PS_AS_GLOBAL(const uint8_t, J.full_buf);
    uint64_t sum = 0;
    for (int b = blockIdx.x * 256 + threadIdx.x; b < n; b += PS_MEAN_WGS * 256) {
        const int by = b / bw, bx = b - by * bw;
        uint32_t  sm = 0;
        _Pragma("unroll") for (int rr = 0; rr < 8; rr += 2) {
            const ps_u32x2 d = *(const ps_u32x2 PS_GLOBAL *)(p + (size_t)(8 * by + rr) * J.full_stride + 8 * bx);
            _Pragma("unroll") for (int k = 0; k < 4; k++) sm += ((d.x >> (8 * k)) & 255u) + ((d.y >> (8 * k)) & 255u);
        }
        sum += (uint64_t)sm << 3;
    }
    atomicAdd(&s_sum, (unsigned long long)sum);
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.y * PS_MEAN_WGS + blockIdx.x] = s_sum;
}

/* calculate_input_average_intensity (:4839-4886): scd_mode 0 writes average_intensity[0] alone */
__global__ void svt_pa_avg_kernel(const ps_hist_job *__restrict__ jobs, int n_pics, int n_regions, int scd_mode, const uint64_t *__restrict__ region_sum,
                                  const uint64_t *__restrict__ part) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pics) return;
    const ps_hist_job J = jobs[i];
    const uint32_t wh = (uint32_t)J.W * (uint32_t)J.H;
    if (scd_mode == 0) {
        uint64_t mean = 0;
        for (int k = 0; k < PS_MEAN_WGS; k++) mean += part[i * PS_MEAN_WGS + k];
        mean = (mean + (wh >> 7)) / (wh >> 6);
        J.avg[0] = (uint8_t)((mean + 128) >> 8);
        return;
    }
    uint64_t tot[3] = {0, 0, 0};
    for (int k = 0; k < n_regions * 3; k++) tot[k % 3] += region_sum[(size_t)i * n_regions * 3 + k];
    J.avg[0] = (uint8_t)((tot[0] + (wh >> 1)) / wh);
    J.avg[1] = (uint8_t)((tot[1] + (wh >> 3)) / (wh >> 2));
    J.avg[2] = (uint8_t)((tot[2] + (wh >> 3)) / (wh >> 2));
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* chroma block means                                                                                                   */
/* ------------------------------------------------------------------------------------------------------------------ */
struct ps_cmean_job {
    const uint8_t *pl[2]; /* sample (0,0) of Cb, Cr */
    uint8_t       *out[2];
    int32_t        stride[2];
};

/* one wave per SB: lane = component * 16 + 8x8 chroma block (the 16x16 luma block it belongs to), rows 0, 2, 4, 6 of it */
__global__ __launch_bounds__(256) void svt_pa_chroma_mean_kernel(const ps_cmean_job *__restrict__ jobs, int width, int height, int nx, int n_sb) {
    __shared__ uint32_t s_mean[4][2][21];
    const ps_cmean_job &J = jobs[blockIdx.y];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, sb = blockIdx.x * 4 + w;
    const int sby = sb / nx, sbx = sb - sby * nx, c = (lane >> 4) & 1, b = lane & 15;
    const bool live = sb < n_sb, complete = live && sbx * 64 + 64 <= width && sby * 64 + 64 <= height;
    if (complete && lane < 32) {
        const uint8_t PS_GLOBAL *p = PS_AS_GLOBAL(const uint8_t, J.pl[c]) + (size_t)(sby * 32 + (b >> 2) * 8) * J.stride[c] + sbx * 32 + (b & 3) * 8;
        uint32_t sm = 0;
        _Pragma("unroll") for (int rr = 0; rr < 8; rr += 2) {
            const ps_u32x2 d = *(const ps_u32x2 PS_GLOBAL *)(p + (size_t)rr * J.stride[c]);
            _Pragma("unroll") for (int k = 0; k < 4; k++) sm += ((d.x >> (8 * k)) & 255u) + ((d.y >> (8 * k)) & 255u);
        }
        s_mean[w][c][5 + b] = sm << 3;
    }
    __syncthreads();
    if (complete && lane < 8) {
        const int cc = lane >> 2, q = lane & 3, o = 5 + (q >> 1) * 8 + (q & 1) * 2;
        s_mean[w][cc][1 + q] = (s_mean[w][cc][o] + s_mean[w][cc][o + 1] + s_mean[w][cc][o + 4] + s_mean[w][cc][o + 5]) >> 2;
    }
    __syncthreads();
    /* the 64x64 mean takes 32x32 block 3 twice and block 2 never (:2010-2015) */
    if (complete && lane < 2) s_mean[w][lane][0] = (s_mean[w][lane][1] + s_mean[w][lane][2] + s_mean[w][lane][4] + s_mean[w][lane][4]) >> 2;
    __syncthreads();
    /* incomplete SBs: zero_out_chroma_block_mean */
    if (live && lane < 42) J.out[lane / 21][(size_t)sb * 21 + lane % 21] = complete ? (uint8_t)(s_mean[w][lane / 21][lane % 21] >> 8) : 0;
}
} // namespace

static const svt_plane *ps_noise_plane(const svt_pa_picture *p, int method) { return method == 0 ? &p->full : method == 1 ? &p->sixteenth : &p->quarter; }

extern "C" int32_t svt_hip_pa_noise_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_pa_picture *pics, const svt_pa_noise_params *params,
                                                 uint8_t *const *d_sb_flat_noise, svt_pa_noise_result *d_result, uint8_t *const *d_denoised,
                                                 uint8_t *const *d_noise) {
    if (!ctx || n_pics < 1 || !pics || !params || !d_sb_flat_noise || !d_result) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa noise: null argument");
    if (params->method < 0 || params->method > 2 || (!d_denoised) != (!d_noise)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa noise: method / optional planes");
    HIP_TRY(hipSetDevice(ctx->device));
    const int M = params->method, sbs = M == 0 ? 1 : M == 1 ? 4 : 2, dec = M == 0 ? 1 : M == 1 ? 4 : 2;
    size_t tiles_max = 0; /* the job records are followed, on the device side only, by one partial sum per tile */
    for (int i = 0; i < n_pics; i++) tiles_max += (size_t)((pics[i].full.width + 63) / 64) * (size_t)((pics[i].full.height + 63) / 64);
    const size_t jobs_b = (sizeof(ps_noise_job) * (size_t)n_pics + 7) & ~(size_t)7;
    char *hb = nullptr, *db = nullptr; /* (the partial sums are written and read by this call's kernels only, all on ctx->stream) */
    if (svt_ctx_stage(ctx, jobs_b + sizeof(uint32_t) * tiles_max, (void **)&hb, (void **)&db)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "pa noise: scratch");
    ps_noise_job *h = (ps_noise_job *)hb, *d = (ps_noise_job *)db;
    uint32_t     *d_part = (uint32_t *)(db + jobs_b);
    int tiles = 0;
    for (int i = 0; i < n_pics; i++) {
        const svt_plane *pl = ps_noise_plane(&pics[i], M);
        const int        FW = pics[i].full.width, FH = pics[i].full.height;
        if (!pl->buf || !d_sb_flat_noise[i] || pl->width < 2 || pl->height < 2 || FW < 1 || FH < 1 || pl->width * dec > FW || pl->height * dec > FH ||
            pl->stride < pl->width + pl->origin_x || (d_denoised && (!d_denoised[i] || !d_noise[i])))
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa noise: plane geometry");
        ps_noise_job &J = h[i];
        J.src = pl->buf + (size_t)pl->origin_y * pl->stride + pl->origin_x;
        J.flags = d_sb_flat_noise[i];
        J.den = d_denoised ? d_denoised[i] : nullptr;
        J.noise = d_noise ? d_noise[i] : nullptr;
        J.stride = pl->stride; J.w = pl->width; J.h = pl->height;
        J.pw = (FW + 63) / 64; J.ph = (FH + 63) / 64;
        J.tiles_x = (J.pw + sbs - 1) / sbs; J.tiles_y = (J.ph + sbs - 1) / sbs;
        /* the full-precision loop runs over every SB; the decimated ones over height / 64 x width / 64 whole tiles (:3838-3839, :3959-3960) */
        J.vis_x = M == 0 ? J.tiles_x : pl->width / 64; J.vis_y = M == 0 ? J.tiles_y : pl->height / 64;
        J.sb_count = M == 0 ? (uint32_t)(pl->width / 64) * (uint32_t)(pl->height / 64) : (uint32_t)(J.vis_x * J.vis_y * sbs * sbs);
        J.tile0 = tiles;
        tiles += J.tiles_x * J.tiles_y;
    }
    /* noise_detection_th selects NOISE_MIN_LEVEL(_DECIM)_0 / _1 (:32-37); the quarter form tests it the other way round (:3884-3888) */
    const uint32_t th = M == 2 ? (params->noise_detection_th == 0 ? 120000u : 70000u) : (params->noise_detection_th == 1 ? 70000u : 120000u);
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof(ps_noise_job) * (size_t)n_pics));
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    if (M == 0) hipLaunchKernelGGL(svt_pa_noise_kernel<0>, dim3(tiles), dim3(256), 0, ctx->stream, (const ps_noise_job *)d, n_pics, th, d_part);
    else if (M == 1) hipLaunchKernelGGL(svt_pa_noise_kernel<1>, dim3(tiles), dim3(256), 0, ctx->stream, (const ps_noise_job *)d, n_pics, th, d_part);
    else hipLaunchKernelGGL(svt_pa_noise_kernel<2>, dim3(tiles), dim3(256), 0, ctx->stream, (const ps_noise_job *)d, n_pics, th, d_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(svt_pa_noise_class_kernel, dim3(n_pics), dim3(256), 0, ctx->stream, (const ps_noise_job *)d, (const uint32_t *)d_part, d_result, M,
                       params->luma_height);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_pa_histogram_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_pa_picture *pics, const svt_plane *cb, const svt_plane *cr,
                                                     int32_t regions_w, int32_t regions_h, int32_t scd_mode, uint32_t *const *d_hist,
                                                     uint8_t *const *d_avg_region, uint8_t *const *d_avg) {
    if (!ctx || n_pics < 1 || !pics || !cb || !cr || !d_hist || !d_avg_region || !d_avg) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa histogram: null argument");
    if (regions_w < 1 || regions_h < 1 || regions_w * regions_h > 1024) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa histogram: region counts");
    HIP_TRY(hipSetDevice(ctx->device));
    const int    n_reg = regions_w * regions_h;
    const size_t jobs_b = (sizeof(ps_hist_job) * (size_t)n_pics + 7) & ~(size_t)7, sums_b = sizeof(uint64_t) * (size_t)n_pics * n_reg * 3,
                 part_b = sizeof(uint64_t) * (size_t)n_pics * PS_MEAN_WGS;
    /* the job records, then (device side only) the region sums and the partial sums of the luma mean: this call's kernels write and read them, all on ctx->stream */
    char *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, jobs_b + sums_b + part_b, (void **)&h, (void **)&d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "pa histogram: scratch");
    ps_hist_job *hj = (ps_hist_job *)h;
    for (int i = 0; i < n_pics; i++) {
        const svt_plane *y = &pics[i].sixteenth, *f = &pics[i].full, *c2[2] = {&cb[i], &cr[i]};
        const int        W = f->width, H = f->height;
        if (!y->buf || !f->buf || !cb[i].buf || !cr[i].buf || !d_hist[i] || !d_avg_region[i] || !d_avg[i]) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa histogram: null plane");
        /* every region holds at least one luma sample of the 1/16 picture and a 2x2 of the source, and the chroma planes cover the picture */
        if (y->width / regions_w < 1 || y->height / regions_h < 1 || W / regions_w < 2 || H / regions_h < 2 || W < 8 || H < 8 ||
            cb[i].width < W / 2 || cb[i].height < H / 2 || cr[i].width < W / 2 || cr[i].height < H / 2 || f->stride < f->origin_x + W)
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa histogram: plane geometry");
        ps_hist_job &J = hj[i];
        J.pl[0] = y->buf + (size_t)y->origin_y * y->stride + y->origin_x; J.stride[0] = y->stride;
        for (int k = 0; k < 2; k++) { J.pl[1 + k] = c2[k]->buf + (size_t)c2[k]->origin_y * c2[k]->stride + c2[k]->origin_x; J.stride[1 + k] = c2[k]->stride; }
        J.full_buf = f->buf; J.full_stride = f->stride;
        J.hist = d_hist[i]; J.avg_region = d_avg_region[i]; J.avg = d_avg[i];
        J.w16 = y->width; J.h16 = y->height; J.W = W; J.H = H;
    }
    uint64_t *d_sums = (uint64_t *)(d + jobs_b), *d_part = (uint64_t *)(d + jobs_b + sums_b);
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof(ps_hist_job) * (size_t)n_pics));
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    hipLaunchKernelGGL(svt_pa_hist_kernel, dim3(n_reg * 3, n_pics), dim3(256), 0, ctx->stream, (const ps_hist_job *)d, regions_w, regions_h, d_sums);
    HIP_TRY(hipGetLastError());
    if (scd_mode == 0) {
        hipLaunchKernelGGL(svt_pa_luma_mean_kernel, dim3(PS_MEAN_WGS, n_pics), dim3(256), 0, ctx->stream, (const ps_hist_job *)d, d_part);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(svt_pa_avg_kernel, dim3((n_pics + 63) / 64), dim3(64), 0, ctx->stream, (const ps_hist_job *)d, n_pics, n_reg, scd_mode,
                       (const uint64_t *)d_sums, (const uint64_t *)d_part);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_pa_chroma_mean_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_plane *cb, const svt_plane *cr, int32_t width,
                                                       int32_t height, uint8_t *const *d_cb_mean, uint8_t *const *d_cr_mean) {
    if (!ctx || n_pics < 1 || !cb || !cr || !d_cb_mean || !d_cr_mean || width < 1 || height < 1) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa chroma mean: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    ps_cmean_job *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof(ps_cmean_job) * (size_t)n_pics, (void **)&h, (void **)&d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "pa chroma mean: scratch");
    const int nx = (width + 63) / 64, n_sb = nx * ((height + 63) / 64);
    for (int i = 0; i < n_pics; i++) {
        const svt_plane *c2[2] = {&cb[i], &cr[i]};
        for (int k = 0; k < 2; k++) {
            /* complete SBs only are read: 32 x 32 chroma samples at (32 * sbx, 32 * sby) */
            if (!c2[k]->buf || c2[k]->width < (width / 64) * 32 || c2[k]->height < (height / 64) * 32 || c2[k]->stride < c2[k]->origin_x + c2[k]->width)
                return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa chroma mean: plane geometry");
            h[i].pl[k] = c2[k]->buf + (size_t)c2[k]->origin_y * c2[k]->stride + c2[k]->origin_x;
            h[i].stride[k] = c2[k]->stride;
        }
        if (!d_cb_mean[i] || !d_cr_mean[i]) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "pa chroma mean: null output");
        h[i].out[0] = d_cb_mean[i]; h[i].out[1] = d_cr_mean[i];
    }
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof(ps_cmean_job) * (size_t)n_pics));
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    hipLaunchKernelGGL(svt_pa_chroma_mean_kernel, dim3((n_sb + 3) / 4, n_pics), dim3(256), 0, ctx->stream, (const ps_cmean_job *)d, width, height, nx, n_sb);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}

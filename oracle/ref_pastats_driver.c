/*
 * ref_pastats_driver.c -- harness that runs the REFERENCE's per-picture statistics of the picture-analysis process
 * (Source/Lib/Codec/EbPictureAnalysisProcess.c): detect_input_picture_noise (:3512-3619), quarter_sample_detect_noise
 * (:3809-3928), sub_sample_detect_noise (:3930-4055), the two *_generate_pixel_intensity_histogram_bins with
 * calculate_input_average_intensity (:4237-4432, :4839-4886), compute_chroma_block_mean / zero_out_chroma_block_mean
 * (:1767-2109) and compute_block_mean_compute_variance (:2115-3356).  TEST INFRASTRUCTURE ONLY (rules: ref_me_driver.c).
 * All of them are static in the reference file, which this harness therefore compiles as part of its own translation
 * unit.  It allocates the control-set objects those functions read and fills exactly the fields they read.
 *
 * request : int32 magic 'SVPS', kind, asm_types (eb_vp9_ASM_TYPES: 0 = C / SSE2 forms, 3 = AVX2 forms), then per kind;
 *           a plane is {int32 stride, origin_x, origin_y, rows} + stride * rows bytes (the whole padded buffer)
 *   1 noise    : int32 method (0 full, 1 half, 2 quarter), full width, full height, noise_detection_th, luma_height,
 *                analysed width, analysed height; the analysed plane
 *                -> sb_flat_noise_array u8[n_sb], int32 pic_noise_class, int32 0, double pic_noise_variance_float,
 *                   the denoised buffer (stride * rows bytes, 0xCD where nothing was written), the 64-row noise strip
 *                   (stride * (64 + 2 * origin_y) bytes, as the last strip left it)
 *   2 histogram: int32 W, H, regions per width, per height (1..4: the reference's arrays end there), scd_mode; the padded
 *                full luma, the 1/16 luma, Cb, Cr (origin = the luma's >> 1, as the reference addresses them)
 *                -> picture_histogram u32[rw][rh][3][256], average_intensity_per_region u8[rw][rh][3],
 *                   average_intensity u8[3] (0xEE where the reference leaves the entry alone)
 *   3 chroma   : int32 W, H, luma origin_x, origin_y; Cb, Cr -> cb_mean u8[n_sb][21], cr_mean u8[n_sb][21]
 *   4 mean/var : int32 W, H; the padded full luma -> y_mean u8[n_sb][85], variance u16[n_sb][85]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "EbDefinitions.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbPictureBufferDesc.h"

/* the reference's file itself, for its static composite functions */
#include "EbPictureAnalysisProcess.c"

static int rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n ? 0 : -1; }
static int rd_plane(FILE *f, uint8_t **buf, int32_t g[4]) {
    if (rd(f, g, 4 * sizeof(int32_t))) return -1;
    const size_t n = (size_t)g[0] * g[3];
    *buf = (uint8_t *)malloc(n + 64); /* (the SIMD forms load whole vectors) */
    return rd(f, *buf, n);
}

/* SB geometry as eb_vp9_sb_params_init (Codec/EbSequenceControlSet.c:281) leaves it */
static void sb_params(SequenceControlSet *scs, int W, int H) {
    const int nx = (W + 63) / 64, ny = (H + 63) / 64;
    scs->luma_width = (uint16_t)W; scs->luma_height = (uint16_t)H;
    scs->picture_width_in_sb = (uint8_t)nx; scs->sb_total_count = (uint16_t)(nx * ny);
    scs->sb_params_array = (SbParams *)calloc((size_t)(nx * ny), sizeof(SbParams));
    for (int y = 0; y < ny; y++)
        for (int x = 0; x < nx; x++) {
            SbParams *p = &scs->sb_params_array[y * nx + x];
            p->origin_x = (uint16_t)(x * 64); p->origin_y = (uint16_t)(y * 64);
            p->width  = (uint8_t)(W - x * 64 < 64 ? W - x * 64 : 64);
            p->height = (uint8_t)(H - y * 64 < 64 ? H - y * 64 : 64);
            p->is_complete_sb = (uint8_t)(p->width == 64 && p->height == 64);
        }
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[3], a[8], g[4];
    if (rd(f, h, sizeof h) || h[0] != 0x53505653) return 3; /* 'SVPS' */
    eb_vp9_ASM_TYPES = (uint32_t)h[2];
    SequenceControlSet      *scs = (SequenceControlSet *)calloc(1, sizeof *scs);
    PictureParentControlSet *pcs = (PictureParentControlSet *)calloc(1, sizeof *pcs);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;

    if (h[1] == 1) {
        if (rd(f, a, 7 * sizeof(int32_t))) return 3;
        const int method = a[0], FW = a[1], FH = a[2], w = a[5], hh = a[6];
        EbPictureBufferDesc in, den, noise;
        memset(&in, 0, sizeof in);
        if (rd_plane(f, &in.buffer_y, g)) return 3;
        in.stride_y = (uint16_t)g[0]; in.origin_x = (uint16_t)g[1]; in.origin_y = (uint16_t)g[2];
        in.width = (uint16_t)w; in.height = (uint16_t)hh;
        den = in; noise = in;
        const size_t n_den = (size_t)g[0] * g[3], n_noise = (size_t)g[0] * (64 + 2 * g[2]);
        den.buffer_y = (uint8_t *)malloc(n_den + 64); memset(den.buffer_y, 0xCD, n_den);
        noise.buffer_y = (uint8_t *)malloc(n_noise + 64); memset(noise.buffer_y, 0xCD, n_noise);
        noise.height = 64;
        sb_params(scs, FW, FH);
        scs->luma_height = (uint16_t)a[4];
        const int n_sb = scs->sb_total_count;
        pcs->sb_total_count = (uint16_t)n_sb;
        pcs->noise_detection_th = (uint8_t)a[3];
        pcs->sb_flat_noise_array = (uint8_t *)calloc((size_t)n_sb, 1); /* (the caller resets the flags, :3640 and its twins) */
        PictureAnalysisContext *pac = (PictureAnalysisContext *)calloc(1, sizeof *pac);
        EbErrorType rc;
        if (method == 0) rc = detect_input_picture_noise(pac, scs, pcs, &in, &noise, &den);
        else if (method == 1) rc = sub_sample_detect_noise(pac, scs, pcs, &in, &noise, &den, scs->picture_width_in_sb);
        else rc = quarter_sample_detect_noise(pac, pcs, &in, &noise, &den, scs->picture_width_in_sb);
        if (rc != EB_ErrorNone) return 4;
        int32_t cls[2] = {(int32_t)pcs->pic_noise_class, 0};
        fwrite(pcs->sb_flat_noise_array, 1, (size_t)n_sb, o);
        fwrite(cls, sizeof(int32_t), 2, o);
        fwrite(&pac->pic_noise_variance_float, sizeof(double), 1, o);
        fwrite(den.buffer_y, 1, n_den, o);
        fwrite(noise.buffer_y, 1, n_noise, o);
    } else if (h[1] == 2) {
        if (rd(f, a, 5 * sizeof(int32_t))) return 3;
        const int W = a[0], H = a[1], rw = a[2], rh = a[3];
        if (rw < 1 || rh < 1 || rw > MAX_NUMBER_OF_REGIONS_IN_WIDTH || rh > MAX_NUMBER_OF_REGIONS_IN_HEIGHT) return 3;
        EbPictureBufferDesc in, y16;
        memset(&in, 0, sizeof in); memset(&y16, 0, sizeof y16);
        if (rd_plane(f, &in.buffer_y, g)) return 3;
        in.stride_y = (uint16_t)g[0]; in.origin_x = (uint16_t)g[1]; in.origin_y = (uint16_t)g[2];
        in.width = (uint16_t)W; in.height = (uint16_t)H;
        if (rd_plane(f, &y16.buffer_y, g)) return 3;
        y16.stride_y = (uint16_t)g[0]; y16.origin_x = (uint16_t)g[1]; y16.origin_y = (uint16_t)g[2];
        y16.width = (uint16_t)(W >> 2); y16.height = (uint16_t)(H >> 2);
        if (rd_plane(f, &in.buffer_cb, g)) return 3;
        in.stride_cb = (uint16_t)g[0];
        if (rd_plane(f, &in.buffer_cr, g)) return 3;
        in.stride_cr = (uint16_t)g[0];
        scs->picture_analysis_number_of_regions_per_width = (uint32_t)rw;
        scs->picture_analysis_number_of_regions_per_height = (uint32_t)rh;
        scs->scd_mode = a[4] ? SCD_MODE_1 : SCD_MODE_0;
        pcs->picture_histogram = (uint32_t ****)calloc((size_t)rw, sizeof(uint32_t ***));
        for (int i = 0; i < rw; i++) {
            pcs->picture_histogram[i] = (uint32_t ***)calloc((size_t)rh, sizeof(uint32_t **));
            for (int j = 0; j < rh; j++) {
                pcs->picture_histogram[i][j] = (uint32_t **)calloc(3, sizeof(uint32_t *));
                for (int c = 0; c < 3; c++) pcs->picture_histogram[i][j][c] = (uint32_t *)calloc(HISTOGRAM_NUMBER_OF_BINS, sizeof(uint32_t));
            }
        }
        memset(pcs->average_intensity, 0xEE, sizeof pcs->average_intensity);
        uint64_t sy = 0, scb = 0, scr = 0; /* the call sequence of gathering_picture_statistics (:4899-4925) */
        sub_sample_luma_generate_pixel_intensity_histogram_bins(scs, pcs, &y16, &sy);
        sub_sample_chroma_generate_pixel_intensity_histogram_bins(scs, pcs, &in, &scb, &scr);
        calculate_input_average_intensity(scs, pcs, &in, sy, scb, scr);
        for (int i = 0; i < rw; i++)
            for (int j = 0; j < rh; j++)
                for (int c = 0; c < 3; c++) fwrite(pcs->picture_histogram[i][j][c], sizeof(uint32_t), HISTOGRAM_NUMBER_OF_BINS, o);
        for (int i = 0; i < rw; i++)
            for (int j = 0; j < rh; j++)
                for (int c = 0; c < 3; c++) { uint8_t b = (uint8_t)pcs->average_intensity_per_region[i][j][c]; fwrite(&b, 1, 1, o); }
        fwrite(pcs->average_intensity, 1, 3, o);
    } else if (h[1] == 3 || h[1] == 4) {
        if (rd(f, a, (h[1] == 3 ? 4 : 2) * sizeof(int32_t))) return 3;
        const int W = a[0], H = a[1];
        sb_params(scs, W, H);
        const int n_sb = scs->sb_total_count;
        EbPictureBufferDesc in;
        memset(&in, 0, sizeof in);
        in.width = (uint16_t)W; in.height = (uint16_t)H;
        pcs->y_mean = (uint8_t **)calloc((size_t)n_sb, sizeof(uint8_t *)); pcs->variance = (uint16_t **)calloc((size_t)n_sb, sizeof(uint16_t *));
        pcs->cb_mean = (uint8_t **)calloc((size_t)n_sb, sizeof(uint8_t *)); pcs->cr_mean = (uint8_t **)calloc((size_t)n_sb, sizeof(uint8_t *));
        for (int i = 0; i < n_sb; i++) {
            pcs->y_mean[i] = (uint8_t *)malloc(85); pcs->variance[i] = (uint16_t *)malloc(85 * 2);
            pcs->cb_mean[i] = (uint8_t *)malloc(21); pcs->cr_mean[i] = (uint8_t *)malloc(21);
            memset(pcs->y_mean[i], 0xCD, 85); memset(pcs->variance[i], 0xCD, 85 * 2);
            memset(pcs->cb_mean[i], 0xCD, 21); memset(pcs->cr_mean[i], 0xCD, 21);
        }
        if (h[1] == 3) {
            in.origin_x = (uint16_t)a[2]; in.origin_y = (uint16_t)a[3];
            if (rd_plane(f, &in.buffer_cb, g)) return 3;
            in.stride_cb = (uint16_t)g[0];
            if (rd_plane(f, &in.buffer_cr, g)) return 3;
            in.stride_cr = (uint16_t)g[0];
        } else {
            if (rd_plane(f, &in.buffer_y, g)) return 3;
            in.stride_y = (uint16_t)g[0]; in.origin_x = (uint16_t)g[1]; in.origin_y = (uint16_t)g[2];
        }
        for (int i = 0; i < n_sb; i++) { /* the per-SB calls of compute_picture_spatial_statistics (:4800-4822) with its addresses */
            const SbParams *p = &scs->sb_params_array[i];
            if (h[1] == 4)
                compute_block_mean_compute_variance(pcs, &in, (uint32_t)i, (uint32_t)((in.origin_y + p->origin_y) * in.stride_y + in.origin_x + p->origin_x));
            else if (p->is_complete_sb)
                compute_chroma_block_mean(pcs, &in, (uint32_t)i, (uint32_t)(((in.origin_y + p->origin_y) >> 1) * in.stride_cb + ((in.origin_x + p->origin_x) >> 1)),
                                          (uint32_t)(((in.origin_y + p->origin_y) >> 1) * in.stride_cr + ((in.origin_x + p->origin_x) >> 1)));
            else
                zero_out_chroma_block_mean(pcs, (uint32_t)i);
        }
        if (h[1] == 3) {
            for (int i = 0; i < n_sb; i++) fwrite(pcs->cb_mean[i], 1, 21, o);
            for (int i = 0; i < n_sb; i++) fwrite(pcs->cr_mean[i], 1, 21, o);
        } else {
            for (int i = 0; i < n_sb; i++) fwrite(pcs->y_mean[i], 1, 85, o);
            for (int i = 0; i < n_sb; i++) fwrite(pcs->variance[i], 2, 85, o);
        }
    } else
        return 3;
    fclose(f);
    fclose(o);
    return 0;
}

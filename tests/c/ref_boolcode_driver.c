/*
 * ref_boolcode_driver.c -- runs the REFERENCE's bool coder and writes what it produced: pack_mb_tokens + eb_vp9_stop_encode
 * (VPX/vp9_bitstream.c:98-162, VPX/bitwriter.c) over token streams under the probabilities eb_vp9_default_coef_probs leaves, and
 * vpx_write (VPX/bitwriter.h:34-84) over raw bool streams.  Compiled by tests/gen_golden_boolcode.py against the reference's headers
 * and linked with the reference's own objects; the three translation units the oracle's object set lacks are compiled into this one
 * by the includes below (pack_mb_tokens is static there).  Nothing of the reference is copied here.
 *
 * request : int32 magic, n_streams; per stream int32 kind, n; kind 0: n x {int32 token, extra, prob_row}; kind 1: n x uint16
 *           (bit << 8 | prob)
 * response: coef_probs[576 * 3], pareto[255 * 8], cat_probs[6 * 14] (uint8); per stream uint32 size, the bytes, double seconds of
 *           one pass of the reference's packing (the best of REPEAT)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>

#include "vpx_dsp_rtcd.h"
#include "vp9_rtcd.h"
#include "prob.c"
#include "bitwriter.c"
#include "vp9_bitstream.c"

#define REPEAT 20

static double drv_now(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2 || hdr[0] != 0x4c4f4f42) return 4;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 5;

    VP9_COMMON *cm = calloc(1, sizeof *cm);
    cm->fc = calloc(1, sizeof *cm->fc);
    eb_vp9_default_coef_probs(cm);
    const vpx_prob *prob_base = &cm->fc->coef_probs[0][0][0][0][0][0];
    if (sizeof cm->fc->coef_probs != 576 * 3 || sizeof eb_vp9_pareto8_full != 255 * 8) return 6;
    fwrite(prob_base, 1, 576 * 3, out);
    fwrite(eb_vp9_pareto8_full, 1, 255 * 8, out);
    for (int t = CATEGORY1_TOKEN; t <= CATEGORY6_TOKEN; t++) {
        uint8_t row[14] = {0};
        if (eb_vp9_extra_bits[t].len > 14) return 7;
        memcpy(row, eb_vp9_extra_bits[t].prob, (size_t)eb_vp9_extra_bits[t].len);
        fwrite(row, 1, 14, out);
    }

    for (int s = 0; s < hdr[1]; s++) {
        int32_t kn[2];
        if (fread(kn, 4, 2, f) != 2 || kn[1] < 0) return 8;
        const int n = kn[1];
        uint8_t  *buf = malloc((size_t)n * 24 + 64);
        double    best = 1e30;
        uint32_t  size = 0;
        if (kn[0] == 0) {
            int32_t    *rec = malloc(sizeof(int32_t) * 3 * (size_t)(n + 1));
            TOKENEXTRA *tok = calloc((size_t)n + 1, sizeof *tok);
            if (fread(rec, 12, (size_t)n, f) != (size_t)n) return 9;
            for (int i = 0; i < n; i++) {
                tok[i].token = (int16_t)rec[3 * i]; tok[i].extra = (int16_t)rec[3 * i + 1];
                tok[i].context_tree = prob_base + 3 * rec[3 * i + 2];
            }
            for (int rep = 0; rep < REPEAT; rep++) {
                VpxWriter   w;
                TOKENEXTRA *tp = tok;
                const double t0 = drv_now();
                eb_vp9_start_encode(&w, buf);
                pack_mb_tokens(&w, &tp, tok + n, VPX_BITS_8);
                eb_vp9_stop_encode(&w);
                const double dt = drv_now() - t0;
                if (tp != tok + n) return 10;
                best = dt < best ? dt : best;
                size = w.pos;
            }
            free(rec); free(tok);
        } else {
            uint16_t *b = malloc(sizeof(uint16_t) * (size_t)(n + 1));
            if (fread(b, 2, (size_t)n, f) != (size_t)n) return 11;
            for (int rep = 0; rep < REPEAT; rep++) {
                VpxWriter    w;
                const double t0 = drv_now();
                eb_vp9_start_encode(&w, buf);
                for (int i = 0; i < n; i++) vpx_write(&w, b[i] >> 8, b[i] & 255);
                eb_vp9_stop_encode(&w);
                const double dt = drv_now() - t0;
                best = dt < best ? dt : best;
                size = w.pos;
            }
            free(b);
        }
        fwrite(&size, 4, 1, out);
        fwrite(buf, 1, size, out);
        fwrite(&best, 8, 1, out);
        free(buf);
    }
    fclose(f);
    fclose(out);
    return 0;
}

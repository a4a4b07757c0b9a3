/*
 * ref_invtx_driver.c -- harness that runs the REFERENCE's inverse transforms on dequantised coefficients given to it directly: the eob
 * dispatch of VPX/vp9_idct.c:111-189 restated over the reference's own eb_vp9_idct*_add_c / eb_vp9_iht*_add_c kernels (VPX/inv_txfm.c,
 * VPX/vp9_idct.c; the wrappers themselves go through run-time-dispatch pointers that stay NULL here), exactly as tests/svt_testlib.py's
 * ref_inv_add does through libsvtref_kernels.so.  TEST INFRASTRUCTURE ONLY (rules: ref_me_driver.c).  Built twice (oracle/Makefile):
 * ref_invtx plain, ref_invtx_ubsan with the reference objects and this file under -fsanitize=signed-integer-overflow,shift
 * -fno-sanitize-recover=all, so that a request outside the domain in which the reference's C is defined ends the program.
 *
 * argv: request file, output file.  Request: int32 count, then per block int32 tx_size, tx_type, eob; N * N prediction bytes; N * N int16
 * dqcoeff (raster).  Output: the N * N reconstructed bytes of every block, in order.  With a third argument "each" a failing block is named
 * on stderr before it runs (the sanitizer's own message follows).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vpx_dsp_rtcd.h"
#include "vp9_rtcd.h"

static void inv_add(const int16_t *d, uint8_t *p, int n, int ts, int tt, int eob) {
    if (tt != 0 && ts < 3) {
        if (ts == 0) eb_vp9_iht4x4_16_add_c(d, p, n, tt);
        else if (ts == 1) eb_vp9_iht8x8_64_add_c(d, p, n, tt);
        else eb_vp9_iht16x16_256_add_c(d, p, n, tt);
    } else if (ts == 0) {
        if (eob > 1) eb_vp9_idct4x4_16_add_c(d, p, n);
        else eb_vp9_idct4x4_1_add_c(d, p, n);
    } else if (ts == 1) {
        if (eob == 1) eb_vp9_idct8x8_1_add_c(d, p, n);
        else if (eob <= 12) eb_vp9_idct8x8_12_add_c(d, p, n);
        else eb_vp9_idct8x8_64_add_c(d, p, n);
    } else if (ts == 2) {
        if (eob == 1) eb_vp9_idct16x16_1_add_c(d, p, n);
        else if (eob <= 10) eb_vp9_idct16x16_10_add_c(d, p, n);
        else if (eob <= 38) eb_vp9_idct16x16_38_add_c(d, p, n);
        else eb_vp9_idct16x16_256_add_c(d, p, n);
    } else {
        if (eob == 1) eb_vp9_idct32x32_1_add_c(d, p, n);
        else if (eob <= 34) eb_vp9_idct32x32_34_add_c(d, p, n);
        else if (eob <= 135) eb_vp9_idct32x32_135_add_c(d, p, n);
        else eb_vp9_idct32x32_1024_add_c(d, p, n);
    }
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s request output [each]\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    int32_t count = 0, head[3];
    if (!in || !out || fread(&count, 4, 1, in) != 1) { fprintf(stderr, "cannot open the files\n"); return 2; }
    static int16_t dq[32 * 32];
    static uint8_t px[32 * 32];
    for (int b = 0; b < count; b++) {
        if (fread(head, 4, 3, in) != 3 || head[0] < 0 || head[0] > 3 || head[1] < 0 || head[1] > 3) { fprintf(stderr, "bad block %d\n", b); return 2; }
        const int n = 4 << head[0], nn = n * n;
        if (fread(px, 1, nn, in) != (size_t)nn || fread(dq, 2, nn, in) != (size_t)nn) { fprintf(stderr, "short block %d\n", b); return 2; }
        if (argc > 3) { fprintf(stderr, "block %d\n", b); fflush(stderr); }
        if (head[2] != 0) inv_add(dq, px, n, head[0], head[1], head[2]); /* (eob 0: the prediction stays) */
        if (fwrite(px, 1, nn, out) != (size_t)nn) return 2;
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}

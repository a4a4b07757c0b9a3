/*
 * ref_fwdtq_driver.c -- harness that runs the REFERENCE's forward half of perform_coding_loop (Codec/EbEncDecProcess.c:390-560) on blocks
 * given to it directly: eb_vp9_residual_kernel (C_DEFAULT/EbPictureOperators_C.c:204) -> eb_vp9_fdct32x32_c / eb_vpx_partial_fdct32x32_c /
 * eb_vp9_fht16x16_c / eb_vp9_fht8x8_c / eb_vp9_fht4x4_c, and for a 4x4 DCT_DCT block eb_vp9_fdct4x4_c, the function the encode pass
 * reaches through eb_vpx_fdct4x4 (VPX/fwd_txfm.c, VPX/vp9_dct.c) -> eb_vp9_quantize_b_c / eb_vp9_quantize_b_32x32_c (VPX/quantize.c) with the
 * reference's own scan tables (VPX/vp9_scan.c).  The run-time-dispatch pointers stay NULL; the `_c` functions are called by name.
 * TEST INFRASTRUCTURE ONLY (rules: ref_me_driver.c).  Built twice (oracle/Makefile): ref_fwdtq plain, ref_fwdtq_ubsan with the reference
 * objects and this file under -fsanitize=signed-integer-overflow,shift -fno-sanitize-recover=all, so that a request outside the domain in
 * which the reference's C is defined ends the program.
 *
 * argv: request file, output file.  Request: int32 count, then per block int32 tx_size, tx_type, partial32; ten int16: zbin, round, quant,
 * quant_shift, dequant as [DC, AC] pairs; N * N source bytes; N * N prediction bytes.  Output per block: N * N int16 coefficients, qcoeff,
 * dqcoeff (raster), then int32 eob.  With a third argument "each" every block is named on stderr before it runs (the sanitizer's own
 * message follows).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vpx_dsp_rtcd.h"
#include "vp9_rtcd.h"
#include "vp9_scan.h"
#include "EbPictureOperators_C.h"

typedef char tran_low_is_16_bits[sizeof(tran_low_t) == 2 ? 1 : -1]; /* the response is read as int16 */

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s request output [each]\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    int32_t count = 0, head[3];
    if (!in || !out || fread(&count, 4, 1, in) != 1) { fprintf(stderr, "cannot open the files\n"); return 2; }
    static uint8_t    src[32 * 32], pred[32 * 32];
    static int16_t    res[32 * 32], qt[10];
    static tran_low_t coeff[32 * 32], q[32 * 32], dq[32 * 32];
    for (int b = 0; b < count; b++) {
        if (fread(head, 4, 3, in) != 3 || head[0] < 0 || head[0] > 3 || head[1] < 0 || head[1] > 3 || (head[0] == 3 && head[1])) { fprintf(stderr, "bad block %d\n", b); return 2; }
        const int n = 4 << head[0], nn = n * n;
        if (fread(qt, 2, 10, in) != 10 || fread(src, 1, nn, in) != (size_t)nn || fread(pred, 1, nn, in) != (size_t)nn) { fprintf(stderr, "short block %d\n", b); return 2; }
        if (argc > 3) { fprintf(stderr, "block %d\n", b); fflush(stderr); }
        const scan_order *so = head[0] == 3 ? &eb_vp9_default_scan_orders[TX_32X32] : &eb_vp9_scan_orders[head[0]][head[1]];
        uint16_t          eob = 0;
        eb_vp9_residual_kernel(src, n, pred, n, res, n, n, n);
        memset(coeff, 0, sizeof coeff); /* (:404: the partial transform writes its low 16x16 only) */
        if (head[0] == 3) {
            if (head[2]) eb_vpx_partial_fdct32x32_c(res, coeff, n);
            else eb_vp9_fdct32x32_c(res, coeff, n);
            eb_vp9_quantize_b_32x32_c(coeff, nn, 0, qt, qt + 2, qt + 4, qt + 6, q, dq, qt + 8, &eob, so->scan, so->iscan);
        } else {
            if (head[0] == 2) eb_vp9_fht16x16_c(res, coeff, n, head[1]);
            else if (head[0] == 1) eb_vp9_fht8x8_c(res, coeff, n, head[1]);
            else if (head[1] == DCT_DCT) eb_vp9_fdct4x4_c(res, coeff, n); /* :548 */
            else eb_vp9_fht4x4_c(res, coeff, n, head[1]);
            eb_vp9_quantize_b_c(coeff, nn, 0, qt, qt + 2, qt + 4, qt + 6, q, dq, qt + 8, &eob, so->scan, so->iscan);
        }
        const int32_t e = eob;
        if (fwrite(coeff, sizeof(tran_low_t), nn, out) != (size_t)nn || fwrite(q, sizeof(tran_low_t), nn, out) != (size_t)nn ||
            fwrite(dq, sizeof(tran_low_t), nn, out) != (size_t)nn || fwrite(&e, 4, 1, out) != 1)
            return 2;
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}

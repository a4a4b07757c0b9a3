/*
 * entropy_coef_check.c -- stand-alone driver of svt_hip_entropy_picture_coef for the sanitizer test (tests/test_entropy_coef_host.py): the
 * file format of tests/c/entropy_check.c; every input in an allocation of exactly its bytes, the counts the caller's for every second
 * picture and the form's own otherwise; prints, per picture, the packet's size, the result's flags, the sum of the packet's bytes and the
 * transform sizes sent.  Built from host/ alone, with its own main.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "svtvp9_hip.h"

int32_t svt_set_error_c(int32_t code, const char *msg) { (void)msg; return code; } /* (the library's lives in csrc/api.hip) */

static void *take(FILE *f, size_t n, size_t align) {
    void *p = NULL;
    if (!n) return NULL;
    if (align > 1) { if (posix_memalign(&p, align, n)) exit(3); }
    else p = malloc(n);
    if (!p || fread(p, 1, n, f) != n) exit(3);
    return p;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 3;
    svt_bool_tables        *tb = (svt_bool_tables *)take(f, sizeof *tb, 1);
    svt_modes_tables       *tm = (svt_modes_tables *)take(f, sizeof *tm, 1);
    svt_modes_inter_tables *ti = (svt_modes_inter_tables *)take(f, sizeof *ti, 1);
    for (uint32_t i = 0; i < n_cases; i++) {
        struct { int32_t mi_stride; uint32_t max_tokens, max_bools, max_tile_bytes, mc_bytes; } h;
        svt_entropy_picture pic;
        uint32_t            sizes[3];
        if (fread(&h, sizeof h, 1, f) != 1 || fread(&pic, sizeof pic, 1, f) != 1 || fread(sizes, sizeof sizes, 1, f) != 1) return 3;
        void *lf = take(f, sizes[0], 1), *mc = take(f, h.mc_bytes, 1), *q = take(f, sizes[1], 16), *em = take(f, sizes[2], 1);
        pic.d_lf_mi = (const svt_lf_mode_info *)lf; pic.d_mc_mi = (const svt_mc_mode_info *)mc; pic.d_qcoeff = (const int16_t *)q; pic.d_eob_map = (const uint16_t *)em;
        pic.d_counts = i & 1 ? (uint32_t *)malloc(SVT_TOK_COUNTS * sizeof(uint32_t)) : NULL;
        const svt_entropy_limits lim = {1, h.max_tokens, h.max_bools, h.max_tile_bytes};
        const uint32_t           cap = SVT_FRAME_UNCOMPRESSED_MAX + svt_hip_boolcode_capacity(svt_hip_coef_update_bools_capacity()) + h.max_tile_bytes + 4;
        uint8_t                 *packet = (uint8_t *)malloc(cap), *probs = (uint8_t *)malloc(SVT_CU_PROBS);
        uint32_t                 size = 0, sum = 0;
        svt_entropy_result       r;
        svt_entropy_host_detail  d;
        svt_cu_result            u;
        const int32_t            rc = svt_hip_entropy_picture_coef(tb, tm, ti, &pic, h.mi_stride, &lim, packet, cap, &size, &r, &d, probs, &u);
        if (rc) { fprintf(stderr, "case %u: rc %d\n", i, rc); return 4; }
        if (size != SVT_FRAME_SIZE_NONE)
            for (uint32_t k = 0; k < size; k++) sum += packet[k];
        for (uint32_t k = 0; k < SVT_CU_PROBS; k++) sum += probs[k];
        printf("%u %u %u %u\n", size, r.flags, sum, u.sent[0] + u.sent[1] + u.sent[2] + u.sent[3]);
        free(lf); free(mc); free(q); free(em); free(pic.d_counts); free(packet); free(probs);
    }
    free(tb); free(tm); free(ti);
    fclose(f);
    return 0;
}

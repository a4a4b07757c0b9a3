/*
 * ref_coef_update_driver.c -- runs the REFERENCE's write_compressed_header (VPX/vp9_bitstream.c:1292-1367) with the counts its encoder
 * never fills: cpi->td.rd_counts.coef_counts, cm->counts.eob_branch and counts->tx.tx_totals come from the request, cm->fc->coef_probs is
 * the request's "old" table, sf.use_fast_coef_updates = TWO_LOOP and sf.coeff_prob_appx_step = 1; every other count is zero, profile 0,
 * tx_mode ALLOW_32X32, as tests/c/ref_frame_driver.c sets them.  Returns the compressed header's bytes and cm->fc->coef_probs afterwards,
 * and the reference's tables: eb_vp9_prob_cost, and remap_prob / prob_diff_update_cost for all 255 x 255 (newp, oldp) pairs.  Compiled by
 * tests/gen_golden_coef_update.py against the reference's headers and linked with the reference's own objects; the translation units
 * the oracle's object set lacks are compiled into this one by the includes below.  Nothing of the reference is copied here.
 *
 * While it runs the driver notes which branches the reference takes: per transform size it calls the reference's own
 * build_tree_distribution and savings searches once more on the state in front of the write and classifies the TWO_LOOP exit (not
 * searched / no entry updates / savings negative / sent); per updated entry (the probability differs afterwards) the arm of
 * encode_term_subexp and encode_uniform its remap index takes, and whether the new probability lies above or below the old one.
 *
 * request : int32 magic, n_cases; per case int32 inter (0: key frame, 1: inter picture), reference_mode, allow_comp_inter_inter,
 *           allow_high_precision_mv (what the records behind the coefficient section depend on), uint32 tx_totals[4], uint32 coef_counts[6912], uint32 eob_branch[576], uint8 old coef_probs[1728]
 * response: per case uint32 size, the compressed header's bytes, uint8 coef_probs[1728], int32 exit[4] (enum exits), int32 updates[4],
 *           int64 savings[4] (0 where not searched); then uint16 cost[256], uint8 remap[255 * 255], uint8 bits[255 * 255] (index
 *           (newp - 1) * 255 + oldp - 1, 0 on the diagonal), uint32 coverage mask (enum cov)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "vpx_dsp_rtcd.h"
#include "vp9_rtcd.h"
#include "prob.c"
#include "bitwriter.c"
#include "bitwriter_buffer.c"
#include "vp9_entropymode.c"
#include "vp9_entropymv.c"
#include "vp9_encodemv.c"
#include "vp9_subexp.c"
#include "vp9_tile_common.c"
#include "vp9_pred_common.c"
#include "vp9_bitstream.c"

enum exits { X_NOT_SEARCHED, X_NO_ENTRY, X_NEGATIVE, X_SENT };
enum cov { V_NOT_SEARCHED, V_NO_ENTRY, V_NEGATIVE, V_SENT, V_SUBEXP_16, V_SUBEXP_32, V_SUBEXP_64, V_UNIFORM_SHORT, V_UNIFORM_LONG, V_NEWP_ABOVE, V_NEWP_BELOW, V_COUNT };

/* the TWO_LOOP dry run of one size, through the reference's own functions */
static int classify(VP9_COMP *cpi, TX_SIZE tx_size, int *updates, int64_t *savings) {
    vp9_coeff_stats       ct[PLANE_TYPES];
    vp9_coeff_probs_model np[PLANE_TYPES];
    *updates = 0; *savings = 0;
    if (cpi->td.counts->tx.tx_totals[tx_size] <= 20) return X_NOT_SEARCHED;
    build_tree_distribution(cpi, tx_size, ct, np);
    vp9_coeff_probs_model *old = cpi->common.fc->coef_probs[tx_size];
    int                    sum = 0;
    for (int i = 0; i < PLANE_TYPES; ++i)
        for (int j = 0; j < REF_TYPES; ++j)
            for (int k = 0; k < COEF_BANDS; ++k)
                for (int l = 0; l < BAND_COEFF_CONTEXTS(k); ++l)
                    for (int t = 0; t < UNCONSTRAINED_NODES; ++t) {
                        vpx_prob       newp = np[i][j][k][l][t];
                        const vpx_prob oldp = old[i][j][k][l][t];
                        const int      s = t == PIVOT_NODE ? eb_vp9_prob_diff_update_savings_search_model(ct[i][j][k][l][0], oldp, &newp, DIFF_UPDATE_PROB, 1)
                                                           : eb_vp9_prob_diff_update_savings_search(ct[i][j][k][l][t], oldp, &newp, DIFF_UPDATE_PROB);
                        const int      u = s > 0 && newp != oldp;
                        sum += (u ? s : 0) - (int)vp9_cost_zero(DIFF_UPDATE_PROB);
                        *updates += u;
                    }
    *savings = sum;
    return *updates == 0 ? X_NO_ENTRY : sum < 0 ? X_NEGATIVE : X_SENT;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2 || hdr[0] != 0x44505543) return 4;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 5;
    VP9_COMP   *cpi = calloc(1, sizeof *cpi);
    VP9_COMMON *cm = &cpi->common;
    if (!cpi) return 6;
    cm->fc = calloc(1, sizeof *cm->fc);
    cpi->td.counts = calloc(1, sizeof *cpi->td.counts);
    if (!cm->fc || !cpi->td.counts) return 6;
    if (sizeof cpi->td.rd_counts.coef_counts != 6912 * 4 || sizeof cm->counts.eob_branch != 576 * 4 || sizeof cm->fc->coef_probs != 1728) return 7;
    eb_vp9_entropy_mv_init();
    uint32_t cov = 0;
    for (int k = 0; k < hdr[1]; k++) {
        int32_t  fr[4];
        uint32_t tx_totals[4];
        uint8_t  old[1728];
        eb_vp9_init_mode_probs(cm->fc);
        eb_vp9_init_mv_probs(cm);
        memset(cpi->td.counts, 0, sizeof *cpi->td.counts);
        memset(&cm->counts, 0, sizeof cm->counts);
        if (fread(fr, 4, 4, f) != 4 || fread(tx_totals, 4, 4, f) != 4 || fread(cpi->td.rd_counts.coef_counts, 4, 6912, f) != 6912 ||
            fread(cm->counts.eob_branch, 4, 576, f) != 576 || fread(old, 1, 1728, f) != 1728)
            return 8;
        memcpy(cm->fc->coef_probs, old, 1728);
        for (int t = 0; t < 4; t++) cpi->td.counts->tx.tx_totals[t] = tx_totals[t];
        cm->profile = PROFILE_0; cm->bit_depth = VPX_BITS_8; cm->tx_mode = ALLOW_32X32; cm->seg.enabled = 0;
        cm->frame_type = fr[0] ? INTER_FRAME : KEY_FRAME; cm->intra_only = 0; cm->show_frame = 1;
        cm->reference_mode = (REFERENCE_MODE)fr[1]; cpi->allow_comp_inter_inter = fr[2]; cm->allow_high_precision_mv = fr[3];
        cpi->sf.use_fast_coef_updates = TWO_LOOP;
        cpi->sf.coeff_prob_appx_step = 1;
        cpi->sf.tx_size_search_method = USE_FULL_RD;
        int32_t exits[4], updates[4];
        int64_t savings[4];
        for (int t = 0; t < 4; t++) {
            exits[t] = classify(cpi, (TX_SIZE)t, &updates[t], &savings[t]);
            cov |= 1u << exits[t];
        }
        uint8_t *data = calloc(1, 1 << 16);
        memset(data, 0xEE, 1 << 16);
        const uint32_t size = (uint32_t)write_compressed_header(cpi, data);
        const uint8_t *now = (const uint8_t *)cm->fc->coef_probs;
        for (int i = 0; i < 1728; i++)
            if (now[i] != old[i]) {
                const int d = remap_prob(now[i], old[i]);
                cov |= 1u << (d < 16 ? V_SUBEXP_16 : d < 32 ? V_SUBEXP_32 : d < 64 ? V_SUBEXP_64 : d - 64 < (1 << 8) - 191 ? V_UNIFORM_SHORT : V_UNIFORM_LONG);
                cov |= 1u << (now[i] > old[i] ? V_NEWP_ABOVE : V_NEWP_BELOW);
                if (exits[i / 432] != X_SENT) return 9; /* a probability moved in a size the dry run did not send */
            }
        fwrite(&size, 4, 1, out);
        fwrite(data, 1, size, out);
        fwrite(now, 1, 1728, out);
        fwrite(exits, 4, 4, out);
        fwrite(updates, 4, 4, out);
        fwrite(savings, 8, 4, out);
        free(data);
    }
    fwrite(eb_vp9_prob_cost, 2, 256, out);
    static uint8_t remap[255 * 255], bits[255 * 255];
    for (int n = 1; n <= 255; n++)
        for (int o = 1; o <= 255; o++)
            if (n != o) {
                remap[(n - 1) * 255 + o - 1] = (uint8_t)remap_prob(n, o);
                bits[(n - 1) * 255 + o - 1] = (uint8_t)(prob_diff_update_cost((vpx_prob)n, (vpx_prob)o) >> VP9_PROB_COST_SHIFT);
            }
    fwrite(remap, 1, sizeof remap, out);
    fwrite(bits, 1, sizeof bits, out);
    fwrite(&cov, 4, 1, out);
    fclose(f);
    fclose(out);
    return 0;
}

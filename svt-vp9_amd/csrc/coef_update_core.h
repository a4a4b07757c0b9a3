/*
 * coef_update_core.h -- the rules of the forward coefficient-probability update, written once as plain inline functions that compile
 * both for the device (csrc/coef_update.hip) and for the host (host/coef_update_host.c), like boolcode_core.h.
 *
 * Replaces update_coef_probs (VPX/vp9_bitstream.c:669-687) with the counts the reference never fills: build_tree_distribution
 * (:511-531), the TWO_LOOP form of update_coef_probs_common (:542-612) and the two savings searches and the sub-exponential code of
 * VPX/vp9_subexp.c, as bool records in front of the bool coder.
 *
 *   svt_cu_node0_coded   does a token record code node 0?  eob_branch[row] counts the records that do.  The predecessor test is
 *                        svt_bool_skip0 over the picture's stream scanned as ONE run: a block's last token is EOB, or the token of
 *                        its last position and then not ZERO (eob is behind a non-zero coefficient), so the record in front of a
 *                        block's first record never is ZERO and block boundaries change nothing; besides, a block's first record has
 *                        band 0, where node 0 is always coded.
 *   svt_cu_entry         entry e (< 396) of a transform size, in the reference's loop order: its row inside the size and its node
 *   svt_cu_branch        branch counts of a row through eb_vp9_coef_tree (VPX/vp9_tokenize.c:57-69), node 0's second count from eob_branch
 *   svt_cu_binary_prob   get_binary_prob (VPX/prob.h:50-65)
 *   svt_cu_remap         remap_prob (VPX/vp9_subexp.c:42-69); its 254-entry table by the rule that generated it (split_index, modulus 13)
 *   svt_cu_update_bits   update_bits[delp] (:20-30) = the bools encode_term_subexp writes
 *   svt_cu_search        eb_vp9_prob_diff_update_savings_search (:109-130) for nodes 0 and 1, .._search_model (:132-171) with stepsize 1
 *                        over pareto[newp - 1] for node 2
 *   svt_cu_send          the TWO_LOOP exit: something updates and the summed savings are not negative
 *   svt_cu_emit          vpx_write(u, 252) and eb_vp9_write_prob_diff_update as bool records, 12 at most
 *
 * Arithmetic is 64-bit.  The reference sums count * cost in 32 bits (cost_branch256, VPX/vp9_cost.h:34-37, an unsigned product put into
 * an int), which wraps once a branch count passes about 2^31 / 4096; the sums here are the true ones, and the two agree wherever the
 * reference does not wrap.  Counts themselves are 32-bit and are added and subtracted as the reference adds and subtracts them.
 *
 * The only table in memory is the probability cost (eb_vp9_prob_cost, generated into host/vp9_cost_table.inc); the kernels keep a copy
 * in LDS.  cost[0] is never read: probabilities are 1 .. 255.
 */
#ifndef SVT_COEF_UPDATE_CORE_H
#define SVT_COEF_UPDATE_CORE_H

#include <stdint.h>
#include "boolcode_core.h"

#define SVT_CU_UPD_PROB 252      /* DIFF_UPDATE_PROB */
#define SVT_CU_MIN_DELP_BITS 5
#define SVT_CU_COST_SHIFT 9      /* VP9_PROB_COST_SHIFT: costs are in 1/512 bit */
#define SVT_CU_TX_TOTAL_MIN 20   /* a size with tx_totals <= 20 is not searched (VPX/vp9_bitstream.c:679) */

/* an entry of the old table: probabilities are 1 .. 255; a 0 (no table a writer produces holds one) is read as 1, so that no index leaves
 * the cost and pareto tables */
SVT_HD int svt_cu_old(uint8_t p) { return p ? p : 1; }
SVT_HD int svt_cu_node0_coded(uint32_t rec, int has_prev, uint32_t prev) { return !svt_bool_skip0(rec, has_prev, prev); }

/* entry e of a transform size: i (plane type), j (reference type), k (band), l (context < BAND_COEFF_CONTEXTS(k)), t (node) nested in this
 * order; returns the row inside the size, ((i * 2 + j) * 6 + k) * 6 + l */
SVT_HD int svt_cu_entry(int e, int *node) {
    const int ij = e / 99, rr = (e % 99) / 3;
    *node = e % 3;
    return rr < 3 ? ij * 36 + rr : ij * 36 + 6 + (rr - 3);
}
/* the blocks tokenised at a size: eob_branch over its band 0 */
SVT_HD uint32_t svt_cu_tx_total(const uint32_t *eob144) {
    uint32_t n = 0;
    for (int ij = 0; ij < 4; ij++)
        for (int l = 0; l < 6; l++) n += eob144[ij * 36 + l];
    return n;
}

/* ct[2 * n], ct[2 * n + 1]: the two counts of node n (0 .. 10) from the 12 token counts of a row (token 11 = EOB) */
SVT_HD void svt_cu_branch(const uint32_t *c, uint32_t eob_branch, uint32_t *ct) {
    const uint32_t c34 = c[3] + c[4], c56 = c[5] + c[6], c78 = c[7] + c[8], c9a = c[9] + c[10];
    const uint32_t low = c[2] + c34, high = c56 + c78 + c9a;
    ct[0] = c[11];       ct[1] = eob_branch - c[11]; /* (VPX/vp9_bitstream.c:523) */
    ct[2] = c[0];        ct[3] = c[1] + low + high;
    ct[4] = c[1];        ct[5] = low + high;
    ct[6] = low;         ct[7] = high;
    ct[8] = c[2];        ct[9] = c34;
    ct[10] = c[3];       ct[11] = c[4];
    ct[12] = c56;        ct[13] = c78 + c9a;
    ct[14] = c[5];       ct[15] = c[6];
    ct[16] = c78;        ct[17] = c9a;
    ct[18] = c[7];       ct[19] = c[8];
    ct[20] = c[9];       ct[21] = c[10];
}

SVT_HD int svt_cu_binary_prob(uint32_t n0, uint32_t n1) {
    const uint32_t den = n0 + n1;
    if (den == 0) return 128;
    const uint64_t p = ((uint64_t)n0 * 256 + (den >> 1)) / den;
    return p > 255 ? 255 : p < 1 ? 1 : (int)p;
}

SVT_HD int svt_cu_recenter(int v, int m) { return v > (m << 1) ? v : v >= m ? (v - m) << 1 : ((m - v) << 1) - 1; }
/* split_index(i, 254, 13): every 13th index from 6 on goes to the front (20 of them), the others follow in order */
SVT_HD int svt_cu_split_index(int i) { return i % 13 == 6 ? i / 13 : 20 + i - (i + 7) / 13; }
/* newp != oldp, both 1 .. 255; 0 .. 253 */
SVT_HD int svt_cu_remap(int newp, int oldp) {
    const int v = newp - 1, m = oldp - 1;
    return svt_cu_split_index(((m << 1) <= 255 ? svt_cu_recenter(v, m) : svt_cu_recenter(254 - v, 254 - m)) - 1);
}
/* the reader's side (inv_remap_prob of a decoder): the probability whose update from oldp carries remap index delp (0 .. 253) */
SVT_HD int svt_cu_inv_recenter(int v, int m) { return v > (m << 1) ? v : (v & 1) ? m - ((v + 1) >> 1) : m + (v >> 1); }
SVT_HD int svt_cu_inv_remap(int delp, int oldp) {
    int j = 0;
    while (j < 253 && svt_cu_split_index(j) != delp) j++;
    const int v = j + 1, m = oldp - 1;
    return (m << 1) <= 255 ? 1 + svt_cu_inv_recenter(v, m) : 255 - svt_cu_inv_recenter(v, 254 - m);
}
SVT_HD int svt_cu_update_bits(int delp) { return delp < 16 ? 5 : delp < 32 ? 6 : delp < 64 ? 8 : delp < 129 ? 10 : 11; }

SVT_HD int64_t svt_cu_cost_branch(uint32_t n0, uint32_t n1, int p, const uint16_t *cost) {
    return (int64_t)n0 * cost[p] + (int64_t)n1 * cost[256 - p];
}
/* cost of the counts of nodes 2 .. 10 when node 2 has probability p and the nodes behind it pareto[p - 1] */
SVT_HD int64_t svt_cu_cost_model(const uint32_t *ct, int p, const uint16_t *cost, const uint8_t (*pareto)[8]) {
    int64_t b = svt_cu_cost_branch(ct[4], ct[5], p, cost);
#if defined(__HIPCC__)
    _Pragma("unroll")
#endif
    for (int i = 0; i < 8; i++) b += svt_cu_cost_branch(ct[6 + 2 * i], ct[7 + 2 * i], pareto[p - 1][i], cost);
    return b;
}
SVT_HD int64_t svt_cu_upd_cost(const uint16_t *cost) { return (int64_t)cost[256 - SVT_CU_UPD_PROB] - cost[SVT_CU_UPD_PROB]; }

/* the savings search of one entry: ct = all 22 branch counts of the row; *newp = the candidate on entry, the best probability on return
 * (oldp when nothing saves); returns the savings in 1/512 bit.  Candidates run from *newp towards oldp, the first of equals wins. */
SVT_HD int64_t svt_cu_search(const uint32_t *ct, int node, int oldp, int *newp, const uint16_t *cost, const uint8_t (*pareto)[8]) {
    const int     step = *newp > oldp ? -1 : 1;
    const int64_t upd = svt_cu_upd_cost(cost);
    const uint32_t n0 = node == 0 ? ct[0] : ct[2], n1 = node == 0 ? ct[1] : ct[3]; /* (constant indices: ct stays in registers on the device) */
    const int64_t old_b = node == 2 ? svt_cu_cost_model(ct, oldp, cost, pareto) : svt_cu_cost_branch(n0, n1, oldp, cost);
    int64_t       best = 0;
    int           bestp = oldp;
    if (old_b > upd + (SVT_CU_MIN_DELP_BITS << SVT_CU_COST_SHIFT))
        for (int p = *newp; p != oldp; p += step) {
            const int64_t new_b = node == 2 ? svt_cu_cost_model(ct, p, cost, pareto) : svt_cu_cost_branch(n0, n1, p, cost);
            const int64_t s = old_b - new_b - ((int64_t)svt_cu_update_bits(svt_cu_remap(p, oldp)) << SVT_CU_COST_SHIFT) - upd;
            if (s > best) { best = s; bestp = p; }
        }
    *newp = bestp;
    return best;
}

/* one entry of the dry run: u = it updates; what it adds to the size's savings */
SVT_HD int64_t svt_cu_entry_savings(int u, int64_t s, const uint16_t *cost) { return (u ? s : 0) - (int64_t)cost[SVT_CU_UPD_PROB]; }
SVT_HD int     svt_cu_send(uint32_t updates, int64_t savings) { return updates != 0 && savings >= 0; }

/* records an entry of a size that is sent writes */
SVT_HD int svt_cu_entry_records(int u, int newp, int oldp) { return 1 + (u ? svt_cu_update_bits(svt_cu_remap(newp, oldp)) : 0); }

SVT_HD int svt_cu_literal(uint16_t *out, int n, int v, int bits) {
    while (bits--) out[n++] = SVT_BOOL_RECORD((v >> bits) & 1, 128);
    return n;
}
/* the flag at 252 and, for an update, encode_term_subexp(remap) (VPX/vp9_subexp.c:76-102) as literal bits; returns svt_cu_entry_records */
SVT_HD int svt_cu_emit(int u, int newp, int oldp, uint16_t *out) {
    int n = 0;
    out[n++] = SVT_BOOL_RECORD(u ? 1 : 0, SVT_CU_UPD_PROB);
    if (!u) return n;
    const int w = svt_cu_remap(newp, oldp);
    n = svt_cu_literal(out, n, w >= 16, 1);
    if (w < 16) return svt_cu_literal(out, n, w, 4);
    n = svt_cu_literal(out, n, w >= 32, 1);
    if (w < 32) return svt_cu_literal(out, n, w - 16, 4);
    n = svt_cu_literal(out, n, w >= 64, 1);
    if (w < 64) return svt_cu_literal(out, n, w - 32, 5);
    const int v = w - 64, m = 65; /* encode_uniform: l = 8, m = (1 << l) - 191 */
    if (v < m) return svt_cu_literal(out, n, v, 7);
    n = svt_cu_literal(out, n, m + ((v - m) >> 1), 7);
    return svt_cu_literal(out, n, (v - m) & 1, 1);
}

/* everything of one entry: from the row's 12 token counts, its eob_branch and the old probabilities.  Returns u; *s = the search's savings */
SVT_HD int svt_cu_entry_decide(const uint32_t *counts12, uint32_t eob_branch, int node, int oldp, const uint16_t *cost, const uint8_t (*pareto)[8],
                               int *newp, int64_t *s) {
    uint32_t ct[22];
    svt_cu_branch(counts12, eob_branch, ct);
    int p = node == 0 ? svt_cu_binary_prob(ct[0], ct[1]) : node == 1 ? svt_cu_binary_prob(ct[2], ct[3]) : svt_cu_binary_prob(ct[4], ct[5]);
    *s = svt_cu_search(ct, node, oldp, &p, cost, pareto);
    *newp = p;
    return *s > 0 && p != oldp;
}

#endif /* SVT_COEF_UPDATE_CORE_H */

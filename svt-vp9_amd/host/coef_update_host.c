/*
 * coef_update_host.c -- host-side (plain C) half of the forward coefficient-probability update (csrc/coef_update.hip):
 *   - svt_hip_coef_update_picture: the rules of csrc/coef_update_core.h (the same inline text the kernels call) walked serially in the
 *     reference's order -- the model of the kernels on machines without a device, and what tests/gen_golden_coef_update.py holds
 *     against the reference's write_compressed_header;
 *   - the probability-cost table (host/vp9_cost_table.inc), the capacity, the validation the device entry shares, and the remap /
 *     update-bits rules tabulated for the tests.
 */
#include <string.h>
#include "../../include/svtvp9_hip.h"
#include "../csrc/coef_update_core.h"
#include "vp9_cost_table.inc"

const uint16_t *svt_hip_coef_update_cost_table(void) { return k_vp9_prob_cost; }

uint32_t svt_hip_coef_update_bools_capacity(void) { return SVT_CU_PREFIX_MAX + SVT_CU_SECTION_MAX + SVT_CU_SUFFIX_MAX; }

void svt_hip_coef_update_remap_tables(uint8_t *remap, uint8_t *bits) {
    for (int n = 1; n <= 255; n++)
        for (int o = 1; o <= 255; o++) {
            const int at = (n - 1) * 255 + o - 1, d = n == o ? 0 : svt_cu_remap(n, o);
            if (remap) remap[at] = (uint8_t)d;
            if (bits) bits[at] = n == o ? 0 : (uint8_t)svt_cu_update_bits(d);
        }
}

/* 0: the descriptor is one both forms take */
int32_t svt_cu_check_picture(const svt_cu_picture *p) {
    if (!p->d_counts || !p->d_eob_branch || !p->d_probs || !p->d_hdr_bools || !p->d_n_hdr_bools || !p->d_segment || !p->d_result) return SVT_HIP_ERR_BAD_PARAMETER;
    if (!p->d_tokens && p->max_tokens) return SVT_HIP_ERR_BAD_PARAMETER;
    if (p->n_prefix > SVT_CU_PREFIX_MAX || p->n_suffix > SVT_CU_SUFFIX_MAX) return SVT_HIP_ERR_BAD_PARAMETER;
    return SVT_HIP_OK;
}

int32_t svt_hip_coef_update_picture(const svt_cu_picture *pic, const svt_bool_tables *tables) {
    if (!pic || !tables || svt_cu_check_picture(pic)) return SVT_HIP_ERR_BAD_PARAMETER;
    const uint8_t *old = pic->d_old_probs ? pic->d_old_probs : tables->coef_probs;
    uint32_t       n_tok = pic->d_n_tokens ? *pic->d_n_tokens : pic->n_tokens;
    if (n_tok > pic->max_tokens) n_tok = pic->max_tokens;
    uint32_t *eob = pic->d_eob_branch;
    memset(eob, 0, sizeof(uint32_t) * SVT_CU_ROWS);
    for (uint32_t i = 0; i < n_tok; i++) {
        const uint32_t rec = pic->d_tokens[i], row = SVT_TOK_PROB_ROW(rec);
        if (row < SVT_CU_ROWS && svt_cu_node0_coded(rec, i > 0, i > 0 ? pic->d_tokens[i - 1] : 0u)) eob[row]++;
    }
    svt_cu_result res;
    memset(&res, 0, sizeof res);
    res.tokens = n_tok;
    uint8_t probs[SVT_CU_PROBS];
    memcpy(probs, old, SVT_CU_PROBS);
    uint16_t *out = pic->d_hdr_bools;
    uint32_t  n = 0;
    for (uint32_t k = 0; k < pic->n_prefix; k++) out[n++] = pic->prefix[k];
    for (int t = 0; t < 4; t++) {
        if (svt_cu_tx_total(eob + 144 * t) <= SVT_CU_TX_TOTAL_MIN) { out[n++] = SVT_BOOL_RECORD(0, 128); continue; }
        int      u[SVT_CU_ENTRIES], newp[SVT_CU_ENTRIES];
        int64_t  savings = 0;
        uint32_t updates = 0;
        for (int e = 0; e < SVT_CU_ENTRIES; e++) {
            int       node;
            const int row = 144 * t + svt_cu_entry(e, &node);
            int64_t   s;
            u[e] = svt_cu_entry_decide(pic->d_counts + 12 * row, eob[row], node, svt_cu_old(old[3 * row + node]), k_vp9_prob_cost, tables->pareto, &newp[e], &s);
            savings += svt_cu_entry_savings(u[e], s, k_vp9_prob_cost);
            updates += (uint32_t)u[e];
        }
        res.updated[t] = updates;
        res.savings[t] = savings;
        res.sent[t] = (uint32_t)svt_cu_send(updates, savings);
        out[n++] = SVT_BOOL_RECORD(res.sent[t], 128);
        if (!res.sent[t]) continue;
        for (int e = 0; e < SVT_CU_ENTRIES; e++) {
            int       node;
            const int row = 144 * t + svt_cu_entry(e, &node);
            n += (uint32_t)svt_cu_emit(u[e], newp[e], svt_cu_old(old[3 * row + node]), out + n);
            if (u[e]) probs[3 * row + node] = (uint8_t)newp[e];
        }
    }
    for (uint32_t k = 0; k < pic->n_suffix; k++) out[n++] = pic->suffix[k];
    res.hdr_bools = n;
    memcpy(pic->d_probs, probs, SVT_CU_PROBS);
    *pic->d_n_hdr_bools = n;
    pic->d_segment->first = 0; pic->d_segment->count = n; pic->d_segment->kind = 1;
    *pic->d_result = res;
    return SVT_HIP_OK;
}

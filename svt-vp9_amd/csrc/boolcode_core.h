/*
 * boolcode_core.h -- the rules of the bool coder, written once as plain inline functions that compile both for the device
 * (csrc/boolcode.hip) and for the host (host/boolcode_host.c), like tokenize_core.h.
 *
 *   svt_bool_skip0   is node 0 of a token record left out?  (pack_mb_tokens stays inside its ZERO loop, VPX/vp9_bitstream.c:116-123)
 *   svt_bool_count   bools of a token record: a function of (token, node 0 left out) alone, which makes every bool offset a scan
 *   svt_bool_expand  the bools themselves, in pack_mb_tokens' order (VPX/vp9_bitstream.c:110-160)
 *   svt_bool_step    one vpx_write (VPX/bitwriter.h:34-84) as far as the range is concerned: split, shift, next range
 *
 * The coder's output as one integer: with r_0 = 255, S_i the shifts summed up to and including symbol i, P_i = S_(i-1), S the total,
 * V = sum over the 1-bools of split_i << (S - P_i) has S + 8 bits.  Counted from its top bit, split_i occupies the bits
 * [P_i, P_i + 8), and the output is the first (S - 16) / 8 bytes from the top: positions do not depend on S.
 */
#ifndef SVT_BOOLCODE_CORE_H
#define SVT_BOOLCODE_CORE_H

#include <stdint.h>
#include "tokenize_core.h"

#define SVT_BOOL_FRAME_TAIL 32 /* eb_vp9_stop_encode's (128, 0) bools; eb_vp9_start_encode adds one in front */
/* bytes n bools occupy at most: 7 bits a bool, the framing bools, the marker byte (svt_hip_boolcode_capacity; n of a type wide enough) */
#define SVT_BOOL_CAPACITY_OF(n) ((7 * ((n) + 1 + SVT_BOOL_FRAME_TAIL) + 7) / 8 + 2)
/* eb_vp9_coef_con_tree (VPX/vp9_entropy.c), inner links only, one nibble per entry: {2, 6, -, 4, -, -, 8, 10, -, -, 12, 14, -, -, -, -} */
#define SVT_BOOL_CON_TREE 0x0000EC00A8004062ull

SVT_HD int svt_bool_band(uint32_t rec) { return (int)(SVT_TOK_PROB_ROW(rec) / 6) % 6; }
SVT_HD int svt_bool_skip0(uint32_t rec, int has_prev, uint32_t prev) { return has_prev && SVT_TOK_TOKEN(prev) == 0 && svt_bool_band(rec) != 0; }
/* length and value of the token's path through the constrained tree: eb_vp9_coef_encodings[t] without its three unconstrained nodes */
SVT_HD int svt_bool_tree_len(int tok) { return tok == 2 ? 2 : tok < 7 ? 3 : 4; }
SVT_HD int svt_bool_tree_value(int tok) { return tok == 2 ? 0 : tok < 7 ? tok - 1 : tok + 5; }
/* eb_vp9_extra_bits[t].len at 8-bit depth */
SVT_HD int svt_bool_cat_bits(int tok) { return tok < 5 ? 0 : tok < 10 ? tok - 4 : 14; }

SVT_HD int svt_bool_count(int tok, int skip0) {
    const int head = skip0 ? 0 : 1;
    if (tok >= SVT_TOK_EOB) return 1;
    if (tok == 0) return head + 1;
    if (tok == 1) return head + 3;
    return head + 2 + svt_bool_tree_len(tok) + svt_bool_cat_bits(tok) + 1;
}

/* writes svt_bool_count(token, skip0) records to out; coef_probs: the 576 x 3 coefficient probabilities of the stream (t's own, or
 * another picture's: svt_hip_boolcode_batch_tables_device), pareto and cat_probs are t's */
SVT_HD int svt_bool_expand_probs(uint32_t rec, int skip0, const uint8_t *coef_probs, const svt_bool_tables *t, uint16_t *out) {
    const int      tok = (int)SVT_TOK_TOKEN(rec);
    const uint32_t e = SVT_TOK_EXTRA(rec), row = SVT_TOK_PROB_ROW(rec) < 576 ? SVT_TOK_PROB_ROW(rec) : 575;
    const uint8_t *p = coef_probs + 3 * row;
    int            n = 0;
    if (tok >= SVT_TOK_EOB) { out[0] = SVT_BOOL_RECORD(0, p[0]); return 1; }
    if (!skip0) out[n++] = SVT_BOOL_RECORD(1, p[0]);
    if (tok == 0) { out[n++] = SVT_BOOL_RECORD(0, p[1]); return n; }
    out[n++] = SVT_BOOL_RECORD(1, p[1]);
    if (tok == 1) {
        out[n++] = SVT_BOOL_RECORD(0, p[2]);
        out[n++] = SVT_BOOL_RECORD(e & 1, 128);
        return n;
    }
    out[n++] = SVT_BOOL_RECORD(1, p[2]);
    const uint8_t *par = t->pareto[p[2] ? p[2] - 1 : 0];
    int            len = svt_bool_tree_len(tok), i = 0;
    const int      v = svt_bool_tree_value(tok);
    do {
        const int bit = (v >> --len) & 1;
        out[n++] = SVT_BOOL_RECORD(bit, par[i >> 1]);
        i = (int)(SVT_BOOL_CON_TREE >> (4 * (i + bit))) & 15;
    } while (len);
    const uint8_t *cat = t->cat_probs[tok >= 5 ? tok - 5 : 0];
    for (int k = svt_bool_cat_bits(tok), j = 0; k > 0; j++) out[n++] = SVT_BOOL_RECORD((e >> 1 >> --k) & 1, cat[j]);
    out[n++] = SVT_BOOL_RECORD(e & 1, 128);
    return n;
}
SVT_HD int svt_bool_expand(uint32_t rec, int skip0, const svt_bool_tables *t, uint16_t *out) { return svt_bool_expand_probs(rec, skip0, t->coef_probs, t, out); }

/* one symbol from range r (128 .. 255): *split is what a 1 adds to the low end; returns next range | shift << 8 */
SVT_HD uint32_t svt_bool_step(uint32_t r, uint32_t rec, uint32_t *split) {
    const uint32_t s = 1 + (((r - 1) * (rec & 255u)) >> 8), x = (rec >> 8) & 1u ? r - s : s;
    const uint32_t shift = (uint32_t)__builtin_clz(x) - 24u;
    *split = s;
    return (x << shift) | shift << 8;
}

#endif /* SVT_BOOLCODE_CORE_H */

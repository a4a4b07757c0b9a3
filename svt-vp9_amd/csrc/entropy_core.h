/*
 * entropy_core.h -- the rules of the entropy pass (csrc/entropy.hip, host/entropy_host.c), written once as plain inline functions that
 * compile both for the device and for the host, like the other *_core.h files.
 *
 *   svt_ent_layout      where every intermediate of a picture lies in the workspace's slab, from the geometry and the limits
 *   svt_ent_verdict_a   the gate in front of the bool coder: may the picture's segment list be handed to it
 *   svt_ent_verdict_b   the gate behind it: is the tile one the caller's budgets hold
 *   svt_ent_result_of   the record the caller reads
 *
 * Why a gate.  The tokeniser and the mode-info stages write nothing beyond the capacities they are given, but their offsets -- and so the
 * segment list -- describe the whole stream, and the bool coder reads tokens[first + k] and bools[first + k] straight from the segments.
 * With buffers smaller than the worst case a picture that exceeds them would make it read past them.  A picture whose verdict is not 0
 * gets an empty segment list: the bool coder then codes the empty stream and touches neither tokens nor bools.  With a verdict of 0
 * every token segment lies below the tokeniser's total <= max_tokens and every bool segment below the stage's total <= its capacity.
 */
#ifndef SVT_ENTROPY_CORE_H
#define SVT_ENTROPY_CORE_H

#include <stdint.h>
#include "frame_core.h"

/* byte offsets inside a picture's part of the slab; every one a multiple of 16 */
typedef struct svt_ent_layout {
    uint64_t tok_off, sb_off, tokens, ext, bools, segments, tile, words, bytes; /* bytes: a picture's part */
    uint32_t n_segments, kf_bools, inter_bools;
    int32_t  n_sb;
} svt_ent_layout;
/* the dwords of `words`: the labelling's status, the mode-info total, the tile's size, the gate's verdict */
enum { SVT_ENT_W_STATUS = 0, SVT_ENT_W_N_BOOLS = 4, SVT_ENT_W_SIZE = 5, SVT_ENT_W_VERDICT = 6, SVT_ENT_WORDS = 16 };

SVT_HD uint64_t svt_ent_align16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

/* 0 and the layout; 1 for a geometry the grid stages do not take */
SVT_HD int svt_ent_layout_of(int width, int height, int mi_stride, uint32_t max_tokens, uint32_t max_tile_bytes, svt_ent_layout *l) {
    svt_tok_geom g;
    int          sb_cols, n_sb;
    if (svt_tok_geom_of(width, height, mi_stride, &g, &sb_cols, &n_sb)) return 1;
    const uint64_t units = (uint64_t)g.mi_rows * (uint64_t)g.mi_cols;
    l->n_sb = n_sb;
    l->n_segments = (uint32_t)n_sb * 256u;       /* svt_hip_modes_segments */
    l->kf_bools = (uint32_t)units * 48u;         /* svt_hip_modes_bools_capacity */
    l->inter_bools = (uint32_t)units * 111u;     /* svt_hip_modes_inter_bools_capacity */
    uint64_t at = 0;
    l->tok_off = at;  at += svt_ent_align16(4 * ((uint64_t)g.w4 * g.h4 * 3 / 2));
    l->sb_off = at;   at += svt_ent_align16(4 * ((uint64_t)n_sb + 1));
    l->tokens = at;   at += svt_ent_align16(4 * (uint64_t)max_tokens);
    l->ext = at;      at += svt_ent_align16(12 * (uint64_t)g.mi_rows * (uint64_t)g.mi_stride);
    l->bools = at;    at += svt_ent_align16(2 * (uint64_t)l->inter_bools);
    l->segments = at; at += svt_ent_align16(12 * (uint64_t)l->n_segments);
    l->tile = at;     at += svt_ent_align16(max_tile_bytes);
    l->words = at;    at += 4 * SVT_ENT_WORDS;
    l->bytes = at;
    return 0;
}

/* The second slab of a workspace, taken when the coefficient-update mode is first enabled: per picture what the update stage
 * (csrc/coef_update.hip) reads and writes and the compressed header's stream.  The header stream cannot overflow: it holds at most
 * SVT_ENT_HDR_BOOLS records whatever the picture, its buffer is the bool coder's capacity for that many, and that capacity is a
 * first_part_size 16 bits can say -- so a picture's header never withholds it and the result record needs no flag for it. */
#define SVT_ENT_HDR_BOOLS (SVT_CU_PREFIX_MAX + SVT_CU_SECTION_MAX + SVT_CU_SUFFIX_MAX)              /* svt_hip_coef_update_bools_capacity */
#define SVT_ENT_HDR_BYTES SVT_BOOL_CAPACITY_OF(SVT_ENT_HDR_BOOLS)                                    /* svt_hip_boolcode_capacity of it: the same macro */
#if SVT_ENT_HDR_BYTES > 0xFFFF
#error "a compressed header with coefficient updates may exceed first_part_size"
#endif
typedef struct svt_ent_coef_layout {
    uint64_t counts, eob_branch, probs, hdr_bools, hdr_bytes, result, words, bytes; /* byte offsets, multiples of 16; bytes: a picture's part */
} svt_ent_coef_layout;
/* the dwords of its `words`: the header's record count, its one segment {first, count, kind}, the coded header's size */
enum { SVT_ENT_CW_N_HDR_BOOLS = 0, SVT_ENT_CW_SEGMENT = 1, SVT_ENT_CW_HDR_SIZE = 4, SVT_ENT_CW_WORDS = 16 };

SVT_HD void svt_ent_coef_layout_of(svt_ent_coef_layout *l) {
    uint64_t at = 0;
    l->counts = at;     at += svt_ent_align16(4 * (uint64_t)SVT_TOK_COUNTS);
    l->eob_branch = at; at += svt_ent_align16(4 * (uint64_t)SVT_CU_ROWS);
    l->probs = at;      at += svt_ent_align16(SVT_CU_PROBS);
    l->hdr_bools = at;  at += svt_ent_align16(2 * (uint64_t)SVT_ENT_HDR_BOOLS);
    l->hdr_bytes = at;  at += svt_ent_align16(SVT_ENT_HDR_BYTES);
    l->result = at;     at += svt_ent_align16(sizeof(svt_cu_result));
    l->words = at;      at += 4 * SVT_ENT_CW_WORDS;
    l->bytes = at;
}

/* the bool coder's own rule for a stream it takes: bit positions are 32-bit */
SVT_HD int svt_ent_bools_codable(uint32_t max_bools) { return 7ull * ((uint64_t)max_bools + 1 + SVT_BOOL_FRAME_TAIL) < 0x100000000ull; }

/* the labelling's four status words by value (a pointer to them would put them into scratch memory on the device); labelled 0: a picture
 * without inter blocks (key frame, intra-only), the words are not looked at */
typedef struct svt_ent_status {
    uint32_t s0, s1, s2, s3;
    int      labelled;
} svt_ent_status;
SVT_HD svt_ent_status svt_ent_status_of(const uint32_t *status) {
    svt_ent_status s = {0, 0, 0, 0, 0};
    if (status) { s.s0 = status[0]; s.s1 = status[1]; s.s2 = status[2]; s.s3 = status[3]; s.labelled = 1; }
    return s;
}
SVT_HD int svt_ent_status_bad(svt_ent_status s) {
    return s.s0 == SVT_MODES_BAD_GRID || s.s1 == SVT_MODES_BAD_GRID || s.s2 == SVT_MODES_BAD_GRID || s.s3 == SVT_MODES_BAD_GRID;
}

/* Phase A.  tok_total: the tokeniser's last sb_off entry; n_bools / bools_capacity: the mode-info stage's total and what its buffer
 * holds; s: the labelling's status */
SVT_HD uint32_t svt_ent_verdict_a(uint32_t tok_total, uint32_t max_tokens, uint32_t n_bools, uint32_t bools_capacity, svt_ent_status s) {
    uint32_t f = 0;
    if (tok_total > max_tokens) f |= SVT_ENT_TOKENS_OVER;
    if (n_bools == SVT_MODES_BAD_GRID) f |= SVT_ENT_BAD_GRID;
    else if (n_bools > bools_capacity) f |= SVT_ENT_MODE_BOOLS_OVER;
    if (s.labelled) {
        if (svt_ent_status_bad(s)) f |= SVT_ENT_BAD_GRID;
        else if (s.s2 != 0) f |= SVT_ENT_UNFAITHFUL_MV;
    }
    return f;
}

/* Phase B.  size: what the bool coder left in *d_size.  A picture withheld in phase A keeps its flags: its tile is the empty stream's */
SVT_HD uint32_t svt_ent_verdict_b(uint32_t verdict_a, uint32_t size, uint32_t max_tile_bytes) {
    if (verdict_a) return verdict_a;
    if (size == SVT_BOOL_SIZE_OVERFLOW) return SVT_ENT_STREAM_OVER;
    return size > max_tile_bytes ? SVT_ENT_TILE_OVER : 0u;
}

/* the caller's record; returns what *d_size becomes: the size of a tile that ships, SVT_BOOL_SIZE_OVERFLOW for one that does not (the
 * frame stage then gives the picture SVT_FRAME_SIZE_NONE).  Leaf counts are 0 where the labelling did not run or refused the grid */
SVT_HD uint32_t svt_ent_result_of(uint32_t flags, uint32_t tok_total, uint32_t n_bools, uint32_t size, svt_ent_status s, svt_entropy_result *r) {
    const int counted = s.labelled && !svt_ent_status_bad(s);
    r->flags = flags;
    r->tokens = tok_total;
    r->mode_bools = n_bools;
    r->tile_bytes = flags ? 0u : size;
    r->inter_leaves = counted ? s.s0 : 0u;
    r->newmv_leaves = counted ? s.s1 : 0u;
    r->unfaithful_leaves = counted ? s.s2 : 0u;
    r->pad_ = 0;
    return flags ? SVT_BOOL_SIZE_OVERFLOW : size;
}

/* cm->comp_fixed_ref / comp_var_ref as eb_vp9_setup_compound_reference_mode (VPX/vp9_pred_common.c:26-40) leaves them: the fixed
 * reference is the one whose sign bias stands alone -- ALTREF when LAST and GOLDEN agree, else GOLDEN when LAST and ALTREF agree, else LAST */
SVT_HD void svt_ent_compound_refs(const uint8_t sign_bias[4], uint8_t *fixed, uint8_t var[2]) {
    if (sign_bias[1] == sign_bias[2]) { *fixed = 3; var[0] = 1; var[1] = 2; }
    else if (sign_bias[1] == sign_bias[3]) { *fixed = 2; var[0] = 1; var[1] = 3; }
    else { *fixed = 1; var[0] = 2; var[1] = 3; }
}

SVT_HD int svt_ent_intra_only(const svt_frame_params *p) { return p->frame_type == 0 || p->intra_only != 0; }

#endif /* SVT_ENTROPY_CORE_H */

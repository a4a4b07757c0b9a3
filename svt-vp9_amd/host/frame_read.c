/*
 * frame_read.c -- the frame reader (plain C, no HIP): the two headers, below them the tile of a key frame or an inter picture
 * (svt_hip_tile_read_host), and both in one call (svt_hip_frame_read_host).  svt_hip_frame_read_header_host parses what
 * svt_hip_frame_header_host / svt_hip_frame_show_existing_host write, the way a DECODER reads it -- read_uncompressed_header and
 * read_compressed_header of the VP9 specification (6.2, 6.3; libvpx vp9_decodeframe.c), not the writer run backwards: where the decoder
 * infers a value instead of reading it (compound prediction allowed from the sign biases, lossless from the quantiser fields, the flags
 * under error_resilient_mode) so does this reader, and a stream whose writer assumed otherwise does not parse back to its parameters.
 * The field order is host/frame_host.c's uncompressed_header / compressed_parts, read instead of written; the bool decoder is
 * csrc/read_core.h's.  The compressed header is decoded bool by bool; a set update flag returns SVT_HIP_ERR_UNSUPPORTED (the plain
 * writers never send a forward update, include/svtvp9_hip.h: the no-update rule) -- except that svt_hip_frame_read_header_coef_host reads
 * coefficient-probability updates (the writer is csrc/coef_update.hip's stage) into the caller's table, with the writer's own entry order.
 *
 * Memory safety: no byte at or beyond frame + size is read (both readers are bounded), nothing but *info (and the coefficient probabilities of the coef reader's table) is written, every loop has a
 * constant trip count.
 */
#include <stdio.h>
#include <string.h>
#include "../../include/svtvp9_hip.h"
#include "../csrc/frame_core.h"
#include "../csrc/read_core.h"
#include "../csrc/coef_update_core.h"

int32_t svt_set_error_c(int32_t code, const char *msg); /* csrc/api.hip: the message behind svt_hip_last_error */

static int32_t fail(int32_t code, const char *what) {
    char msg[128];
    snprintf(msg, sizeof msg, "frame_read: %s", what);
    return svt_set_error_c(code, msg);
}

static int read_sync_code(svt_bit_reader *r) { return svt_bit_literal(r, 24) == 0x498342; }

static void read_frame_size(svt_bit_reader *r, svt_frame_params *p) {
    p->width = (int32_t)svt_bit_literal(r, 16) + 1;
    p->height = (int32_t)svt_bit_literal(r, 16) + 1;
    if (svt_bit_read(r)) { /* render_and_frame_size_different */
        p->render_width = (int32_t)svt_bit_literal(r, 16) + 1;
        p->render_height = (int32_t)svt_bit_literal(r, 16) + 1;
    } else { p->render_width = p->width; p->render_height = p->height; }
}
static int read_lf_delta(svt_bit_reader *r, int last) { /* a delta that is not sent keeps the stream's value */
    if (!svt_bit_read(r)) return last;
    const int m = (int)svt_bit_literal(r, 6);
    return svt_bit_read(r) ? -m : m;
}
static int read_delta_q(svt_bit_reader *r) {
    if (!svt_bit_read(r)) return 0;
    const int m = (int)svt_bit_literal(r, 4);
    return svt_bit_read(r) ? -m : m;
}

/* `count` probability updates, each a flag at probability 252 (vp9_diff_update_prob): 0 when none is set */
static int any_update(svt_bool_reader *b, int count) {
    int set = 0;
    for (int k = 0; k < count; k++) set |= svt_bool_read(b, 252);
    return set;
}

/* the inverse of encode_term_subexp / encode_uniform (VPX/vp9_subexp.c:76-102) */
static int read_term_subexp(svt_bool_reader *b) {
    if (!svt_bool_read(b, 128)) return (int)svt_bool_literal(b, 4);
    if (!svt_bool_read(b, 128)) return (int)svt_bool_literal(b, 4) + 16;
    if (!svt_bool_read(b, 128)) return (int)svt_bool_literal(b, 5) + 32;
    const int v = (int)svt_bool_literal(b, 7), m = (1 << 8) - 191;
    return 64 + (v < m ? v : (v << 1) - m + svt_bool_read(b, 128));
}
/* read_coef_probs of one transform size that is updated: the writer's entries in the writer's order (csrc/coef_update_core.h) */
static void read_coef_updates(svt_bool_reader *b, uint8_t *probs432) {
    for (int e = 0; e < SVT_CU_ENTRIES; e++) {
        int       node;
        const int at = 3 * svt_cu_entry(e, &node) + node;
        if (svt_bool_read(b, SVT_CU_UPD_PROB)) probs432[at] = (uint8_t)svt_cu_inv_remap(read_term_subexp(b), probs432[at]);
    }
}

/* both header readers: tables null = a coefficient update is refused, as every other update is */
static int32_t read_header(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2], svt_frame_read_info *info,
                           svt_bool_tables *tables) {
    if (!frame || !info || !last_ref_deltas || !last_mode_deltas) return fail(SVT_HIP_ERR_BAD_PARAMETER, "null argument");
    memset(info, 0, sizeof *info);
    if (size == 0) return fail(SVT_HIP_ERR_BAD_PARAMETER, "empty frame");
    svt_frame_params *p = &info->params;
    svt_bit_reader    r;
    svt_bit_reader_init(&r, frame, size);
    if (svt_bit_literal(&r, 2) != 2) return fail(SVT_HIP_ERR_BAD_PARAMETER, "frame marker");
    const int profile = svt_bit_read(&r) | svt_bit_read(&r) << 1;
    if (profile > 0) return fail(SVT_HIP_ERR_UNSUPPORTED, "profile above 0");
    for (int i = 0; i < 4; i++) { p->last_ref_deltas[i] = last_ref_deltas[i]; p->ref_deltas[i] = last_ref_deltas[i]; }
    for (int i = 0; i < 2; i++) { p->last_mode_deltas[i] = last_mode_deltas[i]; p->mode_deltas[i] = last_mode_deltas[i]; }
    if (svt_bit_read(&r)) { /* show_existing_frame: the slot's three bits end the frame */
        info->show_existing_frame = 1;
        info->show_existing_slot = (uint8_t)svt_bit_literal(&r, 3);
        info->uncompressed_bytes = 1;
        return SVT_HIP_OK; /* (eight bits: the first byte holds them all) */
    }
    p->frame_type = (uint8_t)svt_bit_read(&r);
    p->show_frame = (uint8_t)svt_bit_read(&r);
    p->error_resilient_mode = (uint8_t)svt_bit_read(&r);
    info->interp_filter = SVT_READ_FILTER_REGULAR; /* (pictures without inter blocks carry none) */
    if (p->frame_type == 0) {
        if (!read_sync_code(&r)) return fail(SVT_HIP_ERR_BAD_PARAMETER, "sync code");
        p->color_space = (uint8_t)svt_bit_literal(&r, 3);
        if (p->color_space == 7) return fail(SVT_HIP_ERR_UNSUPPORTED, "sRGB needs profile 1");
        p->color_range = (uint8_t)svt_bit_read(&r);
        p->refresh_frame_mask = 0xFF; /* a key frame refreshes every slot */
        read_frame_size(&r, p);
    } else {
        p->intra_only = p->show_frame ? 0 : (uint8_t)svt_bit_read(&r);
        p->reset_frame_context = p->error_resilient_mode ? 0 : (uint8_t)svt_bit_literal(&r, 2);
        if (p->intra_only) {
            if (!read_sync_code(&r)) return fail(SVT_HIP_ERR_BAD_PARAMETER, "sync code");
            p->refresh_frame_mask = (uint8_t)svt_bit_literal(&r, 8);
            read_frame_size(&r, p);
        } else {
            p->refresh_frame_mask = (uint8_t)svt_bit_literal(&r, 8);
            for (int k = 0; k < 3; k++) {
                p->ref_dpb_index[k] = (uint8_t)svt_bit_literal(&r, 3);
                p->ref_frame_sign_bias[1 + k] = (uint8_t)svt_bit_read(&r);
            }
            for (int k = 0; k < 3; k++)
                if (svt_bit_read(&r)) return fail(SVT_HIP_ERR_UNSUPPORTED, "frame size taken from a reference (found_ref)");
            read_frame_size(&r, p);
            p->allow_hp = (uint8_t)svt_bit_read(&r);
            if (svt_bit_read(&r)) info->interp_filter = SVT_READ_FILTER_SWITCHABLE;
            else {
                /* literal_to_filter of the decoder: { EIGHTTAP_SMOOTH, EIGHTTAP, EIGHTTAP_SHARP, BILINEAR } */
                static const uint8_t literal_to_filter[4] = {SVT_READ_FILTER_SMOOTH, SVT_READ_FILTER_REGULAR, SVT_READ_FILTER_SHARP, SVT_READ_FILTER_BILINEAR};
                info->interp_filter = literal_to_filter[svt_bit_literal(&r, 2)];
            }
            /* setup_compound_reference_mode's condition: compound prediction exists when the sign biases differ */
            p->allow_comp_inter_inter = p->ref_frame_sign_bias[2] != p->ref_frame_sign_bias[1] || p->ref_frame_sign_bias[3] != p->ref_frame_sign_bias[1];
        }
    }
    if (!p->error_resilient_mode) {
        p->refresh_frame_context = (uint8_t)svt_bit_read(&r);
        p->frame_parallel_decoding_mode = (uint8_t)svt_bit_read(&r);
    } else { p->refresh_frame_context = 0; p->frame_parallel_decoding_mode = 1; }
    info->needs_backward_adaptation = !p->error_resilient_mode && !p->frame_parallel_decoding_mode;
    p->frame_context_idx = (uint8_t)svt_bit_literal(&r, 2);
    p->filter_level = (uint8_t)svt_bit_literal(&r, 6);
    p->sharpness_level = (uint8_t)svt_bit_literal(&r, 3);
    p->mode_ref_delta_enabled = (uint8_t)svt_bit_read(&r);
    if (p->mode_ref_delta_enabled) {
        p->mode_ref_delta_update = (uint8_t)svt_bit_read(&r);
        if (p->mode_ref_delta_update) {
            for (int i = 0; i < 4; i++) p->ref_deltas[i] = (int8_t)read_lf_delta(&r, last_ref_deltas[i]);
            for (int i = 0; i < 2; i++) p->mode_deltas[i] = (int8_t)read_lf_delta(&r, last_mode_deltas[i]);
        }
    }
    p->base_qindex = (uint8_t)svt_bit_literal(&r, 8);
    p->y_dc_delta_q = (int8_t)read_delta_q(&r);
    p->uv_dc_delta_q = (int8_t)read_delta_q(&r);
    p->uv_ac_delta_q = (int8_t)read_delta_q(&r);
    info->lossless = p->base_qindex == 0 && !p->y_dc_delta_q && !p->uv_dc_delta_q && !p->uv_ac_delta_q;
    if (svt_bit_read(&r)) return fail(SVT_HIP_ERR_UNSUPPORTED, "segmentation");
    /* read_tile_info: increment bits while below max_log2_tile_cols (min_log2 is 0 up to 64 SB columns), then the rows */
    const int sb64_cols = (((p->width + 7) >> 3) + 7) >> 3;
    if (sb64_cols > 64) return fail(SVT_HIP_ERR_UNSUPPORTED, "more than 64 superblock columns need more than one tile column");
    int max_log2 = 1;
    while ((sb64_cols >> max_log2) >= 4) max_log2++;
    max_log2--;
    if (max_log2 > 0 && svt_bit_read(&r)) return fail(SVT_HIP_ERR_UNSUPPORTED, "more than one tile column");
    if (svt_bit_read(&r)) return fail(SVT_HIP_ERR_UNSUPPORTED, "more than one tile row");
    const uint32_t first_part_size = svt_bit_literal(&r, 16);
    if (r.overrun) return fail(SVT_HIP_ERR_BAD_PARAMETER, "the uncompressed header is truncated");
    const uint32_t ub = (uint32_t)((r.bits + 7) >> 3);
    info->uncompressed_bytes = ub;
    info->compressed_bytes = first_part_size;
    if (first_part_size == 0) return fail(SVT_HIP_ERR_BAD_PARAMETER, "first_part_size 0");
    if ((uint64_t)ub + first_part_size > size) return fail(SVT_HIP_ERR_BAD_PARAMETER, "the compressed header is truncated");
    /* (lossless: a decoder reads no tx_mode and takes ONLY_4X4 with the Walsh-Hadamard transform; the writers send tx_mode all the same, so the
       bytes are parsed as written and the flag is the caller's to act on -- a tile must not be read under it) */
    /* read_compressed_header */
    svt_bool_reader b;
    if (svt_bool_reader_init(&b, frame + ub, first_part_size)) return fail(SVT_HIP_ERR_BAD_PARAMETER, "marker bit of the compressed header");
    info->tx_mode = (uint8_t)svt_bool_literal(&b, 2);
    if (info->tx_mode == 3) info->tx_mode = (uint8_t)(3 + svt_bool_read(&b, 128));
    if (info->tx_mode == 4) return fail(SVT_HIP_ERR_UNSUPPORTED, "TX_MODE_SELECT");
    for (int t = 0; t <= info->tx_mode; t++) /* read_coef_probs: one update bit per transform size up to the mode's largest */
        if (svt_bool_read(&b, 128)) {
            if (!tables) return fail(SVT_HIP_ERR_UNSUPPORTED, "coefficient probability update");
            read_coef_updates(&b, tables->coef_probs + 432 * t);
        }
    int upd = any_update(&b, 3); /* skip */
    p->reference_mode = SVT_MODES_SINGLE_REFERENCE;
    if (p->frame_type != 0 && !p->intra_only && !upd) {
        upd |= any_update(&b, 7 * 3); /* inter modes */
        if (info->interp_filter == SVT_READ_FILTER_SWITCHABLE) upd |= any_update(&b, 4 * 2);
        upd |= any_update(&b, 4);     /* intra / inter */
        if (!upd && p->allow_comp_inter_inter) { /* read_frame_reference_mode */
            if (svt_bool_read(&b, 128)) p->reference_mode = svt_bool_read(&b, 128) ? SVT_MODES_REFERENCE_SELECT : SVT_MODES_COMPOUND_REFERENCE;
        }
        if (!upd) {
            if (p->reference_mode == SVT_MODES_REFERENCE_SELECT) upd |= any_update(&b, 5);
            if (p->reference_mode != SVT_MODES_COMPOUND_REFERENCE) upd |= any_update(&b, 5 * 2);
            if (p->reference_mode != SVT_MODES_SINGLE_REFERENCE) upd |= any_update(&b, 5);
            upd |= any_update(&b, 4 * 9);   /* y modes */
            upd |= any_update(&b, 16 * 3);  /* partitions */
            upd |= any_update(&b, 3 + 2 * (1 + 10 + 1 + 10) + 2 * (2 * 3 + 3)); /* read_mv_probs */
            if (p->allow_hp) upd |= any_update(&b, 2 * 2);
        }
    }
    if (upd) return fail(SVT_HIP_ERR_UNSUPPORTED, "forward probability update");
    if (svt_bool_past_end(&b)) return fail(SVT_HIP_ERR_BAD_PARAMETER, "the compressed header ends inside a symbol");
    return SVT_HIP_OK;
}

int32_t svt_hip_frame_read_header_host(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2],
                                       svt_frame_read_info *info) {
    return read_header(frame, size, last_ref_deltas, last_mode_deltas, info, NULL);
}
int32_t svt_hip_frame_read_header_coef_host(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2],
                                            svt_frame_read_info *info, svt_bool_tables *tables_inout) {
    if (!tables_inout) return fail(SVT_HIP_ERR_BAD_PARAMETER, "null argument");
    return read_header(frame, size, last_ref_deltas, last_mode_deltas, info, tables_inout);
}

/* ------------------------------------------------------------------------------------------------------------------------------------ */
/* key-frame tile reader: the inverse of csrc/modeinfo_core.h (partition, skip, intra modes) and csrc/tokenize_core.h + boolcode_core.h     */
/* (tokens), block by block in coding order.  Every context is read from the grid and the eob map filled so far with the writers' own      */
/* functions: the leaves above and left of a node are decoded in front of it (modeinfo_core.h's argument).                                  */
/* ------------------------------------------------------------------------------------------------------------------------------------ */
#include "../csrc/modeinfo_inter_core.h"
#include "../csrc/mvrefs_core.h"

typedef struct tile_reader {
    svt_bool_reader         b;
    svt_tok_geom            g;
    int                     sb_cols, filter_level;
    const svt_bool_tables  *bt;
    const svt_modes_tables *mt;
    const int16_t          *scan;      /* canonical scan array (svt_hip_vp9_scan_tables) */
    svt_lf_mode_info       *mi;
    int16_t                *q;
    uint16_t               *emap;
    svt_tile_read_result   *res;
    int                     err;       /* 0, or the first refusal's code */
    const char             *why;
    /* a picture that is not intra-only: the frame's tables and parameters, the two further grids */
    const svt_modes_inter_tables *it;  /* null: key frame / intra-only picture */
    const svt_tile_read_params   *par;
    svt_mc_mode_info       *mc;
    svt_mi_inter_ext       *ext;
    svt_mii_frame           f;
} tile_reader;

static int read_intra_mode(svt_bool_reader *b, const uint8_t *probs);
/* vpx_reader_find_end: the bytes in front of the first one the window has not started to consume; a window that has been filled up to the
 * buffer's end (libvpx then stops rewinding: its count holds LOTS_OF_BITS) answers the end */
static uint64_t bool_reader_end(const svt_bool_reader *b) {
    if (b->fetched >= b->size) return b->size;
    return b->fetched - (b->count > 8 ? (uint64_t)(b->count - 1) / 8 : 0);
}
static void refuse(tile_reader *t, const char *why) { if (!t->err) { t->err = SVT_HIP_ERR_UNSUPPORTED; t->why = why; } }

/* the loop-filter level of a block as the decoder derives it (vp9_loop_filter_frame_init + get_filter_level, no segmentation): the
 * header's level, and with mode_ref_delta_enabled + ref_deltas[ref_frame[0]] * scale (+ mode_deltas[mode is not ZEROMV] * scale for an inter
 * block), scale = 1 << (level >> 5), clamped to 0 .. 63 */
static int block_filter_level(const svt_tile_read_params *p, int ref_frame0, int mode) {
    int lvl = p->filter_level;
    if (p->mode_ref_delta_enabled && lvl) {
        const int scale = 1 << (lvl >> 5);
        lvl += p->ref_deltas[ref_frame0 & 3] * scale;
        if (ref_frame0 > 0) lvl += p->mode_deltas[mode != 12] * scale;
        lvl = lvl < 0 ? 0 : lvl > 63 ? 63 : lvl;
    }
    return lvl;
}

/* the four-leaf tree 0 | (1 | (2 | 3)) of svt_mii_tree4, read: the number of leading ones, at most 3 */
static int read_tree4(svt_bool_reader *b, const uint8_t *probs) {
    int v = 0;
    while (v < 3 && svt_bool_read(b, probs[v])) v++;
    return v;
}
/* read_mv_component, the inverse of svt_mii_mv_comp_bools; the class is read by matching the bits so far against the writer's own path
 * table (every class consistent with a prefix names the same next node) */
static int read_mv_component(svt_bool_reader *b, int usehp, const svt_modes_mv_comp *p) {
    const int sign = svt_bool_read(b, p->sign);
    int c = -1, v = 0;
    for (int k = 0; k < 7 && c < 0; k++) {
        int node = 0;
        for (int cc = 0; cc <= 10; cc++)
            if (svt_mii_class_len(cc) > k && (svt_mii_class_path(cc) >> (svt_mii_class_len(cc) - k)) == v) { node = svt_mii_class_node(cc, k); break; }
        v = v << 1 | svt_bool_read(b, p->classes[node]);
        for (int cc = 0; cc <= 10; cc++)
            if (svt_mii_class_len(cc) == k + 1 && svt_mii_class_path(cc) == v) c = cc;
    }
    if (c < 0) c = 10; /* (unreachable: the eleven paths are a complete prefix code) */
    int d = 0;
    if (c == 0) d = svt_bool_read(b, p->class0[0]);
    else
        for (int i = 0; i < c; i++) d |= svt_bool_read(b, p->bits[i]) << i;
    const int fr = read_tree4(b, c == 0 ? p->class0_fp[d] : p->fp);
    const int hp = usehp ? svt_bool_read(b, c == 0 ? p->class0_hp : p->hp) : 1; /* a bit that is not coded reads as set */
    const int mag = (c ? 8 << c : 0) + (d << 3 | fr << 1 | hp) + 1;
    return sign ? -mag : mag;
}

/* an inter picture's leaf of `level` at unit (r, c), behind its partition symbols: pack_inter_mode_mvs read back (svt_mii_unit_bools),
 * the candidates by svt_mvr_derive on the grids filled so far, then the leaf's tokens */
static void read_leaf_tokens(tile_reader *t, int r, int c, int n, const svt_lf_mode_info *rec);
static void read_inter_leaf(tile_reader *t, int r, int c, int level, int sb_type) {
    const int n = 1 << level, idx = r * t->g.mi_stride + c;
    const svt_mii_view v = {t->mi, t->mc, t->ext, t->f};
    const int a = svt_mii_neighbour(&v, r > 0, idx - t->g.mi_stride), lf = svt_mii_neighbour(&v, c > 0, idx - 1);
    svt_lf_mode_info rec;
    svt_mc_mode_info mc;
    svt_mi_inter_ext ext;
    memset(&rec, 0, sizeof rec); memset(&mc, 0, sizeof mc); memset(&ext, 0, sizeof ext);
    rec.sb_type = (uint8_t)sb_type;
    rec.tx_size = (uint8_t)(sb_type == 0 ? 0 : level < 2 ? level + 1 : 3);
    rec.skip = (uint8_t)svt_bool_read(&t->b, t->it->skip_probs[svt_nb_skip(a) + svt_nb_skip(lf)]);
    rec.is_inter = (uint8_t)svt_bool_read(&t->b, t->it->intra_inter_prob[svt_mii_ctx_intra_inter(a, lf)]);
    mc.ref_list[0] = mc.ref_list[1] = -1;
    mc.bw8 = mc.bh8 = (uint8_t)n;
    if (!rec.is_inter) {
        const uint8_t *yp = t->it->y_mode_prob[sb_type == 0 ? 0 : level < 2 ? level + 1 : 3];
        if (sb_type) rec.pad_[1] = (uint8_t)read_intra_mode(&t->b, yp);
        else {
            const int m0 = read_intra_mode(&t->b, yp), m1 = read_intra_mode(&t->b, yp), m2 = read_intra_mode(&t->b, yp), m3 = read_intra_mode(&t->b, yp);
            rec.pad_[1] = (uint8_t)(m0 | m1 << 4);
            rec.pad_[0] = (uint8_t)(m2 | m3 << 4);
        }
        rec.pad_[2] = (uint8_t)read_intra_mode(&t->b, t->it->uv_mode_prob[svt_mi_y_mode(&rec, 3)]);
        rec.filter_level = (uint8_t)block_filter_level(t->par, 0, 0);
    } else {
        if (sb_type == 0) { refuse(t, "inter blocks below 8x8"); return; }
        int comp = t->f.reference_mode == SVT_MODES_COMPOUND_REFERENCE;
        if (t->f.reference_mode == SVT_MODES_REFERENCE_SELECT) comp = svt_bool_read(&t->b, t->it->comp_inter_prob[svt_mii_ctx_comp_inter(a, lf, t->f.comp_fixed_ref)]);
        if (comp) {
            const int fix_idx = t->f.ref_frame_sign_bias[t->f.comp_fixed_ref & 3] != 0;
            const int bit = svt_bool_read(&t->b, t->it->comp_ref_prob[svt_mii_ctx_comp_ref(a, lf, &t->f)]);
            ext.ref_frame[fix_idx] = t->f.comp_fixed_ref;
            ext.ref_frame[!fix_idx] = t->f.comp_var_ref[bit];
        } else {
            ext.ref_frame[0] = 1;
            if (svt_bool_read(&t->b, t->it->single_ref_prob[svt_mii_ctx_single_p1(a, lf)][0]))
                ext.ref_frame[0] = (uint8_t)(2 + svt_bool_read(&t->b, t->it->single_ref_prob[svt_mii_ctx_single_p2(a, lf)][1]));
        }
        for (int k = 0; k <= comp; k++) { /* the list that stands for the reference frame */
            const int f = ext.ref_frame[k];
            mc.ref_list[k] = (int8_t)(t->par->list_ref_frame[0] == f ? 0 : t->par->list_ref_frame[1] == f ? 1 : -1);
            if (mc.ref_list[k] < 0) { refuse(t, "a reference frame with no list in list_ref_frame"); return; }
        }
        /* the window of the leaf's SB over what is decoded so far (mvrefs_host.c's loop); every position the derivation reads lies in a
           leaf decoded before this one */
        const int sb_r = r & ~7, sb_c = c & ~7;
        const svt_mvr_view mv = svt_mvr_view_of(t->mi, t->mc, t->ext, 0, t->par->restrict_ref_mvs, t->f.ref_frame_sign_bias);
        uint32_t win[SVT_MVR_WIN_WORDS];
        for (int i = 0; i < SVT_MVR_WIN * SVT_MVR_WIN; i++) {
            int wr, wc;
            svt_mvr_entry e = svt_mvr_no_entry();
            if (svt_mvr_window_unit(&t->g, sb_r, sb_c, i, &wr, &wc)) e = svt_mvr_pack(&mv, &t->g, wr, wc);
            svt_mvr_window_put(win, i, e);
        }
        ext.mode_context = (uint8_t)svt_mvr_context(win, r - sb_r + 3, c - sb_c + 3, level);
        const int tv = read_tree4(&t->b, t->it->inter_mode_probs[ext.mode_context]);
        ext.mode = (uint8_t)(tv == 0 ? 12 : tv == 3 ? 13 : 9 + tv);
        for (int k = 0; k <= comp; k++) {
            uint32_t l0 = 0, l1 = 0;
            (void)svt_mvr_derive(&mv, &t->g, win, r - sb_r + 3, c - sb_c + 3, r, c, level, ext.ref_frame[k], &l0, &l1);
            ext.ref_mv_row[k] = (int16_t)svt_mvr_row(l0); ext.ref_mv_col[k] = (int16_t)svt_mvr_col(l0);
            uint32_t use = ext.mode == 10 ? l0 : ext.mode == 11 ? l1 : 0;
            int row = svt_mvr_row(use), col = svt_mvr_col(use);
            const int usehp = t->f.allow_hp && svt_mii_use_mv_hp(ext.ref_mv_row[k], ext.ref_mv_col[k]);
            if (ext.mode == 13) {
                const int j = read_tree4(&t->b, t->it->mv_joints); /* 2 * (row differs) + (column differs) */
                const int drow = j & 2 ? read_mv_component(&t->b, usehp, &t->it->mv_comps[0]) : 0;
                const int dcol = j & 1 ? read_mv_component(&t->b, usehp, &t->it->mv_comps[1]) : 0;
                row = (int16_t)(ext.ref_mv_row[k] + drow); col = (int16_t)(ext.ref_mv_col[k] + dcol);
            }
            /* a decoder lowers the precision of a candidate that carries no high-precision bit (find_best_ref_mvs): an odd one is counted */
            const uint32_t cand = ext.mode == 11 ? l1 : l0;
            if (ext.mode != 12 && !(t->f.allow_hp && svt_mii_use_mv_hp(svt_mvr_row(cand), svt_mvr_col(cand))) && ((svt_mvr_row(cand) | svt_mvr_col(cand)) & 1))
                t->res->odd_candidates++;
            mc.mv_row[k] = (int16_t)row; mc.mv_col[k] = (int16_t)col;
        }
        rec.filter_level = (uint8_t)block_filter_level(t->par, ext.ref_frame[0], ext.mode);
        t->res->inter_leaves++;
    }
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++) {
            const int i = (r + y) * t->g.mi_stride + c + x;
            svt_mi_inter_ext e = ext;
            if (x | y) { e.mode = e.mode_context = 0; e.ref_mv_row[0] = e.ref_mv_row[1] = e.ref_mv_col[0] = e.ref_mv_col[1] = 0; } /* (svt_mvr_unit's format) */
            t->mi[i] = rec; t->mc[i] = mc; t->ext[i] = e;
        }
    t->res->leaves++;
    t->res->skipped_leaves += rec.skip;
    read_leaf_tokens(t, r, c, n, &rec);
}


/* eb_vp9_coef_con_tree (VPX/vp9_entropy.c): the constrained part of the token tree, leaves TWO .. CATEGORY6 = 2 .. 10 */
static const int8_t coef_con_tree[16] = {2, 6, -2, 4, -3, -4, 8, 10, -5, -6, 12, 14, -7, -8, -9, -10};

/* one intra mode through the writer's own path table (svt_mi_mode_len / svt_mi_mode_path): bools are read until the bits so far are a
 * mode's whole path; node k's probability index is svt_mi_mode_bools' */
static int read_intra_mode(svt_bool_reader *b, const uint8_t *probs) {
    int v = 0, d45_side = 0;
    for (int k = 0; k < SVT_MI_MODE_BOOLS; k++) {
        const int bit = svt_bool_read(b, probs[k < 4 ? k : k + 2 * d45_side]);
        if (k == 3) d45_side = bit;
        v = v << 1 | bit;
        for (int m = 0; m < 10; m++)
            if (svt_mi_mode_len(m) == k + 1 && svt_mi_mode_path(m) == v) return m;
    }
    return -1; /* (unreachable: the ten paths are a complete prefix code) */
}

/* decode_coefs (libvpx vp9_detokenize.c) of one transform block into its position-addressed coefficients; returns the eob */
static int read_block_tokens(tile_reader *t, int plane, int x4, int y4, const svt_tok_block *k) {
    const int      n = 16 << (2 * k->ts), ptype = plane ? 1 : 0;
    const int16_t *scan = t->scan + svt_tok_scan_offset(k->ts, k->tt);
    int16_t       *q = t->q + svt_coeff_offset(plane, x4 * 4, y4 * 4, t->sb_cols);
    int            c = 0, after_zero = 0;
    while (c < n) {
        int ctx = k->ctx;
        if (c) {
            int a, b2;
            svt_tok_neighbors(k->ts, k->tt, scan[c], &a, &b2);
            ctx = (1 + svt_tok_energy(q[a]) + svt_tok_energy(q[b2])) >> 1;
        }
        const uint8_t *p = t->bt->coef_probs + 3 * ((((k->ts * 2 + ptype) * 2 + k->inter) * 6 + svt_tok_band(c, k->ts)) * 6 + ctx);
        if (!after_zero && !svt_bool_read(&t->b, p[0])) break; /* EOB */
        t->res->tokens++;
        if (!svt_bool_read(&t->b, p[1])) { after_zero = 1; c++; continue; } /* ZERO: the next position carries no EOB check */
        after_zero = 0;
        int val = 1;
        if (svt_bool_read(&t->b, p[2])) {
            const int tok = svt_br_tree(&t->b, coef_con_tree, t->bt->pareto[p[2] ? p[2] - 1 : 0]);
            int       extra = 0;
            const uint8_t *cat = t->bt->cat_probs[tok >= 5 ? tok - 5 : 0];
            for (int j = 0; j < svt_bool_cat_bits(tok); j++) extra = extra << 1 | svt_bool_read(&t->b, cat[j]); /* MSB first */
            val = svt_tok_base(tok) + extra;
        }
        q[scan[c]] = (int16_t)(svt_bool_read(&t->b, 128) ? -val : val);
        c++;
    }
    if (c < n) t->res->tokens++; /* (the EOB token) */
    return c;
}

/* a leaf of `level` (side 1 << level units; sb_type 0 = four 4x4 blocks) at unit (r, c): skip, modes, tokens */
static void read_leaf(tile_reader *t, int r, int c, int level, int sb_type) {
    if (t->it) { read_inter_leaf(t, r, c, level, sb_type); return; }
    const int n = 1 << level;
    svt_lf_mode_info *b = &t->mi[r * t->g.mi_stride + c];
    const svt_lf_mode_info *ab = r ? b - t->g.mi_stride : NULL, *lb = c ? b - 1 : NULL;
    svt_lf_mode_info rec;
    memset(&rec, 0, sizeof rec);
    rec.sb_type = (uint8_t)sb_type;
    rec.tx_size = (uint8_t)(sb_type == 0 ? 0 : level < 2 ? level + 1 : 3); /* ALLOW_32X32: the largest transform of the block */
    rec.filter_level = (uint8_t)t->filter_level;
    rec.skip = (uint8_t)svt_bool_read(&t->b, t->mt->skip_probs[(ab && ab->skip) + (lb && lb->skip)]);
    const int a0 = ab ? svt_mi_y_mode(ab, 2) : 0, a1 = ab ? svt_mi_y_mode(ab, 3) : 0, l0 = lb ? svt_mi_y_mode(lb, 1) : 0, l2 = lb ? svt_mi_y_mode(lb, 3) : 0;
    if (sb_type) rec.pad_[1] = (uint8_t)read_intra_mode(&t->b, t->mt->kf_y_mode_prob[a0][l0]);
    else {
        const int m0 = read_intra_mode(&t->b, t->mt->kf_y_mode_prob[a0][l0]), m1 = read_intra_mode(&t->b, t->mt->kf_y_mode_prob[a1][m0]);
        const int m2 = read_intra_mode(&t->b, t->mt->kf_y_mode_prob[m0][l2]), m3 = read_intra_mode(&t->b, t->mt->kf_y_mode_prob[m1][m2]);
        rec.pad_[1] = (uint8_t)(m0 | m1 << 4);
        rec.pad_[0] = (uint8_t)(m2 | m3 << 4);
    }
    rec.pad_[2] = (uint8_t)read_intra_mode(&t->b, t->mt->kf_uv_mode_prob[svt_mi_y_mode(&rec, 3)]);
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++) t->mi[(r + y) * t->g.mi_stride + c + x] = rec; /* (the leaf lies inside the picture: read_node) */
    t->res->leaves++;
    t->res->skipped_leaves += rec.skip;
    read_leaf_tokens(t, r, c, n, &rec);
}

/* the tokens of the leaf of n x n units at (r, c), whose record *rec is in the grid: Y, Cb, Cr, each plane's transform blocks in raster order */
static void read_leaf_tokens(tile_reader *t, int r, int c, int n, const svt_lf_mode_info *rec) {
    if (rec->skip) return;
    for (int plane = 0; plane < 3; plane++) {
        const int ts = plane ? svt_uv_tx_size(rec->sb_type, rec->tx_size) : rec->tx_size, s = 1 << ts;
        const int x0 = plane ? c : 2 * c, y0 = plane ? r : 2 * r, w = plane ? n : 2 * n, pw4 = plane ? t->g.w4 >> 1 : t->g.w4;
        for (int y4 = y0; y4 < y0 + w; y4 += s)
            for (int x4 = x0; x4 < x0 + w; x4 += s) {
                svt_tok_block k;
                if (!svt_tok_block_at(t->mi, t->emap, &t->g, plane, x4, y4, &k)) continue;
                t->emap[svt_tok_map_offset(&t->g, plane) + y4 * pw4 + x4] = (uint16_t)read_block_tokens(t, plane, x4, y4, &k);
            }
    }
}

/* read_partition + decode_partition at the node of `level` (3 = 64x64) whose origin is unit (r, c) */
static void read_node(tile_reader *t, int r, int c, int level) {
    if (r >= t->g.mi_rows || c >= t->g.mi_cols || t->err) return;
    const svt_lf_mode_info *b = &t->mi[r * t->g.mi_stride + c], *ab = r ? b - t->g.mi_stride : NULL, *lb = c ? b - 1 : NULL;
    const int sa = ab ? svt_mi_seg_context(ab->sb_type) : 0, sl = lb ? svt_mi_seg_context(lb->sb_type) : 0;
    const int hbs = (1 << level) >> 1, has_rows = r + hbs < t->g.mi_rows, has_cols = c + hbs < t->g.mi_cols;
    const int      pctx = 4 * level + 2 * ((sl >> level) & 1) + ((sa >> level) & 1);
    const uint8_t *p = t->it ? t->it->partition_prob[pctx] : t->mt->kf_partition_probs[pctx];
    int split = 1, rect = 0; /* partition_tree: NONE 0; HORZ 1 0; VERT 1 1 0; SPLIT 1 1 1 */
    if (has_rows && has_cols) {
        split = svt_bool_read(&t->b, p[0]);
        if (split && !svt_bool_read(&t->b, p[1])) rect = 1;
        else if (split && !svt_bool_read(&t->b, p[2])) rect = 1;
    } else if (has_cols) rect = !svt_bool_read(&t->b, p[1]);
    else if (has_rows) rect = !svt_bool_read(&t->b, p[2]);
    if (rect) { refuse(t, "rectangular partition"); return; }
    if (!split) { /* a leaf that reaches over the picture edge is legal VP9 that the writers never produce (svt_mi_check): caught before it indexes anything */
        if (r + (1 << level) > t->g.mi_rows || c + (1 << level) > t->g.mi_cols) { t->err = SVT_HIP_ERR_UNSUPPORTED; t->why = "a leaf that crosses the picture edge"; return; }
        read_leaf(t, r, c, level, 3 * (level + 1));
        return;
    }
    if (level == 0) { read_leaf(t, r, c, 0, 0); return; }
    for (int i = 0; i < 4; i++) read_node(t, r + (i >> 1) * hbs, c + (i & 1) * hbs, level - 1);
}

int32_t svt_hip_tile_read_kf_host(const uint8_t *tile, uint32_t size, int32_t width, int32_t height, int32_t mi_stride, int32_t filter_level,
                                  const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables, svt_lf_mode_info *lf_mi, int16_t *qcoeff,
                                  uint16_t *eob_map, svt_tile_read_result *result) {
    if (!tile || !bool_tables || !modes_tables || !lf_mi || !qcoeff || !eob_map || !result || size == 0 || filter_level < 0 || filter_level > 63)
        return fail(SVT_HIP_ERR_BAD_PARAMETER, "tile: bad argument");
    tile_reader t;
    memset(&t, 0, sizeof t);
    int n_sb = 0;
    if (svt_tok_geom_of(width, height, mi_stride, &t.g, &t.sb_cols, &n_sb)) return fail(SVT_HIP_ERR_BAD_PARAMETER, "tile: picture size");
    memset(result, 0, sizeof *result);
    for (int r = 0; r < t.g.mi_rows; r++) memset(lf_mi + (size_t)r * mi_stride, 0, sizeof(svt_lf_mode_info) * (size_t)t.g.mi_cols);
    memset(qcoeff, 0, sizeof(int16_t) * (size_t)n_sb * SVT_SB_COEFFS);
    memset(eob_map, 0, sizeof(uint16_t) * (size_t)t.g.w4 * t.g.h4 * 3 / 2);
    t.bt = bool_tables; t.mt = modes_tables; t.mi = lf_mi; t.q = qcoeff; t.emap = eob_map; t.res = result; t.filter_level = filter_level;
    t.scan = svt_hip_vp9_scan_tables(NULL, NULL);
    if (!t.scan) return fail(SVT_HIP_ERR_NO_RESOURCES, "tile: scan tables");
    if (svt_bool_reader_init(&t.b, tile, size)) return fail(SVT_HIP_ERR_BAD_PARAMETER, "tile: marker bit");
    for (int r = 0; r < t.g.mi_rows && !t.err; r += 8)
        for (int c = 0; c < t.g.mi_cols && !t.err; c += 8) read_node(&t, r, c, 3);
    if (t.err) return fail(t.err, t.why);
    result->tile_bytes = (uint32_t)bool_reader_end(&t.b);
    result->past_end = (uint32_t)svt_bool_past_end(&t.b);
    return SVT_HIP_OK;
}

/* eb_vp9_setup_compound_reference_mode: the fixed and the two variable references from the sign biases */
static void compound_references(svt_mii_frame *f) {
    const uint8_t *sb = f->ref_frame_sign_bias;
    if (sb[1] == sb[2]) { f->comp_fixed_ref = 3; f->comp_var_ref[0] = 1; f->comp_var_ref[1] = 2; }
    else if (sb[1] == sb[3]) { f->comp_fixed_ref = 2; f->comp_var_ref[0] = 1; f->comp_var_ref[1] = 3; }
    else { f->comp_fixed_ref = 1; f->comp_var_ref[0] = 2; f->comp_var_ref[1] = 3; }
}

int32_t svt_hip_tile_read_host(const uint8_t *tile, uint32_t size, const svt_tile_read_params *par, const svt_bool_tables *bool_tables,
                               const svt_modes_tables *modes_tables, const svt_modes_inter_tables *inter_tables, svt_lf_mode_info *lf_mi,
                               svt_mc_mode_info *mc_mi, svt_mi_inter_ext *ext, int16_t *qcoeff, uint16_t *eob_map, svt_tile_read_result *result) {
    if (!par) return fail(SVT_HIP_ERR_BAD_PARAMETER, "tile: bad argument");
    if (par->lossless) return fail(SVT_HIP_ERR_UNSUPPORTED, "lossless (q index 0 without deltas): a decoder takes ONLY_4X4 and the Walsh-Hadamard transform");
    if (par->intra_only) {
        if (par->mode_ref_delta_enabled && (par->ref_deltas[0] < -63 || par->ref_deltas[0] > 63)) return fail(SVT_HIP_ERR_BAD_PARAMETER, "tile: loop-filter delta");
        return svt_hip_tile_read_kf_host(tile, size, par->width, par->height, par->mi_stride, block_filter_level(par, 0, 0), bool_tables, modes_tables, lf_mi, qcoeff, eob_map, result);
    }
    if (!tile || !bool_tables || !inter_tables || !lf_mi || !mc_mi || !ext || !qcoeff || !eob_map || !result || size == 0 || par->filter_level > 63 ||
        par->reference_mode > SVT_MODES_REFERENCE_SELECT)
        return fail(SVT_HIP_ERR_BAD_PARAMETER, "tile: bad argument");
    if (par->interp_filter != SVT_READ_FILTER_REGULAR) return fail(SVT_HIP_ERR_UNSUPPORTED, "an interpolation filter other than the regular 8-tap one (switchable included)");
    tile_reader t;
    memset(&t, 0, sizeof t);
    int n_sb = 0;
    if (svt_tok_geom_of(par->width, par->height, par->mi_stride, &t.g, &t.sb_cols, &n_sb)) return fail(SVT_HIP_ERR_BAD_PARAMETER, "tile: picture size");
    t.f.reference_mode = par->reference_mode; t.f.allow_hp = par->allow_hp != 0;
    for (int i = 0; i < 4; i++) t.f.ref_frame_sign_bias[i] = par->ref_frame_sign_bias[i] != 0;
    compound_references(&t.f);
    memset(result, 0, sizeof *result);
    for (int r = 0; r < t.g.mi_rows; r++) {
        memset(lf_mi + (size_t)r * par->mi_stride, 0, sizeof(svt_lf_mode_info) * (size_t)t.g.mi_cols);
        memset(mc_mi + (size_t)r * par->mi_stride, 0, sizeof(svt_mc_mode_info) * (size_t)t.g.mi_cols);
        memset(ext + (size_t)r * par->mi_stride, 0, sizeof(svt_mi_inter_ext) * (size_t)t.g.mi_cols);
    }
    memset(qcoeff, 0, sizeof(int16_t) * (size_t)n_sb * SVT_SB_COEFFS);
    memset(eob_map, 0, sizeof(uint16_t) * (size_t)t.g.w4 * t.g.h4 * 3 / 2);
    t.bt = bool_tables; t.it = inter_tables; t.par = par; t.mi = lf_mi; t.mc = mc_mi; t.ext = ext; t.q = qcoeff; t.emap = eob_map; t.res = result;
    t.scan = svt_hip_vp9_scan_tables(NULL, NULL);
    if (!t.scan) return fail(SVT_HIP_ERR_NO_RESOURCES, "tile: scan tables");
    if (svt_bool_reader_init(&t.b, tile, size)) return fail(SVT_HIP_ERR_BAD_PARAMETER, "tile: marker bit");
    for (int r = 0; r < t.g.mi_rows && !t.err; r += 8)
        for (int c = 0; c < t.g.mi_cols && !t.err; c += 8) read_node(&t, r, c, 3);
    if (t.err) return fail(t.err, t.why);
    result->tile_bytes = (uint32_t)bool_reader_end(&t.b);
    result->past_end = (uint32_t)svt_bool_past_end(&t.b);
    return SVT_HIP_OK;
}

/* header and tile; updated: null for the plain reader, which refuses a coefficient update; else a copy of the caller's tables that the
 * header's updates are applied to and the tile is read with */
static int32_t frame_read(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2], int32_t mi_stride,
                          int32_t restrict_ref_mvs, const uint8_t list_ref_frame[2], const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables,
                          const svt_modes_inter_tables *inter_tables, svt_frame_read_info *info, svt_lf_mode_info *lf_mi, svt_mc_mode_info *mc_mi,
                          svt_mi_inter_ext *ext, int16_t *qcoeff, uint16_t *eob_map, svt_tile_read_result *result, svt_bool_tables *updated) {
    if (!list_ref_frame) return fail(SVT_HIP_ERR_BAD_PARAMETER, "null argument");
    const int32_t rc = updated ? svt_hip_frame_read_header_coef_host(frame, size, last_ref_deltas, last_mode_deltas, info, updated)
                               : svt_hip_frame_read_header_host(frame, size, last_ref_deltas, last_mode_deltas, info);
    if (rc) return rc;
    if (updated) bool_tables = updated;
    if (info->show_existing_frame) return fail(SVT_HIP_ERR_BAD_PARAMETER, "a show-existing frame has no tile");
    const svt_frame_params *p = &info->params;
    svt_tile_read_params par;
    memset(&par, 0, sizeof par);
    par.width = p->width; par.height = p->height; par.mi_stride = mi_stride;
    par.intra_only = p->frame_type == 0 || p->intra_only; par.reference_mode = p->reference_mode; par.allow_hp = p->allow_hp;
    par.restrict_ref_mvs = restrict_ref_mvs != 0; par.interp_filter = info->interp_filter; par.lossless = info->lossless;
    par.filter_level = p->filter_level; par.mode_ref_delta_enabled = p->mode_ref_delta_enabled;
    for (int i = 0; i < 4; i++) { par.ref_deltas[i] = p->ref_deltas[i]; par.ref_frame_sign_bias[i] = p->ref_frame_sign_bias[i]; }
    par.mode_deltas[0] = p->mode_deltas[0]; par.mode_deltas[1] = p->mode_deltas[1];
    par.list_ref_frame[0] = list_ref_frame[0]; par.list_ref_frame[1] = list_ref_frame[1];
    if ((p->width & 7) || (p->height & 7)) return fail(SVT_HIP_ERR_UNSUPPORTED, "a picture size that is no multiple of 8");
    const uint32_t at = info->uncompressed_bytes + info->compressed_bytes;
    if (at >= size) return fail(SVT_HIP_ERR_BAD_PARAMETER, "the frame ends in front of its tile");
    return svt_hip_tile_read_host(frame + at, size - at, &par, bool_tables, modes_tables, inter_tables, lf_mi, mc_mi, ext, qcoeff, eob_map, result);
}

int32_t svt_hip_frame_read_host(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2], int32_t mi_stride,
                                int32_t restrict_ref_mvs, const uint8_t list_ref_frame[2], const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables,
                                const svt_modes_inter_tables *inter_tables, svt_frame_read_info *info, svt_lf_mode_info *lf_mi, svt_mc_mode_info *mc_mi,
                                svt_mi_inter_ext *ext, int16_t *qcoeff, uint16_t *eob_map, svt_tile_read_result *result) {
    return frame_read(frame, size, last_ref_deltas, last_mode_deltas, mi_stride, restrict_ref_mvs, list_ref_frame, bool_tables, modes_tables, inter_tables, info, lf_mi,
                      mc_mi, ext, qcoeff, eob_map, result, NULL);
}

int32_t svt_hip_frame_read_coef_host(const uint8_t *frame, uint32_t size, const int8_t last_ref_deltas[4], const int8_t last_mode_deltas[2], int32_t mi_stride,
                                     int32_t restrict_ref_mvs, const uint8_t list_ref_frame[2], const svt_bool_tables *bool_tables,
                                     const svt_modes_tables *modes_tables, const svt_modes_inter_tables *inter_tables, svt_frame_read_info *info,
                                     svt_lf_mode_info *lf_mi, svt_mc_mode_info *mc_mi, svt_mi_inter_ext *ext, int16_t *qcoeff, uint16_t *eob_map,
                                     svt_tile_read_result *result, svt_bool_tables *tables_out) {
    if (!bool_tables) return fail(SVT_HIP_ERR_BAD_PARAMETER, "null argument");
    svt_bool_tables own = *bool_tables; /* the caller's tables stay what they were */
    const int32_t   rc = frame_read(frame, size, last_ref_deltas, last_mode_deltas, mi_stride, restrict_ref_mvs, list_ref_frame, bool_tables, modes_tables, inter_tables, info,
                                    lf_mi, mc_mi, ext, qcoeff, eob_map, result, &own);
    if (!rc && tables_out) *tables_out = own;
    return rc;
}

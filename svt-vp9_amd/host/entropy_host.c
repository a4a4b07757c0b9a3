/*
 * entropy_host.c -- host-side (plain C) half of the entropy pass (csrc/entropy.hip, rules in csrc/entropy_core.h):
 *   - the limits and the workspace's size, host values;
 *   - svt_hip_entropy_picture: the pass on host pointers -- the stages' host forms in the device entry's order and the same gate text --
 *     the model the GPU tests compare the device entry with; svt_hip_entropy_picture_coef, the same body in the coefficient-update mode;
 *   - svt_hip_entropy_deliverable and svt_hip_compound_refs_from_sign_bias, pure functions of a picture's frame parameters;
 *   - svt_entropy_check_picture, the per-picture checks both forms share.
 */
#include <stdlib.h>
#include <string.h>
#include "../../include/svtvp9_hip.h"
#include "../csrc/entropy_core.h"

void svt_hip_entropy_limits_worst(int32_t width, int32_t height, int32_t max_pics, svt_entropy_limits *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    svt_tok_geom g;
    int          sb_cols, n_sb;
    if (svt_tok_geom_of(width, height, width >> 3, &g, &sb_cols, &n_sb)) return;
    out->max_pics = max_pics < 0 ? 0u : (uint32_t)max_pics;
    out->max_tokens = svt_hip_tokenize_capacity(width, height);
    const uint64_t bools = (uint64_t)svt_hip_boolcode_bools_capacity(out->max_tokens) + svt_hip_modes_inter_bools_capacity(width, height);
    out->max_bools = bools > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bools;
    out->max_tile_bytes = svt_hip_boolcode_capacity(out->max_bools);
}

/* 0: limits a workspace can be created under */
int32_t svt_entropy_check_limits(int32_t width, int32_t height, int32_t mi_stride, const svt_entropy_limits *limits, svt_ent_layout *l) {
    if (!limits || limits->max_pics < 1 || limits->max_pics > SVT_FRAME_MAX_PICS || !svt_ent_bools_codable(limits->max_bools)) return SVT_HIP_ERR_BAD_PARAMETER;
    return svt_ent_layout_of(width, height, mi_stride, limits->max_tokens, limits->max_tile_bytes, l) ? SVT_HIP_ERR_BAD_PARAMETER : SVT_HIP_OK;
}

uint64_t svt_hip_entropy_work_bytes(int32_t width, int32_t height, int32_t mi_stride, const svt_entropy_limits *limits) {
    svt_ent_layout l;
    return svt_entropy_check_limits(width, height, mi_stride, limits, &l) ? 0 : l.bytes * limits->max_pics;
}

/* what both forms refuse of one picture, pointers aside; header (SVT_FRAME_HEADER_MAX bytes) receives the two headers */
int32_t svt_entropy_check_picture(const svt_entropy_picture *p, int32_t width, int32_t height, uint8_t *header, uint32_t *header_len) {
    uint32_t ub = 0, cb = 0;
    if (!p->d_lf_mi || !p->d_qcoeff || !p->d_eob_map || ((uintptr_t)p->d_qcoeff & 15) || p->trailer_len > 4) return SVT_HIP_ERR_BAD_PARAMETER;
    if (p->frame.width != width || p->frame.height != height) return SVT_HIP_ERR_BAD_PARAMETER;
    const int intra = svt_ent_intra_only(&p->frame);
    if (intra ? p->d_mc_mi != NULL : p->d_mc_mi == NULL) return SVT_HIP_ERR_BAD_PARAMETER;
    if (!intra)
        for (int k = 0; k < 2; k++)
            if (p->list_ref_frame[k] < 1 || p->list_ref_frame[k] > 3) return SVT_HIP_ERR_BAD_PARAMETER;
    if (svt_hip_frame_header_host(&p->frame, header, SVT_FRAME_HEADER_MAX, &ub, &cb)) return SVT_HIP_ERR_BAD_PARAMETER;
    *header_len = ub + cb;
    return SVT_HIP_OK;
}

uint32_t svt_hip_entropy_gate_host(uint32_t tok_total, uint32_t max_tokens, uint32_t n_bools, uint32_t bools_capacity, const uint32_t *status, uint32_t size,
                                   uint32_t max_tile_bytes, uint32_t *verdict_a, svt_entropy_result *result) {
    const uint32_t    a = svt_ent_verdict_a(tok_total, max_tokens, n_bools, bools_capacity, svt_ent_status_of(status));
    svt_entropy_result r;
    const uint32_t    out = svt_ent_result_of(svt_ent_verdict_b(a, size, max_tile_bytes), tok_total, n_bools, size, svt_ent_status_of(status), &r);
    if (verdict_a) *verdict_a = a;
    if (result) *result = r;
    return out;
}

/* bools of the stream a segment list describes: every raw bool one, every token what svt_bool_expand writes for it */
static uint64_t stream_bools(const uint32_t *tokens, const svt_bool_segment *segs, uint32_t n_segs) {
    uint64_t n = 0;
    for (uint32_t s = 0; s < n_segs; s++) {
        if (segs[s].kind) { n += segs[s].count; continue; }
        for (uint32_t k = 0; k < segs[s].count; k++) {
            const uint32_t rec = tokens[segs[s].first + k];
            n += (uint64_t)svt_bool_count((int)SVT_TOK_TOKEN(rec), svt_bool_skip0(rec, k > 0, k > 0 ? tokens[segs[s].first + k - 1] : 0));
        }
    }
    return n;
}

/* what the coefficient-update mode refuses of a picture beyond svt_entropy_check_picture: a decoder would store the updated probabilities */
int32_t svt_entropy_check_picture_coef(const svt_entropy_picture *p) {
    return !p->frame.error_resilient_mode && p->frame.refresh_frame_context ? SVT_HIP_ERR_BAD_PARAMETER : SVT_HIP_OK;
}

/* both host forms; coef: the coefficient-update mode, with its second slab beside the first */
static int32_t entropy_picture(const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables, const svt_modes_inter_tables *inter_tables,
                               const svt_entropy_picture *pic, int32_t mi_stride, const svt_entropy_limits *limits, uint8_t *packet, uint32_t packet_capacity,
                               uint32_t *packet_size, svt_entropy_result *result, svt_entropy_host_detail *detail, int coef, uint8_t *probs_out,
                               svt_cu_result *update_out) {
    if (!bool_tables || !pic || !limits || !packet_size || !result || (!packet && packet_capacity)) return SVT_HIP_ERR_BAD_PARAMETER;
    const int32_t  width = pic->frame.width, height = pic->frame.height;
    svt_ent_layout l;
    if (!svt_ent_bools_codable(limits->max_bools) || svt_ent_layout_of(width, height, mi_stride, limits->max_tokens, limits->max_tile_bytes, &l))
        return SVT_HIP_ERR_BAD_PARAMETER;
    uint8_t  header[SVT_FRAME_HEADER_MAX];
    uint32_t header_len = 0;
    if (svt_entropy_check_picture(pic, width, height, header, &header_len)) return SVT_HIP_ERR_BAD_PARAMETER;
    const int intra = svt_ent_intra_only(&pic->frame);
    if (intra ? !modes_tables : !inter_tables) return SVT_HIP_ERR_BAD_PARAMETER;
    svt_ent_coef_layout cl;
    svt_cu_picture      cu;
    uint32_t            size_bit = 0;
    svt_ent_coef_layout_of(&cl);
    memset(&cu, 0, sizeof cu);
    if (coef) { /* the uncompressed header alone, and the compressed header's records round the coefficient section */
        uint32_t n_prefix = 0, n_suffix = 0;
        if (svt_entropy_check_picture_coef(pic) || svt_hip_frame_header_uncompressed_host(&pic->frame, header, SVT_FRAME_UNCOMPRESSED_MAX, &header_len, &size_bit) ||
            svt_hip_frame_header_parts_host(&pic->frame, cu.prefix, &n_prefix, cu.suffix, &n_suffix))
            return SVT_HIP_ERR_BAD_PARAMETER;
        cu.n_prefix = (uint16_t)n_prefix; cu.n_suffix = (uint16_t)n_suffix;
    }

    /* the picture's part of a workspace, in host memory; in the coefficient-update mode its part of the second slab behind it */
    uint8_t *slab = (uint8_t *)calloc(1, (size_t)l.bytes + (coef ? (size_t)cl.bytes : 0));
    if (!slab) return SVT_HIP_ERR_NO_RESOURCES;
    uint8_t *const  slab2 = slab + l.bytes;
    uint32_t *const cwords = (uint32_t *)(slab2 + cl.words);
    uint32_t *const counts = !coef || pic->d_counts ? pic->d_counts : (uint32_t *)(slab2 + cl.counts);
    uint32_t *const         tok_off = (uint32_t *)(slab + l.tok_off), *const sb_off = (uint32_t *)(slab + l.sb_off), *const tokens = (uint32_t *)(slab + l.tokens);
    svt_mi_inter_ext *const ext = (svt_mi_inter_ext *)(slab + l.ext);
    uint16_t *const         bools = (uint16_t *)(slab + l.bools);
    svt_bool_segment *const segs = (svt_bool_segment *)(slab + l.segments);
    uint8_t *const          tile = slab + l.tile;
    uint32_t *const         words = (uint32_t *)(slab + l.words);
    uint32_t *const         status = intra ? NULL : words + SVT_ENT_W_STATUS;
    const uint32_t          bools_capacity = intra ? l.kf_bools : l.inter_bools;
    int32_t                 rc;

    const svt_tok_picture tp = {pic->d_lf_mi, pic->d_qcoeff, pic->d_eob_map, tokens, limits->max_tokens, 0, tok_off, sb_off, counts};
    rc = svt_hip_tokenize_picture(&tp, width, height, mi_stride);
    if (!rc && intra) {
        const svt_modes_picture mp = {pic->d_lf_mi, pic->d_eob_map, tok_off, bools, segs, words + SVT_ENT_W_N_BOOLS, bools_capacity, 0};
        rc = svt_hip_modes_kf_picture(modes_tables, &mp, width, height, mi_stride);
    } else if (!rc) {
        svt_md_inter_picture dp;
        memset(&dp, 0, sizeof dp);
        dp.d_lf_mi = pic->d_lf_mi; dp.d_mc_mi = pic->d_mc_mi; dp.d_ext_out = ext; dp.d_status = status;
        memcpy(dp.list_ref_frame, pic->list_ref_frame, 2);
        memcpy(dp.ref_frame_sign_bias, pic->frame.ref_frame_sign_bias, 4);
        dp.restrict_ref_mvs = pic->restrict_ref_mvs; dp.allow_hp = pic->frame.allow_hp; dp.reference_mode = pic->frame.reference_mode;
        svt_ent_compound_refs(pic->frame.ref_frame_sign_bias, &dp.comp_fixed_ref, dp.comp_var_ref);
        rc = svt_hip_md_inter_modes_picture(&dp, width, height, mi_stride);
        if (!rc) {
            svt_modes_inter_picture ip;
            memset(&ip, 0, sizeof ip);
            ip.d_lf_mi = pic->d_lf_mi; ip.d_eob_map = pic->d_eob_map; ip.d_tok_off = tok_off; ip.d_bools = bools; ip.d_segments = segs;
            ip.d_n_bools = words + SVT_ENT_W_N_BOOLS; ip.capacity = bools_capacity; ip.d_mc_mi = pic->d_mc_mi; ip.d_ext = ext;
            ip.reference_mode = dp.reference_mode; ip.allow_hp = dp.allow_hp; ip.comp_fixed_ref = dp.comp_fixed_ref;
            memcpy(ip.comp_var_ref, dp.comp_var_ref, 2);
            memcpy(ip.ref_frame_sign_bias, dp.ref_frame_sign_bias, 4);
            rc = svt_hip_modes_inter_picture(inter_tables, &ip, width, height, mi_stride);
        }
    }
    if (!rc && coef) {
        cu.d_tokens = tokens; cu.d_n_tokens = sb_off + l.n_sb; cu.d_counts = counts; cu.d_eob_branch = (uint32_t *)(slab2 + cl.eob_branch);
        cu.d_probs = slab2 + cl.probs; cu.d_hdr_bools = (uint16_t *)(slab2 + cl.hdr_bools); cu.d_n_hdr_bools = cwords + SVT_ENT_CW_N_HDR_BOOLS;
        cu.d_segment = (svt_bool_segment *)(cwords + SVT_ENT_CW_SEGMENT); cu.d_result = (svt_cu_result *)(slab2 + cl.result); cu.max_tokens = limits->max_tokens;
        rc = svt_hip_coef_update_picture(&cu, bool_tables);
    }
    svt_bool_tables *own = NULL; /* the tables with the picture's probabilities */
    if (!rc && coef) {
        own = (svt_bool_tables *)malloc(sizeof *own);
        if (!own) rc = SVT_HIP_ERR_NO_RESOURCES;
        else {
            *own = *bool_tables;
            memcpy(own->coef_probs, cu.d_probs, SVT_CU_PROBS);
        }
    }
    uint64_t n_stream = 0;
    if (!rc) {
        /* the gate, phase A: a withheld picture's list is emptied, so that nothing below reads tokens or bools */
        const uint32_t total = sb_off[l.n_sb], a = svt_ent_verdict_a(total, limits->max_tokens, words[SVT_ENT_W_N_BOOLS], bools_capacity, svt_ent_status_of(status));
        words[SVT_ENT_W_VERDICT] = a;
        if (a) memset(segs, 0, sizeof(svt_bool_segment) * (size_t)l.n_segments);
        /* the bool coder, with its own rule for a stream above max_bools */
        n_stream = stream_bools(tokens, segs, l.n_segments);
        if (n_stream > limits->max_bools) words[SVT_ENT_W_SIZE] = SVT_BOOL_SIZE_OVERFLOW;
        else
            rc = svt_hip_boolcode_host(own ? own : bool_tables, tokens, a ? 0 : (total < limits->max_tokens ? total : limits->max_tokens), bools,
                                       a ? 0 : words[SVT_ENT_W_N_BOOLS], segs, l.n_segments, tile, limits->max_tile_bytes, words + SVT_ENT_W_SIZE);
    }
    if (!rc && coef) /* the compressed header's stream, coded also for a picture that does not ship */
        rc = svt_hip_boolcode_host(bool_tables, NULL, 0, cu.d_hdr_bools, *cu.d_n_hdr_bools, cu.d_segment, 1, slab2 + cl.hdr_bytes, SVT_ENT_HDR_BYTES,
                                   cwords + SVT_ENT_CW_HDR_SIZE);
    free(own);
    if (!rc) {
        /* phase B and the frame stage's rule for one picture */
        const uint32_t coded = words[SVT_ENT_W_SIZE];
        const uint32_t flags = svt_ent_verdict_b(words[SVT_ENT_W_VERDICT], coded, limits->max_tile_bytes);
        words[SVT_ENT_W_SIZE] = svt_ent_result_of(flags, sb_off[l.n_sb], words[SVT_ENT_W_N_BOOLS], coded, svt_ent_status_of(status), result);
        const uint32_t comp = coef ? cwords[SVT_ENT_CW_HDR_SIZE] : 0;
        const uint32_t size = coef ? svt_frame_parts_size(header_len, pic->trailer_len, comp, SVT_ENT_HDR_BYTES, words[SVT_ENT_W_SIZE], limits->max_tile_bytes)
                                   : svt_frame_packet_size(header_len, pic->trailer_len, words[SVT_ENT_W_SIZE], limits->max_tile_bytes);
        if (detail) {
            detail->stream_bools = n_stream > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n_stream;
            detail->header_bytes = header_len + comp;
            detail->coded_size = coded;
            detail->pad_ = 0;
        }
        *packet_size = size;
        if (size != SVT_FRAME_SIZE_NONE) {
            if (size > packet_capacity) rc = SVT_HIP_ERR_BAD_PARAMETER;
            else {
                if (coef) {
                    for (uint32_t t = 0; t < header_len; t++) packet[t] = svt_frame_size_field_byte(header[t], t, size_bit, comp);
                    memcpy(packet + header_len, slab2 + cl.hdr_bytes, comp);
                } else
                    memcpy(packet, header, header_len);
                memcpy(packet + header_len + comp, tile, words[SVT_ENT_W_SIZE]);
                memcpy(packet + header_len + comp + words[SVT_ENT_W_SIZE], pic->trailer, pic->trailer_len);
            }
        }
        if (coef && probs_out) memcpy(probs_out, cu.d_probs, SVT_CU_PROBS);
        if (coef && update_out) *update_out = *cu.d_result;
    }
    free(slab);
    return rc;
}

int32_t svt_hip_entropy_picture(const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables, const svt_modes_inter_tables *inter_tables,
                                const svt_entropy_picture *pic, int32_t mi_stride, const svt_entropy_limits *limits, uint8_t *packet, uint32_t packet_capacity,
                                uint32_t *packet_size, svt_entropy_result *result, svt_entropy_host_detail *detail) {
    return entropy_picture(bool_tables, modes_tables, inter_tables, pic, mi_stride, limits, packet, packet_capacity, packet_size, result, detail, 0, NULL, NULL);
}

int32_t svt_hip_entropy_picture_coef(const svt_bool_tables *bool_tables, const svt_modes_tables *modes_tables, const svt_modes_inter_tables *inter_tables,
                                     const svt_entropy_picture *pic, int32_t mi_stride, const svt_entropy_limits *limits, uint8_t *packet, uint32_t packet_capacity,
                                     uint32_t *packet_size, svt_entropy_result *result, svt_entropy_host_detail *detail, uint8_t *probs, svt_cu_result *update) {
    return entropy_picture(bool_tables, modes_tables, inter_tables, pic, mi_stride, limits, packet, packet_capacity, packet_size, result, detail, 1, probs, update);
}

uint64_t svt_hip_entropy_coef_update_bytes(const svt_entropy_limits *limits) {
    svt_ent_coef_layout cl;
    if (!limits || limits->max_pics < 1 || limits->max_pics > SVT_FRAME_MAX_PICS || !svt_ent_bools_codable(limits->max_bools)) return 0;
    svt_ent_coef_layout_of(&cl);
    return cl.bytes * limits->max_pics;
}

uint32_t svt_hip_entropy_deliverable(const svt_frame_params *p) {
    if (!p) return 0;
    uint32_t f = 0;
    if (!p->error_resilient_mode && !p->frame_parallel_decoding_mode) f |= SVT_ENT_NEEDS_BACKWARD_ADAPTATION;
    if (p->base_qindex == 0 && p->y_dc_delta_q == 0 && p->uv_dc_delta_q == 0 && p->uv_ac_delta_q == 0) f |= SVT_ENT_LOSSLESS;
    if (!svt_ent_intra_only(p)) {
        const int readable = p->ref_frame_sign_bias[2] != p->ref_frame_sign_bias[1] || p->ref_frame_sign_bias[3] != p->ref_frame_sign_bias[1];
        if ((p->allow_comp_inter_inter != 0) != readable) f |= SVT_ENT_COMP_FLAG_MISMATCH;
        if (!readable && p->reference_mode != SVT_MODES_SINGLE_REFERENCE) f |= SVT_ENT_REFERENCE_MODE_UNREAD;
    }
    return f;
}

void svt_hip_compound_refs_from_sign_bias(const uint8_t sign_bias[4], uint8_t *comp_fixed_ref, uint8_t comp_var_ref[2]) {
    if (sign_bias && comp_fixed_ref && comp_var_ref) svt_ent_compound_refs(sign_bias, comp_fixed_ref, comp_var_ref);
}

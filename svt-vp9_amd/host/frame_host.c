/*
 * frame_host.c -- host-side (plain C) half of the frame stage (csrc/frame.hip, rules in csrc/frame_core.h):
 *   - svt_hip_frame_header_host: write_uncompressed_header, first_part_size and write_compressed_header of eb_vp9_pack_bitstream
 *     (VPX/vp9_bitstream.c:1186-1412).  The compressed header carries no probability update -- the reference's FRAME_COUNTS stay zero
 *     (VPX/vp9_tokenize.c:405-425 compiles the increments out, tx_totals is never incremented, Codec/EbResourceCoordinationProcess.c:666
 *     clears them), so update_coef_probs writes a 0 bit per transform size (:679-681) and every eb_vp9_cond_prob_diff_update
 *     (VPX/vp9_subexp.c:173-185), prob_diff_update (:56-66) and update_mv (VPX/vp9_encodemv.c:144-155) a 0 at probability 252 -- and is
 *     built as raw bool records and coded by svt_hip_boolcode_host: no second writer;
 *   - svt_hip_frame_header_parts_host / svt_hip_frame_header_coef_host: the same records in front of and behind update_coef_probs, and the
 *     two headers around a coefficient section that does update (csrc/coef_update.hip), from the same text;
 *   - svt_hip_frame_show_existing_host: the one-byte frame of show_existing_frame;
 *   - svt_hip_frame_assemble_host: the packet layout of csrc/frame_core.h over host pointers, the model of the assembly kernel;
 *   - svt_hip_frame_header_uncompressed_host and svt_hip_frame_assemble_parts_host: the uncompressed header alone with the place of
 *     first_part_size, and the model of the three-part assembly that fills it in from the compressed header's size.
 */
#include <string.h>
#include "../../include/svtvp9_hip.h"
#include "../csrc/frame_core.h"

/* vpx_write_bit_buffer (VPX/bitwriter_buffer.c): MSB first */
typedef struct {
    uint8_t  buf[SVT_FRAME_UNCOMPRESSED_MAX];
    uint32_t bits;
} bit_writer;

static void put_bit(bit_writer *w, int bit) {
    if (bit) w->buf[w->bits >> 3] |= (uint8_t)(0x80u >> (w->bits & 7));
    w->bits++;
}
static void put_literal(bit_writer *w, uint32_t v, int n) {
    while (n--) put_bit(w, (int)((v >> n) & 1u));
}

static void put_sync_code(bit_writer *w) { put_literal(w, 0x498342, 24); }

static void put_render_size(bit_writer *w, const svt_frame_params *p) { /* write_render_size, :1094-1101 */
    const int scaling = p->width != p->render_width || p->height != p->render_height;
    put_bit(w, scaling);
    if (scaling) {
        put_literal(w, (uint32_t)p->render_width - 1, 16);
        put_literal(w, (uint32_t)p->render_height - 1, 16);
    }
}
static void put_frame_size(bit_writer *w, const svt_frame_params *p) {
    put_literal(w, (uint32_t)p->width - 1, 16);
    put_literal(w, (uint32_t)p->height - 1, 16);
    put_render_size(w, p);
}

static void put_lf_delta(bit_writer *w, int delta, int last) { /* encode_loopfilter, :703-723 */
    const int changed = delta != last;
    put_bit(w, changed);
    if (changed) {
        put_literal(w, (uint32_t)(delta < 0 ? -delta : delta) & 0x3F, 6);
        put_bit(w, delta < 0);
    }
}
static void put_delta_q(bit_writer *w, int dq) { /* write_delta_q, :728-736 */
    put_bit(w, dq != 0);
    if (dq) {
        put_literal(w, (uint32_t)(dq < 0 ? -dq : dq), 4);
        put_bit(w, dq < 0);
    }
}

static int in_range(int v, int lo, int hi) { return v >= lo && v <= hi; }

static int params_ok(const svt_frame_params *p) {
    const uint8_t flags[] = {p->show_frame, p->error_resilient_mode, p->intra_only, p->refresh_frame_context, p->frame_parallel_decoding_mode,
                             p->ref_frame_sign_bias[0], p->ref_frame_sign_bias[1], p->ref_frame_sign_bias[2], p->ref_frame_sign_bias[3], p->allow_hp,
                             p->allow_comp_inter_inter, p->color_range, p->mode_ref_delta_enabled, p->mode_ref_delta_update};
    for (unsigned i = 0; i < sizeof flags; i++)
        if (flags[i] > 1) return 0;
    if (p->frame_type > 1 || p->reset_frame_context > 3 || p->frame_context_idx > 3 || p->reference_mode > SVT_MODES_REFERENCE_SELECT) return 0;
    for (int i = 0; i < 3; i++)
        if (p->ref_dpb_index[i] > 7) return 0;
    if (p->color_space > 6) return 0; /* 7 = SRGB: profile 1 */
    /* beyond 64 SB columns eb_vp9_get_tile_n_bits gives min_log2_tile_cols > 0 (VPX/vp9_tile_common.c:40-57): one tile column is not codable */
    if (!in_range(p->width, 1, 4096) || !in_range(p->height, 1, 65536) || !in_range(p->render_width, 1, 65536) || !in_range(p->render_height, 1, 65536)) return 0;
    if (p->filter_level > 63 || p->sharpness_level > 7) return 0;
    for (int i = 0; i < 4; i++)
        if (!in_range(p->ref_deltas[i], -63, 63) || !in_range(p->last_ref_deltas[i], -63, 63)) return 0;
    for (int i = 0; i < 2; i++)
        if (!in_range(p->mode_deltas[i], -63, 63) || !in_range(p->last_mode_deltas[i], -63, 63)) return 0;
    if (!in_range(p->y_dc_delta_q, -15, 15) || !in_range(p->uv_dc_delta_q, -15, 15) || !in_range(p->uv_ac_delta_q, -15, 15)) return 0;
    /* intra_only is coded only when show_frame is 0 (:1220-1221): a decoder takes it as 0 otherwise */
    if (p->frame_type != 0 && p->show_frame && p->intra_only) return 0;
    return 1;
}

/* write_uncompressed_header (:1186-1290) and the 16 bits of first_part_size behind it; returns the bit position of those 16 bits */
static uint32_t uncompressed_header(bit_writer *w, const svt_frame_params *p) {
    put_literal(w, 2, 2); /* VP9_FRAME_MARKER */
    put_literal(w, 0, 2); /* profile 0 */
    put_bit(w, 0);        /* show_existing_frame */
    put_bit(w, p->frame_type);
    put_bit(w, p->show_frame);
    put_bit(w, p->error_resilient_mode);
    if (p->frame_type == 0) {
        put_sync_code(w);
        put_literal(w, p->color_space, 3); /* write_bitdepth_colorspace_sampling at profile 0: no bit depth, no subsampling */
        put_bit(w, p->color_range);
        put_frame_size(w, p);
    } else {
        if (!p->show_frame) put_bit(w, p->intra_only);
        if (!p->error_resilient_mode) put_literal(w, p->reset_frame_context, 2);
        if (p->intra_only) {
            put_sync_code(w); /* profile 0: 4:2:0 8 bit is assumed, nothing more */
            put_literal(w, p->refresh_frame_mask, 8);
            put_frame_size(w, p);
        } else {
            put_literal(w, p->refresh_frame_mask, 8);
            for (int r = 0; r < 3; r++) {
                put_literal(w, p->ref_dpb_index[r], 3);
                put_bit(w, p->ref_frame_sign_bias[1 + r]);
            }
            for (int r = 0; r < 3; r++) put_bit(w, 0); /* write_frame_size_with_refs: found = 0 for every reference */
            put_literal(w, (uint32_t)p->width - 1, 16);
            put_literal(w, (uint32_t)p->height - 1, 16);
            put_render_size(w, p);
            put_bit(w, p->allow_hp);
            put_bit(w, 0);        /* write_interp_filter(0, ..): not switchable, */
            put_literal(w, 1, 2); /* filter_to_literal[0] */
        }
    }
    if (!p->error_resilient_mode) {
        put_bit(w, p->refresh_frame_context);
        put_bit(w, p->frame_parallel_decoding_mode);
    }
    put_literal(w, p->frame_context_idx, 2);
    /* encode_loopfilter (:689-726) */
    put_literal(w, p->filter_level, 6);
    put_literal(w, p->sharpness_level, 3);
    put_bit(w, p->mode_ref_delta_enabled);
    if (p->mode_ref_delta_enabled) {
        put_bit(w, p->mode_ref_delta_update);
        if (p->mode_ref_delta_update) {
            for (int i = 0; i < 4; i++) put_lf_delta(w, p->ref_deltas[i], p->last_ref_deltas[i]);
            for (int i = 0; i < 2; i++) put_lf_delta(w, p->mode_deltas[i], p->last_mode_deltas[i]);
        }
    }
    /* encode_quantization (:738-743) */
    put_literal(w, p->base_qindex, 8);
    put_delta_q(w, p->y_dc_delta_q);
    put_delta_q(w, p->uv_dc_delta_q);
    put_delta_q(w, p->uv_ac_delta_q);
    put_bit(w, 0); /* encode_segmentation: off */
    /* write_tile_info (:870-885) at log2_tile_cols = 0 with min_log2_tile_cols = 0: a 0 when more columns were possible, i.e. when
       max_log2_tile_cols > 0: (sb64_cols >> 1) >= MIN_TILE_WIDTH_B64 = 4; then log2_tile_rows = 0 */
    const int sb64_cols = (((p->width + 7) >> 3) + 7) >> 3;
    if (sb64_cols >= 8) put_bit(w, 0);
    put_bit(w, 0);
    const uint32_t at = w->bits;
    put_literal(w, 0, 16);
    return at;
}

/* write_compressed_header (:1292-1367) as bool records, in two parts: what stands in front of update_coef_probs and what stands behind
 * it; together with the section in between at most SVT_FRAME_COMPRESSED_MAX_BOOLS when the section is four "no update" bits */
static void compressed_parts(const svt_frame_params *p, uint16_t *b, uint32_t *n_prefix, uint16_t *suffix, uint32_t *n_suffix) {
    uint32_t n = 0;
#define LITERAL_BIT(bit) (b[n++] = SVT_BOOL_RECORD((bit), 128))
#define NO_UPDATE(count) do { for (int k_ = 0; k_ < (count); k_++) b[n++] = SVT_BOOL_RECORD(0, 252); } while (0)
    LITERAL_BIT(1); LITERAL_BIT(1); /* encode_txfm_probs: min(tx_mode, ALLOW_32X32) = 3, */
    LITERAL_BIT(0);                 /* not TX_MODE_SELECT */
    *n_prefix = n;
    b = suffix; n = 0;              /* update_coef_probs stands here */
    NO_UPDATE(3);                   /* update_skip_probs */
    if (p->frame_type != 0 && !p->intra_only) {
        NO_UPDATE(7 * 3);           /* inter_mode_probs */
        NO_UPDATE(4);               /* intra_inter_prob */
        if (p->allow_comp_inter_inter) {
            const int compound = p->reference_mode != SVT_MODES_SINGLE_REFERENCE, hybrid = p->reference_mode == SVT_MODES_REFERENCE_SELECT;
            LITERAL_BIT(compound);
            if (compound) {
                LITERAL_BIT(hybrid);
                if (hybrid) NO_UPDATE(5); /* comp_inter_prob */
            }
        }
        if (p->reference_mode != SVT_MODES_COMPOUND_REFERENCE) NO_UPDATE(5 * 2); /* single_ref_prob */
        if (p->reference_mode != SVT_MODES_SINGLE_REFERENCE) NO_UPDATE(5);       /* comp_ref_prob */
        NO_UPDATE(4 * 9);           /* y_mode_prob */
        NO_UPDATE(16 * 3);          /* partition_prob */
        /* eb_vp9_write_nmv_probs (VPX/vp9_encodemv.c:169-199): joints; per component sign, classes, class0, bits; per component
           class0_fp, fp; with allow_hp per component class0_hp, hp */
        NO_UPDATE(3 + 2 * (1 + 10 + 1 + 10) + 2 * (2 * 3 + 3));
        if (p->allow_hp) NO_UPDATE(2 * 2);
    }
#undef LITERAL_BIT
#undef NO_UPDATE
    *n_suffix = n;
}

int32_t svt_hip_frame_header_parts_host(const svt_frame_params *p, uint16_t *prefix, uint32_t *n_prefix, uint16_t *suffix, uint32_t *n_suffix) {
    if (!p || !prefix || !n_prefix || !suffix || !n_suffix || !params_ok(p)) return SVT_HIP_ERR_BAD_PARAMETER;
    compressed_parts(p, prefix, n_prefix, suffix, n_suffix);
    return SVT_HIP_OK;
}

/* the uncompressed header, then the compressed header coded from the given records, first_part_size from the coder's answer */
static int32_t header_from_bools(const svt_frame_params *p, const uint16_t *bools, uint32_t n, uint8_t *out, uint32_t capacity, uint32_t *uncompressed_bytes,
                                 uint32_t *compressed_bytes) {
    static const svt_bool_tables no_tables; /* the stream has no token records: never read */
    bit_writer w;
    memset(&w, 0, sizeof w);
    const uint32_t at = uncompressed_header(&w, p), ub = (w.bits + 7) >> 3;
    if (ub > capacity) return SVT_HIP_ERR_BAD_PARAMETER;
    const svt_bool_segment seg = {0, n, 1};
    uint32_t               cb = 0;
    const int32_t          rc = svt_hip_boolcode_host(&no_tables, NULL, 0, bools, n, &seg, 1, out + ub, capacity - ub, &cb);
    if (rc) return rc;
    if (cb > 0xffff || cb > capacity - ub) return SVT_HIP_ERR_BAD_PARAMETER;
    for (uint32_t t = 0; t < ub; t++) out[t] = svt_frame_size_field_byte(w.buf[t], t, at, cb); /* first_part_size over its place holder */
    *uncompressed_bytes = ub;
    *compressed_bytes = cb;
    return SVT_HIP_OK;
}

int32_t svt_hip_frame_header_host(const svt_frame_params *p, uint8_t *out, uint32_t capacity, uint32_t *uncompressed_bytes, uint32_t *compressed_bytes) {
    if (!p || !out || !uncompressed_bytes || !compressed_bytes || !params_ok(p)) return SVT_HIP_ERR_BAD_PARAMETER;
    uint16_t bools[SVT_FRAME_COMPRESSED_MAX_BOOLS], suffix[SVT_FRAME_COMPRESSED_MAX_BOOLS];
    uint32_t n = 0, ns = 0;
    compressed_parts(p, bools, &n, suffix, &ns);
    for (int t = 0; t < 4; t++) bools[n++] = SVT_BOOL_RECORD(0, 128); /* update_coef_probs: tx_totals <= 20 for TX_4X4 .. TX_32X32 */
    memcpy(bools + n, suffix, sizeof(uint16_t) * ns);
    uint8_t  hdr[SVT_FRAME_HEADER_MAX + 8];
    uint32_t ub = 0, cb = 0;
    const int32_t rc = header_from_bools(p, bools, n + ns, hdr, sizeof hdr, &ub, &cb);
    if (rc) return rc;
    if (cb > SVT_FRAME_COMPRESSED_MAX || ub + cb > capacity) return SVT_HIP_ERR_BAD_PARAMETER;
    memcpy(out, hdr, ub + cb);
    *uncompressed_bytes = ub;
    *compressed_bytes = cb;
    return SVT_HIP_OK;
}

int32_t svt_hip_frame_header_coef_host(const svt_frame_params *p, const uint16_t *hdr_bools, uint32_t n_hdr_bools, uint8_t *out, uint32_t capacity,
                                       uint32_t *uncompressed_bytes, uint32_t *compressed_bytes) {
    if (!p || !hdr_bools || !out || !uncompressed_bytes || !compressed_bytes || !params_ok(p)) return SVT_HIP_ERR_BAD_PARAMETER;
    return header_from_bools(p, hdr_bools, n_hdr_bools, out, capacity, uncompressed_bytes, compressed_bytes);
}

int32_t svt_hip_frame_header_uncompressed_host(const svt_frame_params *p, uint8_t *out, uint32_t capacity, uint32_t *bytes, uint32_t *size_bit) {
    if (!p || !out || !bytes || !size_bit || !params_ok(p)) return SVT_HIP_ERR_BAD_PARAMETER;
    bit_writer w;
    memset(&w, 0, sizeof w);
    const uint32_t at = uncompressed_header(&w, p), ub = (w.bits + 7) >> 3;
    if (ub > capacity) return SVT_HIP_ERR_BAD_PARAMETER;
    memcpy(out, w.buf, ub);
    *bytes = ub;
    *size_bit = at;
    return SVT_HIP_OK;
}

int32_t svt_hip_frame_show_existing_host(int32_t dpb_slot, uint8_t *out) {
    if (!out || dpb_slot < 0 || dpb_slot > 7) return SVT_HIP_ERR_BAD_PARAMETER;
    *out = (uint8_t)(0x88 | dpb_slot); /* frame marker 10, profile 00, show_existing_frame 1, the slot's 3 bits */
    return SVT_HIP_OK;
}

int32_t svt_frame_check_packets(int32_t n_pics, const svt_frame_packet *pk) {
    if (!pk || n_pics < 1 || n_pics > SVT_FRAME_MAX_PICS) return SVT_HIP_ERR_BAD_PARAMETER;
    for (int i = 0; i < n_pics; i++)
        if (!pk[i].d_tile_size || (!pk[i].d_tile && pk[i].tile_capacity) || pk[i].header_len > SVT_FRAME_HEADER_MAX || pk[i].trailer_len > 4)
            return SVT_HIP_ERR_BAD_PARAMETER;
    return SVT_HIP_OK;
}

int32_t svt_hip_frame_assemble_host(int32_t n_pics, const svt_frame_packet *pk, uint8_t *arena, uint32_t arena_capacity, svt_frame_entry *table) {
    if (svt_frame_check_packets(n_pics, pk) || !table || (!arena && arena_capacity)) return SVT_HIP_ERR_BAD_PARAMETER;
    uint32_t sizes[SVT_FRAME_MAX_PICS], none;
    for (int i = 0; i < n_pics; i++) sizes[i] = svt_frame_packet_size(pk[i].header_len, pk[i].trailer_len, *pk[i].d_tile_size, pk[i].tile_capacity);
    for (int i = 0; i < n_pics; i++) {
        const uint32_t off = svt_frame_layout(sizes, i, &none);
        table[i].offset = off;
        table[i].size = sizes[i];
        if (sizes[i] == SVT_FRAME_SIZE_NONE) continue;
        const uint32_t tile = *pk[i].d_tile_size;
        uint64_t       pos = off;
        uint32_t       n = svt_frame_span(pos, pk[i].header_len, arena_capacity);
        if (n) memcpy(arena + pos, pk[i].header, n);
        pos += pk[i].header_len;
        n = svt_frame_span(pos, tile, arena_capacity);
        if (n) memcpy(arena + pos, pk[i].d_tile, n);
        pos += tile;
        n = svt_frame_span(pos, pk[i].trailer_len, arena_capacity);
        if (n) memcpy(arena + pos, pk[i].trailer, n);
    }
    table[n_pics].offset = svt_frame_layout(sizes, n_pics, &none);
    table[n_pics].size = none;
    return SVT_HIP_OK;
}

int32_t svt_frame_check_parts(int32_t n_pics, const svt_frame_parts_packet *pk) {
    if (!pk || n_pics < 1 || n_pics > SVT_FRAME_MAX_PICS) return SVT_HIP_ERR_BAD_PARAMETER;
    for (int i = 0; i < n_pics; i++)
        if (!pk[i].d_tile_size || !pk[i].d_compressed_size || (!pk[i].d_tile && pk[i].tile_capacity) || (!pk[i].d_compressed && pk[i].compressed_capacity) ||
            pk[i].header_len > SVT_FRAME_UNCOMPRESSED_MAX || (uint32_t)pk[i].size_bit + 16 > 8u * pk[i].header_len || pk[i].trailer_len > 4)
            return SVT_HIP_ERR_BAD_PARAMETER;
    return SVT_HIP_OK;
}

int32_t svt_hip_frame_assemble_parts_host(int32_t n_pics, const svt_frame_parts_packet *pk, uint8_t *arena, uint32_t arena_capacity, svt_frame_entry *table) {
    if (svt_frame_check_parts(n_pics, pk) || !table || (!arena && arena_capacity)) return SVT_HIP_ERR_BAD_PARAMETER;
    uint32_t sizes[SVT_FRAME_MAX_PICS], none;
    for (int i = 0; i < n_pics; i++)
        sizes[i] = svt_frame_parts_size(pk[i].header_len, pk[i].trailer_len, *pk[i].d_compressed_size, pk[i].compressed_capacity, *pk[i].d_tile_size, pk[i].tile_capacity);
    for (int i = 0; i < n_pics; i++) {
        const uint32_t off = svt_frame_layout(sizes, i, &none);
        table[i].offset = off;
        table[i].size = sizes[i];
        if (sizes[i] == SVT_FRAME_SIZE_NONE) continue;
        const uint32_t comp = *pk[i].d_compressed_size, tile = *pk[i].d_tile_size;
        uint64_t       pos = off;
        uint32_t       n = svt_frame_span(pos, pk[i].header_len, arena_capacity);
        for (uint32_t t = 0; t < n; t++) arena[pos + t] = svt_frame_size_field_byte(pk[i].header[t], t, pk[i].size_bit, comp);
        pos += pk[i].header_len;
        n = svt_frame_span(pos, comp, arena_capacity);
        if (n) memcpy(arena + pos, pk[i].d_compressed, n);
        pos += comp;
        n = svt_frame_span(pos, tile, arena_capacity);
        if (n) memcpy(arena + pos, pk[i].d_tile, n);
        pos += tile;
        n = svt_frame_span(pos, pk[i].trailer_len, arena_capacity);
        if (n) memcpy(arena + pos, pk[i].trailer, n);
    }
    table[n_pics].offset = svt_frame_layout(sizes, n_pics, &none);
    table[n_pics].size = none;
    return SVT_HIP_OK;
}

/*
 * ref_frame_driver.c -- runs the REFERENCE's eb_vp9_pack_bitstream (VPX/vp9_bitstream.c:1369-1412: write_uncompressed_header,
 * first_part_size, write_compressed_header, the copy of the entropy coder's stream) on stub PictureControlSet / VP9_COMP structures
 * and writes the frames it produced.  cm->fc comes from eb_vp9_default_coef_probs, eb_vp9_init_mode_probs and eb_vp9_init_mv_probs; the
 * counts are zero, as Codec/EbResourceCoordinationProcess.c:666 leaves them; profile 0, segmentation off, one tile, tx_mode
 * ALLOW_32X32, as the reference's encoder sets them.  Compiled by tests/gen_golden_frame.py against the reference's headers and linked
 * with the reference's own objects; the translation units the oracle's object set lacks are compiled into this one by the includes
 * below (both header writers are static there).  Nothing of the reference is copied here.
 *
 * While it runs, the driver notes from the reference's own structures (and with frame_is_intra_only and eb_vp9_get_tile_n_bits) which
 * branches of the two header writers each case takes, so that the generator can assert the fixture's coverage on the reference's side.
 *
 * request : int32 magic, n_cases; per case int32 show_existing (then int32 slot and nothing else), or 0 and N_VALUES int32 in the order
 *           of tests/frame_model.py:FIELDS, int32 tile_bytes, the tile's bytes
 * response: per case uint32 size, the frame's bytes, uint32 bytes of the uncompressed header (first_part_size included), uint32
 *           first_part_size as written; then 2 uint32 of coverage masks (enum ucov, enum ccov)
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

#define N_VALUES 45
#define LAST_DELTAS_AT 35 /* last_ref_deltas among the values */

enum ucov { U_KEY, U_INTRA_ONLY, U_INTER, U_HIDDEN, U_SHOWN, U_RESILIENT_0, U_RESILIENT_1, U_RENDER_SAME, U_RENDER_DIFFERS, U_LF_DELTAS_OFF, U_LF_NO_UPDATE,
            U_LF_UPDATE, U_LF_CHANGED_POS, U_LF_CHANGED_NEG, U_LF_UNCHANGED, U_DQ_ZERO, U_DQ_NEG, U_DQ_POS, U_TILE_BIT_0, U_TILE_BIT_1, U_SHOW_EXISTING, U_COUNT };
enum ccov { C_INTRA, C_INTER, C_COMP_NOT_ALLOWED, C_COMP_SINGLE, C_COMP_COMPOUND, C_COMP_HYBRID, C_SINGLE_REFS, C_NO_SINGLE_REFS, C_COMP_REFS, C_NO_COMP_REFS, C_HP_0,
            C_HP_1, C_COUNT };

static void note(const VP9_COMP *cpi, uint32_t cov[2]) {
    const VP9_COMMON *cm = &cpi->common;
    int               lo, hi;
    cov[0] |= 1u << (cm->frame_type == KEY_FRAME ? U_KEY : cm->intra_only ? U_INTRA_ONLY : U_INTER);
    if (cm->frame_type != KEY_FRAME) cov[0] |= 1u << (cm->show_frame ? U_SHOWN : U_HIDDEN);
    cov[0] |= 1u << (cm->error_resilient_mode ? U_RESILIENT_1 : U_RESILIENT_0);
    cov[0] |= 1u << (cm->width != cm->render_width || cm->height != cm->render_height ? U_RENDER_DIFFERS : U_RENDER_SAME);
    cov[0] |= 1u << (!cm->lf.mode_ref_delta_enabled ? U_LF_DELTAS_OFF : cm->lf.mode_ref_delta_update ? U_LF_UPDATE : U_LF_NO_UPDATE);
    if (cm->lf.mode_ref_delta_enabled && cm->lf.mode_ref_delta_update)
        for (int i = 0; i < MAX_REF_LF_DELTAS + MAX_MODE_LF_DELTAS; i++) {
            const int d = i < MAX_REF_LF_DELTAS ? cm->lf.ref_deltas[i] : cm->lf.mode_deltas[i - MAX_REF_LF_DELTAS];
            const int l = i < MAX_REF_LF_DELTAS ? cm->lf.last_ref_deltas[i] : cm->lf.last_mode_deltas[i - MAX_REF_LF_DELTAS];
            cov[0] |= 1u << (d == l ? U_LF_UNCHANGED : d < 0 ? U_LF_CHANGED_NEG : U_LF_CHANGED_POS);
        }
    const int dq[3] = {cm->y_dc_delta_q, cm->uv_dc_delta_q, cm->uv_ac_delta_q};
    for (int i = 0; i < 3; i++) cov[0] |= 1u << (dq[i] == 0 ? U_DQ_ZERO : dq[i] < 0 ? U_DQ_NEG : U_DQ_POS);
    eb_vp9_get_tile_n_bits(cm->mi_cols, &lo, &hi);
    if (lo != 0) exit(30); /* one tile column is not codable: the product refuses such a width */
    cov[0] |= 1u << (cm->log2_tile_cols < hi ? U_TILE_BIT_1 : U_TILE_BIT_0);
    if (frame_is_intra_only(cm)) { cov[1] |= 1u << C_INTRA; return; }
    cov[1] |= 1u << C_INTER;
    cov[1] |= 1u << (!cpi->allow_comp_inter_inter ? C_COMP_NOT_ALLOWED : cm->reference_mode == SINGLE_REFERENCE ? C_COMP_SINGLE :
                     cm->reference_mode == REFERENCE_MODE_SELECT ? C_COMP_HYBRID : C_COMP_COMPOUND);
    cov[1] |= 1u << (cm->reference_mode != COMPOUND_REFERENCE ? C_SINGLE_REFS : C_NO_SINGLE_REFS);
    cov[1] |= 1u << (cm->reference_mode != SINGLE_REFERENCE ? C_COMP_REFS : C_NO_COMP_REFS);
    cov[1] |= 1u << (cm->allow_high_precision_mv ? C_HP_1 : C_HP_0);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2 || hdr[0] != 0x4d415246) return 4;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 5;

    VP9_COMP                *cpi = calloc(1, sizeof *cpi);
    VP9_COMMON              *cm = &cpi->common;
    PictureControlSet       *pcs = calloc(1, sizeof *pcs);
    PictureParentControlSet *ppcs = calloc(1, sizeof *ppcs);
    EntropyCoder            *ec = calloc(1, sizeof *ec);
    OutputBitstreamUnit     *unit = calloc(1, sizeof *unit);
    uint32_t                 cov[2] = {0, 0};
    if (!cpi || !pcs || !ppcs || !ec || !unit) return 6;
    pcs->parent_pcs_ptr = ppcs;
    pcs->entropy_coder_ptr = ec;
    ec->ec_output_bitstream_ptr = (EbPtr)unit;
    cm->fc = calloc(1, sizeof *cm->fc);
    cpi->td.counts = calloc(1, sizeof *cpi->td.counts); /* zero: Codec/EbResourceCoordinationProcess.c:666 */
    eb_vp9_entropy_mv_init();

    for (int k = 0; k < hdr[1]; k++) {
        int32_t  show_existing, v[N_VALUES], tile_bytes = 0;
        uint8_t *tile = NULL;
        if (fread(&show_existing, 4, 1, f) != 1) return 7;
        uint8_t *dest = NULL;
        size_t   size = 0;
        uint32_t ub = 0, first_part = 0;
        if (show_existing) {
            int32_t slot;
            if (fread(&slot, 4, 1, f) != 1 || slot < 0 || slot > 7) return 8;
            ppcs->show_existing_frame_index_array[2] = (uint8_t)slot;
            dest = calloc(1, 64);
            eb_vp9_pack_bitstream(pcs, cpi, dest, &size, 1, 2);
            cov[0] |= 1u << U_SHOW_EXISTING;
        } else {
            if (fread(v, 4, N_VALUES, f) != N_VALUES || fread(&tile_bytes, 4, 1, f) != 1 || tile_bytes < 0) return 9;
            tile = malloc((size_t)tile_bytes + 1);
            if (fread(tile, 1, (size_t)tile_bytes, f) != (size_t)tile_bytes) return 10;
            const int32_t *p = v;
            /* the frame context a picture is coded with, and the tables every update is measured against */
            eb_vp9_init_mode_probs(cm->fc);
            eb_vp9_init_mv_probs(cm);
            eb_vp9_default_coef_probs(cm);
            memset(cpi->td.counts, 0, sizeof *cpi->td.counts);
            memset(&cm->counts, 0, sizeof cm->counts);
            cm->profile = PROFILE_0; cm->bit_depth = VPX_BITS_8; cm->subsampling_x = 1; cm->subsampling_y = 1;
            cm->tx_mode = ALLOW_32X32; cm->seg.enabled = 0; cm->log2_tile_cols = 0; cm->log2_tile_rows = 0;
            cm->frame_type = (FRAME_TYPE)*p++; cm->show_frame = *p++; cm->error_resilient_mode = *p++; cm->intra_only = *p++;
            cm->reset_frame_context = *p++; cm->refresh_frame_context = *p++; cm->frame_parallel_decoding_mode = *p++; cm->frame_context_idx = *p++;
            ppcs->ref_signal.refresh_frame_mask = (uint8_t)*p++;
            for (int i = 0; i < 3; i++) ppcs->ref_signal.ref_dpb_index[i] = (uint8_t)*p++;
            for (int i = 0; i < 4; i++) cm->ref_frame_sign_bias[i] = *p++;
            cm->allow_high_precision_mv = *p++; cm->reference_mode = (REFERENCE_MODE)*p++; cpi->allow_comp_inter_inter = *p++;
            cm->color_space = (vpx_color_space_t)*p++; cm->color_range = (vpx_color_range_t)*p++;
            cm->width = *p++; cm->height = *p++; cm->render_width = *p++; cm->render_height = *p++;
            cm->mi_cols = (cm->width + 7) >> 3; cm->mi_rows = (cm->height + 7) >> 3; /* eb_vp9_set_mb_mi */
            cm->lf.filter_level = *p++; cm->lf.sharpness_level = *p++; cm->lf.mode_ref_delta_enabled = (uint8_t)*p++; cm->lf.mode_ref_delta_update = (uint8_t)*p++;
            for (int i = 0; i < 4; i++) cm->lf.ref_deltas[i] = (signed char)*p++;
            for (int i = 0; i < 2; i++) cm->lf.mode_deltas[i] = (signed char)*p++;
            for (int i = 0; i < 4; i++) cm->lf.last_ref_deltas[i] = (signed char)*p++;
            for (int i = 0; i < 2; i++) cm->lf.last_mode_deltas[i] = (signed char)*p++;
            cm->base_qindex = *p++; cm->y_dc_delta_q = *p++; cm->uv_dc_delta_q = *p++; cm->uv_ac_delta_q = *p++;
            if (p != v + N_VALUES) return 11;
            note(cpi, cov);
            ec->residual_bc.pos = (unsigned int)tile_bytes;
            unit->buffer_begin = tile;
            dest = calloc(1, (size_t)tile_bytes + 4096);
            memset(dest, 0xEE, (size_t)tile_bytes + 4096); /* (a byte the writers leave untouched would show) */
            eb_vp9_pack_bitstream(pcs, cpi, dest, &size, 0, 0);
            /* the tile lies at the frame's end; the uncompressed header's length from the reference's own writer, run once more on a
               scratch buffer with the loop-filter state the first run advanced put back */
            if (size < (size_t)tile_bytes + 3 || memcmp(dest + size - tile_bytes, tile, (size_t)tile_bytes)) return 12;
            struct vpx_write_bit_buffer wb = {calloc(1, 4096), 0};
            p = v + LAST_DELTAS_AT;
            for (int i = 0; i < 4; i++) cm->lf.last_ref_deltas[i] = (signed char)*p++;
            for (int i = 0; i < 2; i++) cm->lf.last_mode_deltas[i] = (signed char)*p++;
            write_uncompressed_header(pcs, cpi, &wb, 0, 0);
            eb_vp9_wb_write_literal(&wb, 0, 16);
            ub = (uint32_t)eb_vp9_wb_bytes_written(&wb);
            for (size_t b = wb.bit_offset - 16; b < wb.bit_offset; b++) first_part = first_part << 1 | ((dest[b >> 3] >> (7 - (b & 7))) & 1u); /* as written into the frame */
            if ((size_t)ub + first_part + (size_t)tile_bytes != size) return 13;
            free(wb.bit_buffer);
        }
        const uint32_t s32 = (uint32_t)size;
        fwrite(&s32, 4, 1, out);
        fwrite(dest, 1, size, out);
        fwrite(&ub, 4, 1, out);
        fwrite(&first_part, 4, 1, out);
        free(dest);
        free(tile);
    }
    fwrite(cov, 4, 2, out);
    fclose(f);
    fclose(out);
    return 0;
}

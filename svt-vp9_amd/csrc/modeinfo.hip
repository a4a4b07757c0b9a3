/*
 * modeinfo.hip -- the key-frame mode-info syntax of batches of pictures (gfx950), a stage of syntax_stage.h's count -> scan -> emit
 * skeleton.
 *
 * Replaces, for intra-only pictures, write_partition and write_mb_modes_kf as eb_vp9_entropy_coding_kernel calls them per block in
 * front of pack_mb_tokens (Codec/EbEntropyCodingProcess.c:110-442, Source/Lib/VPX/vp9_bitstream.c:323-417).
 *
 * The reference walks SBs and their quad-trees serially and carries above / left context arrays, but every context is a function of
 * the grid alone (modeinfo_core.h), and the bools of a unit are a function of its own record and its two neighbours'.  The count needs
 * neither the neighbours nor probabilities.  A wave's part of LDS holds 64 units x SVT_MI_UNIT_BOOLS (48) records = 6 144 bytes; four
 * waves a workgroup = 24 576 bytes.
 */
#include "syntax_stage.h"

namespace {

struct mi_stage {
    typedef svt_modes_picture       picture;
    typedef const svt_lf_mode_info *view;
    typedef svt_modes_tables        tables;
    static constexpr int         UNIT_BOOLS = SVT_MI_UNIT_BOOLS, EMIT_WAVES = 4, SCRATCH_SLOT = SVT_SLOT_MI_SB_OFF, TABLES_SLOT = SVT_SLOT_MI_TABLES;
    static constexpr const char *NAME = "modes";
    static __device__ __forceinline__ int check(const view &v, const svt_tok_geom *g, int r, int c) { return svt_mi_check(v, g, r, c); }
    static __device__ __forceinline__ int unit_bools(const view &v, const svt_tok_geom *g, int r, int c, const tables *t, uint16_t *out) { return svt_mi_unit_bools(v, g, r, c, t, out); }
    static __device__ __forceinline__ const svt_lf_mode_info *grid(const view &v) { return v; }
    static const char *fill(const picture &p, syn_pic_dev<mi_stage> &P) {
        P.v = p.d_lf_mi;
        return syn_fill_common(p, P, !p.d_lf_mi);
    }
};

} // namespace

extern "C" int32_t svt_hip_modes_set_tables(svt_hip_ctx *ctx, const svt_modes_tables *tables) { return syn_set_tables<mi_stage>(ctx, tables); }

extern "C" int32_t svt_hip_modes_kf_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_modes_picture *pics, int32_t width, int32_t height, int32_t mi_stride) {
    return syn_batch_device<mi_stage>(ctx, n_pics, pics, width, height, mi_stride);
}

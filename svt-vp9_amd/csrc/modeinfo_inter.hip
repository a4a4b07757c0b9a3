/*
 * modeinfo_inter.hip -- the mode-info syntax of batches of inter pictures (gfx950), a stage of syntax_stage.h's count -> scan -> emit
 * skeleton.  The counterpart of modeinfo.hip for every picture that is not intra-only.
 *
 * Replaces write_partition and pack_inter_mode_mvs as eb_vp9_entropy_coding_kernel calls them per block in front of pack_mb_tokens
 * (Codec/EbEntropyCodingProcess.c:60-449, Source/Lib/VPX/vp9_bitstream.c:206-321, 399-417).
 *
 * Every context is a function of the grids (modeinfo_inter_core.h), and the bools of a unit are a function of its own records and its
 * two neighbours'.  The count reads no probabilities and no neighbours: the MV differences decide joint, class, fraction and the
 * high-precision bit; the emit pass derives the neighbours' contexts.
 * A wave's part of LDS holds 64 units x SVT_MII_UNIT_BOOLS (111) records = 14 208 bytes; two waves a workgroup = 28 416 bytes, so the
 * 160 KB of a CU hold five workgroups = ten waves (four waves a workgroup: two workgroups = eight waves).
 */
#include "syntax_stage.h"
#include "modeinfo_inter_core.h"

namespace {

struct mii_stage {
    typedef svt_modes_inter_picture picture;
    typedef svt_mii_view            view;
    typedef svt_modes_inter_tables  tables;
    static constexpr int         UNIT_BOOLS = SVT_MII_UNIT_BOOLS, EMIT_WAVES = 2, SCRATCH_SLOT = SVT_SLOT_MII_SB_OFF, TABLES_SLOT = SVT_SLOT_MII_TABLES;
    static constexpr const char *NAME = "modes_inter";
    static __device__ __forceinline__ int check(const view &v, const svt_tok_geom *g, int r, int c) { return svt_mii_check(&v, g, r, c); }
    static __device__ __forceinline__ int unit_bools(const view &v, const svt_tok_geom *g, int r, int c, const tables *t, uint16_t *out) { return svt_mii_unit_bools(&v, g, r, c, t, out); }
    static __device__ __forceinline__ const svt_lf_mode_info *grid(const view &v) { return v.mi; }
    static const char *fill(const picture &p, syn_pic_dev<mii_stage> &P) {
        if (const char *what = syn_fill_common(p, P, !p.d_lf_mi || !p.d_mc_mi || !p.d_ext)) return what;
        P.v.mi = p.d_lf_mi; P.v.mc = p.d_mc_mi; P.v.ext = p.d_ext; P.v.f = svt_mii_frame_of(&p);
        return svt_mii_bad_frame(&P.v.f) ? "reference_mode above 2, or a compound reference outside 1 .. 3" : nullptr;
    }
};

} // namespace

extern "C" int32_t svt_hip_modes_inter_set_tables(svt_hip_ctx *ctx, const svt_modes_inter_tables *tables) { return syn_set_tables<mii_stage>(ctx, tables); }

extern "C" int32_t svt_hip_modes_inter_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_modes_inter_picture *pics, int32_t width, int32_t height,
                                                    int32_t mi_stride) {
    return syn_batch_device<mii_stage>(ctx, n_pics, pics, width, height, mi_stride);
}

/* me_types.h -- what every ME file shares: the picture descriptor, the LDS layout and per-SB state, the phase context, and the
 * motion-vector / PU / search-area geometry helpers.  me_layout.h needs no more than this. */
#ifndef SVT_ME_TYPES_H
#define SVT_ME_TYPES_H
#include "me_prims.h"

#define ME_SB 64
#define ME_MAX_SAD_VALUE (64 * 64 * 255)

/* Picture descriptor as seen by the kernel (device pointers inside the planes). */
typedef struct me_pic_dev {
    svt_pa_picture    cur, ref[2];
    svt_me_pu_result *results;
    uint32_t         *rcme;
    /* the parameters that change from picture to picture inside a configuration (me_spec.h) and what the host derives from
     * them (HME level-0 areas scaled by the temporal layer's multiplier): one launch serves pictures of several layers */
    uint8_t           num_ref_lists, temporal_layer_index, hierarchical_levels, same_ref_poc;
    int16_t           hme_w0[2], hme_h0[2], hme_tw0, hme_th0;
    int16_t           hme_band; /* me_fast.h: search rows of the (widest) level-0 window that fit the LDS scratch at a time */
} me_pic_dev;

/* LDS layout (byte offsets), computed on the host from the parameters (me_lds_layout) */
typedef struct me_lds_layout {
    int32_t off_state;   /* me_state_t */
    int32_t off_src;     /* 64 x 64 source SB, stride 64 */
    int32_t off_region;  /* integer reference samples of the current list's search region */
    int32_t off_planes;  /* B, H, J half-pel planes (3 x plane_bytes); aliased by HME window / SAD scratch */
    int32_t off_quarter; /* 32x32 quarter-resolution SB (only when HME level 1 is enabled) */
    int32_t off_ssd;     /* SSD_SEARCH only: candidate SSDs [85][9]; entry 8 of a PU is the integer position's, then the PU's best so far */
    int32_t off_cand;    /* sub-pel candidate distortions [pu][8] / bi-pred distortion [pu]: entries 0..167 (PUs 0..20), dwords */
    int32_t off_cand_hi; /* entries 168..679 (the 8x8 PUs: at most 2 x 64 x 255 each) as halfwords, when cand_dwords = 680; else -1 */
    int32_t cand_dwords; /* 8 x (21 when the 8x8 PUs are never refined nor bi-predicted, else 85) */
    int32_t off_pred0;   /* host emulation only (the kernel keeps them in registers): list 0 prediction of the bi-pred lanes */
    int32_t region_stride, region_rows;
    int32_t plane_stride; /* row stride of the half-pel planes: they are narrower than the region (no search tail) */
    int32_t plane_bytes;
    int32_t scratch_bytes; /* bytes available at off_planes */
    int32_t total_bytes;
    int32_t compact;     /* me_layout.h: no tail columns in the region rows, quarter SB inside the SSD tables */
    /* HME level-0 search areas already scaled by the temporal layer's multiplier (Codec/EbDefinitions.h:989-1005): the
     * divisions by 100 are done once per launch on the host instead of by the planning thread of every SB */
    int16_t hme_w0[2], hme_h0[2], hme_tw0, hme_th0;
} me_lds_layout;

#define ME_RGN_GX 4 /* left guard columns of the region buffer (search position 0 is dword aligned) */
#define ME_RGN_GY 3 /* top guard rows */
#define ME_PL_G 2   /* guard of the half-pel planes */

/* ---- HME work list: (region, band of search rows) windows staged in the scratch and searched batch by batch ---- */
#define ME_HME_MAX_WIN 16
typedef struct me_hme_win {
    int16_t  gx, gy;         /* reference-picture coordinates of window column 0 / row 0 */
    uint32_t off;            /* byte offset of the window inside the scratch (the scratch can exceed 64 KB: search areas up to 127 x 127) */
    uint16_t wstride;        /* window row stride (bytes, odd number of dwords) */
    uint16_t tl, ts;         /* first load task / first search task of this window inside its batch */
    uint16_t sw, sh;         /* search positions */
    uint16_t y0;             /* first search row of this window inside its region (row band offset) */
    uint16_t rows;           /* window rows */
    uint8_t  nd;             /* window dwords per row */
    uint8_t  slot;           /* region (key) this window belongs to */
    uint32_t inv_nu, inv_ng; /* me_magic_of(16-byte units per window row) / (search tasks per search row): the planning thread divides once */
} me_hme_win;

/* per-SB state in LDS */
typedef struct me_state_t {
    union {
        uint64_t key[85];      /* full-pel arg-min keys of the current list */
        struct {               /* HME work list: dead once the level's results are in hme_x/y/sad, before the keys are set */
            int32_t    hme_nbatch, hme_bstart[ME_HME_MAX_WIN + 1]; /* batches of windows that fit the scratch together */
            me_hme_win hme_win[ME_HME_MAX_WIN];
        };
    };
    uint64_t hme_key;          /* arg-min key of the stand-alone SAD-loop kernel */
    uint64_t hme_keys[4];      /* arg-min keys of the region searches of the current HME level */
    uint64_t hme_sad[3][4];    /* per level, per region slot (rh*2 + rw): best SAD * 2 */
    int16_t  hme_x[3][4], hme_y[3][4]; /* per level, per region slot: search centre in / best position out */
    int16_t  hme_cox[4], hme_coy[4], hme_cw[4], hme_ch[4]; /* clipped search areas of the current level */
    int16_t  hme_xc, hme_yc;   /* HME result; persists from list 0 to list 1 when no level runs */
    int32_t  hme_rh;           /* [quirk] the reference's region-row counter, not reset between the lists */
    uint32_t best_sad[2][85];  /* search (z-order) index */
    uint32_t best_mv[2][85];
    uint32_t red[8];           /* small sum reductions */
    uint32_t spu[85];          /* refined PUs of the current list, dense: pu | n << 7 | (px>>3) << 14 | (py>>3) << 17 | log2(w/8) << 20 */
    uint32_t supel[9];         /* su_pel_enable sums: sx,sy,ssad for 32/16/8 */
    svt_plane refd[3];         /* descriptors (full, 1/4, 1/16) of the current list's reference picture, copied from HBM once */
    uint8_t  dir[88];          /* 85 used; padded so that the block below stays dword aligned */
    /* rows 0,2,4.. of the 1/16-resolution SB, read as dwords by the HME search: a misaligned ds_read is replayed at ~64
     * cycles per wave-instruction (SQ_LDS_UNALIGNED_STALL was 2/3 of all LDS cycles of the kernel before this was aligned) */
    uint8_t  sixteenth_sb[16 * 8] __attribute__((aligned(16)));
} me_state_t;

/* everything a phase needs */
typedef struct me_ctx_t {
    const me_pic_dev    *pic;
    const svt_me_params *p;
    me_lds_layout        L;
    uint8_t             *lds;
    me_state_t          *st;
    uint8_t             *src;    /* LDS */
    uint8_t             *region; /* LDS */
    uint8_t             *planes; /* LDS */
    uint8_t             *hme_scratch; /* LDS: where the HME levels stage their windows -- the region buffer and the planes behind it, both dead while a list's
                                         hierarchical search runs (the region is staged after it, the planes are interpolated from the region) */
    int                  hme_scratch_bytes;
    uint8_t             *quarter_sb; /* LDS, valid when HME level 1 is enabled */
    uint32_t            *ssdc;       /* LDS, SSD_SEARCH only: SSD of the sub-pel candidates [pu][9] (8 = integer position) */
    uint32_t            *cand;       /* LDS: sub-pel candidate distortions [pu][8] (see me_cand_get); bi-pred distortion [pu] */
    uint32_t            *cand_hi;    /* LDS: the 8x8 PUs' entries of that table as halfwords (L.off_cand_hi >= 0: else they are never refined, and this is cand) */
    uint32_t            *pred0;  /* host emulation only: list 0 prediction dwords of the bi-pred lanes [16][256] */
    int                  pic_w, pic_h, sb_x, sb_y, sb_w, sb_h, sb_index;
    unsigned long long  *prof;   /* optional per-phase cycle accumulators (profiling builds), else NULL */
    uint32_t            *redo;   /* compact layout: set to 1 when this SB needs the full layout (its clipped search area has tail columns); else NULL */
} me_ctx_t;

/* raster index -> search (z-order) index of the 8x8 / 16x16 PUs (Codec/EbMotionEstimation.c:51-54) by bit
 * interleaving: raster = y*8 + x (3+3 bits) or y*4 + x (2+2 bits), z = ... y1 x1 y0 x0 */
SVT_DEV int me_z8(int b) { return (b & 1) | ((b & 2) << 1) | ((b & 4) << 2) | ((b & 8) >> 2) | (b & 16) >> 1 | (b & 32); }
SVT_DEV int me_z4(int b) { return (b & 1) | ((b & 2) << 1) | ((b & 4) >> 1) | (b & 8); }

SVT_DEV int16_t me_mvx(uint32_t mv) { return (int16_t)(mv & 0xFFFF); }
SVT_DEV int16_t me_mvy(uint32_t mv) { return (int16_t)(mv >> 16); }
SVT_DEV uint32_t me_pack_mv(int x, int y) { return ((uint32_t)(uint16_t)y << 16) | (uint16_t)x; }
SVT_DEV const uint8_t *me_pix(const svt_plane *p, int x, int y) {
    return p->buf + (ptrdiff_t)(p->origin_y + y) * p->stride + p->origin_x + x;
}
SVT_DEV int me_pu_nidx(int pu) { return pu > 20 ? me_z8(pu - 21) + 21 : pu > 4 ? me_z4(pu - 5) + 5 : pu; }
SVT_DEV void me_pu_geom(int pu, int *x, int *y, int *w) {
    if (pu == 0) { *x = 0; *y = 0; *w = 64; }
    else if (pu < 5) { *x = ((pu - 1) & 1) * 32; *y = ((pu - 1) >> 1) * 32; *w = 32; }
    else if (pu < 21) { *x = ((pu - 5) & 3) * 16; *y = ((pu - 5) >> 2) * 16; *w = 16; }
    else { *x = ((pu - 21) & 7) * 8; *y = ((pu - 21) >> 3) * 8; *w = 8; }
}

/* [quirk] origin is updated first and the width test re-evaluated afterwards, so left/top clipping never
 * shrinks the area (Codec/EbMotionEstimation.c:5022-5054 and the HME copies). */
SVT_DEV void me_clip_area(int origin, int16_t *area_origin, int16_t *area_size, int pad, int pic_dim) {
    int16_t o = *area_origin, s = *area_size;
    o = (int16_t)(((origin + o) < -pad) ? -pad - origin : o);
    s = (int16_t)(((origin + o) < -pad) ? s - (-pad - (origin + o)) : s);
    o = (int16_t)(((origin + o) > pic_dim - 1) ? o - ((origin + o) - (pic_dim - 1)) : o);
    if ((origin + o + s) > pic_dim) {
        int t = s - ((origin + o + s) - pic_dim);
        s     = (int16_t)(t > 1 ? t : 1);
    }
    *area_origin = o;
    *area_size   = s;
}
SVT_DEV int16_t me_clip_center(int origin, int16_t c, int pad, int pic_dim) {
    c = (int16_t)(((origin + c) < -pad) ? -pad - origin : c);
    c = (int16_t)(((origin + c) > pic_dim - 1) ? c - ((origin + c) - (pic_dim - 1)) : c);
    return c;
}
#endif

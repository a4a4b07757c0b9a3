/*
 * shim_plan.c -- the group planner of libSvtVp9Enc.so (shim_plan.h).  The pictures are cut into parts as the reference cuts them
 * (svt_hip_minigop_split, host/gop_shard.c); a part that is a whole period of its own levels keeps the random-access hierarchy, every
 * other part is a P chain.
 */
#include <string.h>

#include "../../include/svtvp9_hip.h"
#include "shim_plan.h"

static shim_plan_pic *add_pic(shim_plan *P, int64_t number, int64_t ref0, int64_t ref1, int layer, int levels, int wave) {
    shim_plan_pic *j = &P->pic[P->n++];
    j->number = number; j->ref0 = ref0; j->ref1 = ref1; j->layer = layer; j->levels = levels; j->wave = wave;
    j->n_lists = ref1 >= 0 ? 2 : 1;
    j->used_as_ref = layer < levels;
    return j;
}

/* the hierarchy between two already-listed pictures lo < hi by bisection, decode order; returns the deepest layer it made (0: none) */
static int add_hierarchy(shim_plan *P, int64_t lo, int64_t hi, int layer, int levels, int wave0) {
    if (hi - lo < 2 || P->n >= SHIM_MAX_MINIGOP) return 0;
    const int64_t mid = (lo + hi) / 2;
    add_pic(P, mid, lo, hi, layer, levels, wave0 + layer);
    const int a = add_hierarchy(P, lo, mid, layer + 1, levels, wave0), b = add_hierarchy(P, mid, hi, layer + 1, levels, wave0);
    return a > layer || b > layer ? (a > b ? a : b) : layer; /* (a, b are 0 or deeper than layer) */
}

int shim_plan_group(int64_t first, int pending, int levels, int cut_by_intra, int64_t prev_base, shim_plan *P) {
    svt_minigop_part parts[4];
    memset(P, 0, sizeof *P);
    if (pending < 1 || pending > SHIM_MAX_MINIGOP) return -1;
    const int np = svt_hip_minigop_split(pending + (cut_by_intra ? 1 : 0), levels, cut_by_intra, parts);
    if (np < 1) return -1;
    if (cut_by_intra) parts[np - 1].length -= 1; /* the intra picture itself is the caller's */
    int64_t prev = prev_base;
    for (int k = 0; k < np; k++) {
        if (parts[k].length < 1) continue;
        const int64_t p0 = first + parts[k].start, base = p0 + parts[k].length - 1;
        const int     lv = parts[k].hierarchical_levels;
        if (parts[k].random_access && prev >= 0) { /* base picture first (decode order), then the B hierarchy: a wave per layer */
            if (P->n_waves + lv + 1 > SHIM_MAX_WAVES) return -1;
            add_pic(P, base, prev, prev, 0, lv, P->n_waves)->used_as_ref = 1;
            const int deepest = add_hierarchy(P, prev, base, 1, lv, P->n_waves);
            for (int l = 0; l <= lv; l++) {
                P->wave[P->n_waves + l].layer = l;
                P->wave[P->n_waves + l].deep_eligible = l >= 2 && l >= deepest - 1 && l <= deepest;
            }
            P->n_waves += lv + 1;
        } else { /* low-delay P: the reference's structure tables (Codec/EbPredictionStructure.c) are picture decision, not reproduced --
                    every picture is predicted from its predecessor and serves as the next one's reference: a wave (of layer 0) each */
            for (int64_t q = p0; q <= base; q++) add_pic(P, q, q - 1, -1, 0, lv, P->n_waves++)->used_as_ref = 1;
        }
        prev = base;
    }
    P->first = first; P->last = first + pending - 1;
    P->oldest = first;
    for (int i = 0; i < P->n; i++) {
        if (P->pic[i].ref0 >= 0 && P->pic[i].ref0 < P->oldest) P->oldest = P->pic[i].ref0;
        if (P->pic[i].ref1 >= 0 && P->pic[i].ref1 < P->oldest) P->oldest = P->pic[i].ref1;
    }
    return 0;
}

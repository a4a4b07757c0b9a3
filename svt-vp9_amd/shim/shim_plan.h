/*
 * shim_plan.h -- the structure of one group of pictures (a mini-GOP, or what an intra refresh / the end of the stream left of one): decode
 * order, references, temporal layers, waves, and which waves may go to the deep-layer stream.  Integer logic only: no HIP, no shim state.
 */
#ifndef SHIM_PLAN_H
#define SHIM_PLAN_H
#include <stdint.h>

#define SHIM_MAX_MINIGOP 16
#define SHIM_MAX_WAVES (SHIM_MAX_MINIGOP + 8)

typedef struct shim_plan_pic { /* one picture of the group, in decode order */
    int64_t number, ref0, ref1; /* display numbers; ref1 = -1 with one list */
    int     layer, levels, n_lists, used_as_ref;
    int     wave;               /* the batch of mutually independent pictures it is coded with: its references belong to earlier waves */
} shim_plan_pic;

typedef struct shim_plan_wave {
    int layer;          /* the temporal layer all its pictures share */
    int deep_eligible;  /* one of the two deepest layers of its part, and layer >= 2: nothing of the NEXT group depends on it */
} shim_plan_wave;

typedef struct shim_plan {
    shim_plan_pic  pic[SHIM_MAX_MINIGOP];
    shim_plan_wave wave[SHIM_MAX_WAVES];
    int            n, n_waves;
    int64_t        first, last, oldest; /* first / last picture of the group; the oldest picture its work reads (a reference) */
} shim_plan;

/* The group of `pending` pictures from display number `first`, behind the base (or intra) picture `prev_base` (-1: none).  levels: the
 * configured hierarchical levels.  cut_by_intra: the group was released by an intra refresh -- the reference's pre-assignment buffer
 * then holds the intra picture as its last element (Codec/EbPictureDecisionProcess.c:1641-1646) and the split is made over pending + 1.
 * Returns 0, or -1 when svt_hip_minigop_split refuses the group. */
int shim_plan_group(int64_t first, int pending, int levels, int cut_by_intra, int64_t prev_base, shim_plan *P);

#endif

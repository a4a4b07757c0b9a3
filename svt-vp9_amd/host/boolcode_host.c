/*
 * boolcode_host.c -- host-side (plain C) companions of the bool coder (csrc/boolcode.hip):
 *   - svt_hip_boolcode_host: the rules of csrc/boolcode_core.h (the same inline text the kernels call) in front of the plain serial
 *     writer -- low end, range, bit count, backward carry walk -- which is the model on machines without the reference
 *     (pack_mb_tokens over vpx_write, VPX/vp9_bitstream.c:98-162, VPX/bitwriter.h:34-84, VPX/bitwriter.c);
 *   - the capacities and the validation of a segment list the host-pointer entry points share.
 */
#include <stdlib.h>
#include <string.h>
#include "../../include/svtvp9_hip.h"
#include "../csrc/boolcode_core.h"

uint32_t svt_hip_boolcode_capacity(uint32_t n_bools) {
    const uint64_t bytes = SVT_BOOL_CAPACITY_OF((uint64_t)n_bools);
    return bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bytes;
}
uint32_t svt_hip_boolcode_bools_capacity(uint32_t n_tokens) {
    const uint64_t n = (uint64_t)n_tokens * SVT_BOOL_MAX_PER_TOKEN;
    return n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
}

/* 0: every segment lies inside its buffer; *items = records of all segments */
int32_t svt_boolcode_check_segments(uint32_t n_tokens, uint32_t n_bools, const svt_bool_segment *segments, uint32_t n_segments, uint64_t *items) {
    uint64_t n = 0;
    for (uint32_t s = 0; s < n_segments; s++) {
        const uint64_t end = (uint64_t)segments[s].first + segments[s].count;
        if (segments[s].kind > 1 || end > (segments[s].kind ? n_bools : n_tokens)) return SVT_HIP_ERR_BAD_PARAMETER;
        n += segments[s].count;
    }
    *items = n;
    return SVT_HIP_OK;
}

typedef struct {
    uint32_t low, range;
    int      count;
    size_t   pos;
    uint8_t *buf;
} bool_writer;

static void put(bool_writer *w, uint32_t rec) {
    uint32_t       split;
    const uint32_t next = svt_bool_step(w->range, rec, &split);
    int            shift = (int)(next >> 8);
    if ((rec >> 8) & 1) w->low += split;
    w->range = next & 255u;
    w->count += shift;
    if (w->count >= 0) {
        const int offset = shift - w->count;
        if ((w->low << (offset - 1)) & 0x80000000u) { /* the carry walks back over the bytes that are all ones */
            size_t x = w->pos;
            while (x > 0 && w->buf[x - 1] == 0xff) w->buf[--x] = 0;
            if (x > 0) w->buf[x - 1]++;
        }
        w->buf[w->pos++] = (uint8_t)(w->low >> (24 - offset));
        w->low = (w->low << offset) & 0xffffffu;
        shift = w->count;
        w->count -= 8;
    }
    w->low <<= shift;
}

int32_t svt_hip_boolcode_host(const svt_bool_tables *tables, const uint32_t *tokens, uint32_t n_tokens, const uint16_t *bools, uint32_t n_bools,
                              const svt_bool_segment *segments, uint32_t n_segments, uint8_t *bytes, uint32_t capacity, uint32_t *size) {
    if (!size || (!bytes && capacity) || (!tokens && n_tokens) || (!bools && n_bools) || (!segments && n_segments)) return SVT_HIP_ERR_BAD_PARAMETER;
    const svt_bool_segment whole = {0, n_tokens, 0};
    if (!segments) { segments = &whole; n_segments = 1; }
    uint64_t items = 0;
    if (svt_boolcode_check_segments(n_tokens, n_bools, segments, n_segments, &items)) return SVT_HIP_ERR_BAD_PARAMETER;
    if (items && !tables) return SVT_HIP_ERR_BAD_PARAMETER;
    if (items * SVT_BOOL_MAX_PER_TOKEN > 0x1fffffffull) return SVT_HIP_ERR_BAD_PARAMETER;
    bool_writer w = {0, 255, -24, 0, NULL};
    w.buf = (uint8_t *)malloc((size_t)svt_hip_boolcode_capacity((uint32_t)(items * SVT_BOOL_MAX_PER_TOKEN)) + 8);
    if (!w.buf) return SVT_HIP_ERR_NO_RESOURCES;
    put(&w, SVT_BOOL_RECORD(0, 128));
    for (uint32_t s = 0; s < n_segments; s++) {
        const svt_bool_segment *g = &segments[s];
        for (uint32_t k = 0; k < g->count; k++) {
            if (g->kind) { put(&w, bools[g->first + k]); continue; }
            uint16_t       out[SVT_BOOL_MAX_PER_TOKEN];
            const uint32_t rec = tokens[g->first + k];
            const int      n = svt_bool_expand(rec, svt_bool_skip0(rec, k > 0, k > 0 ? tokens[g->first + k - 1] : 0), tables, out);
            for (int i = 0; i < n; i++) put(&w, out[i]);
        }
    }
    for (int i = 0; i < SVT_BOOL_FRAME_TAIL; i++) put(&w, SVT_BOOL_RECORD(0, 128));
    if ((w.buf[w.pos - 1] & 0xe0) == 0xc0) w.buf[w.pos++] = 0;
    *size = (uint32_t)w.pos;
    if (capacity) memcpy(bytes, w.buf, w.pos < capacity ? w.pos : capacity);
    free(w.buf);
    return SVT_HIP_OK;
}

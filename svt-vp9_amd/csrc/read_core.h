/*
 * read_core.h -- the reading primitives of the frame reader (host/frame_read.c), plain inline C: what the writers' stages have no
 * counterpart for.  Everything that is symmetrical between writing and reading (contexts, tables, field order) stays where the
 * writers keep it.
 *
 *   svt_bit_reader    vpx_read_bit_buffer: the uncompressed header's bits, MSB first, bounded by the buffer's end
 *   svt_bool_reader   vpx_reader (the VP9 specification's boolean decoder, 9.2): init with the marker bit, fill, read, normalise
 *   svt_br_tree       vpx_read_tree over a vpx_tree_index array
 *
 * Memory safety: neither reader dereferences a byte at or beyond its `end`; what lies beyond reads as zero bits and is counted
 * (svt_bit_reader.overrun, svt_bool_past_end), so a caller decides whether a truncated stream is an error.
 */
#ifndef SVT_READ_CORE_H
#define SVT_READ_CORE_H

#include <stdint.h>

typedef struct svt_bit_reader {
    const uint8_t *buf;
    uint64_t       bits, limit; /* position and end, in bits */
    uint32_t       overrun;     /* bits asked for beyond the end (they read 0) */
} svt_bit_reader;

static inline void svt_bit_reader_init(svt_bit_reader *r, const uint8_t *buf, uint64_t size) {
    r->buf = buf; r->bits = 0; r->limit = size * 8; r->overrun = 0;
}
static inline int svt_bit_read(svt_bit_reader *r) {
    if (r->bits >= r->limit) { r->overrun++; return 0; }
    const int b = (r->buf[r->bits >> 3] >> (7 - (r->bits & 7))) & 1;
    r->bits++;
    return b;
}
static inline uint32_t svt_bit_literal(svt_bit_reader *r, int n) {
    uint32_t v = 0;
    while (n--) v = v << 1 | (uint32_t)svt_bit_read(r);
    return v;
}

/* vpx_reader (VPX bitreader.h / the specification's 9.2.1-9.2.2) with a 64-bit window: `value` holds the next count + 8 bits of the
 * stream left-aligned; a read compares against split << 56, keeps or subtracts, and shifts range back into 128 .. 255. */
typedef struct svt_bool_reader {
    const uint8_t *buf, *end;
    uint64_t       value;
    int            count;       /* bits in the window beyond the 8 under comparison */
    uint32_t       range;
    uint64_t       fetched;     /* bytes taken into the window, the zero bytes beyond the end included */
    uint64_t       size;
} svt_bool_reader;

static inline void svt_bool_fill(svt_bool_reader *r) {
    int shift = 64 - 8 - (r->count + 8);
    while (shift >= 0) {
        const uint64_t byte = r->buf < r->end ? *r->buf++ : 0;
        r->fetched++;
        r->count += 8;
        r->value |= byte << shift;
        shift -= 8;
    }
}
static inline int svt_bool_read(svt_bool_reader *r, int prob) {
    const uint32_t split = (r->range * (uint32_t)prob + (256u - (uint32_t)prob)) >> 8;
    if (r->count < 0) svt_bool_fill(r);
    const uint64_t big = (uint64_t)split << 56;
    int bit = 0;
    if (r->value >= big) { r->range -= split; r->value -= big; bit = 1; }
    else r->range = split;
    int shift = 0;                                     /* vpx_norm[range]: range back into 128 .. 255 */
    while (!((r->range << shift) & 0x80u)) shift++;    /* (range >= 1: split is 1 .. range - 1 for prob 1 .. 255) */
    r->range <<= shift;
    r->value <<= shift;
    r->count -= shift;
    return bit;
}
static inline int svt_bool_literal(svt_bool_reader *r, int n) {
    int v = 0;
    while (n--) v = v << 1 | svt_bool_read(r, 128);
    return v;
}
/* bits consumed so far / did the decoder consume bits that the buffer does not hold (vpx_reader_has_error) */
static inline uint64_t svt_bool_consumed_bits(const svt_bool_reader *r) { return r->fetched * 8 - (uint64_t)(r->count + 8); }
static inline int svt_bool_past_end(const svt_bool_reader *r) { return svt_bool_consumed_bits(r) > r->size * 8; }
/* vpx_reader_init: returns the marker bit, which a conformant stream has as 0; size 0 is an error of the caller's */
static inline int svt_bool_reader_init(svt_bool_reader *r, const uint8_t *buf, uint64_t size) {
    r->buf = buf; r->end = buf + size; r->value = 0; r->count = -8; r->range = 255; r->fetched = 0; r->size = size;
    svt_bool_fill(r);
    return svt_bool_read(r, 128);
}
/* vpx_read_tree: tree[i] > 0 the next node pair, <= 0 the negated leaf; probs[i >> 1] the node's probability */
static inline int svt_br_tree(svt_bool_reader *r, const int8_t *tree, const uint8_t *probs) {
    int i = 0;
    while ((i = tree[i + svt_bool_read(r, probs[i >> 1])]) > 0) {}
    return -i;
}

#endif /* SVT_READ_CORE_H */

/*
 * frame_core.h -- the rules of frame-packet assembly, written once as plain inline functions that compile both for the device
 * (csrc/frame.hip) and for the host (host/frame_host.c), like boolcode_core.h; and the derivation of SVT_FRAME_HEADER_MAX.
 *
 *   svt_frame_packet_size   bytes of a picture's packet, or SVT_FRAME_SIZE_NONE when its tile was not coded
 *   svt_frame_layout        offset of a picture from the sizes in front of it; the total and the pictures without a packet
 *   svt_frame_span          the part [0, n) of a run of bytes at arena position `pos` that lies below the arena's capacity
 *   svt_frame_parts_size    svt_frame_packet_size for a packet whose compressed header is a device stream of its own
 *   svt_frame_size_field_byte   a byte of the uncompressed header with first_part_size filled in
 *
 * SVT_FRAME_HEADER_MAX (include/svtvp9_hip.h) = 27 + 29 = 56, from the syntax (VPX/vp9_bitstream.c):
 *
 * Uncompressed header, the longest path through write_uncompressed_header (:1186-1290), in bits:
 *     8   frame marker 2, profile 2, show_existing_frame 1, frame_type 1, show_frame 1, error_resilient_mode 1
 *   100   the longest of the three bodies -- a non-key intra-only picture: intra_only 1, reset_frame_context 2, sync code 24,
 *         refresh_frame_mask 8, write_frame_size 32 + write_render_size 1 + 32
 *         (a key frame has 93: sync code 24, colour space 3 + range 1, frame size 32, render size 33;
 *          an inter picture 95: intra_only 1, reset 2, refresh mask 8, 3 x (index 3 + sign bias 1), 3 x found 1, frame size 32,
 *          render size 33, allow_hp 1, interpolation filter 1 + 2)
 *     2   refresh_frame_context, frame_parallel_decoding_mode
 *     2   frame_context_idx
 *    59   encode_loopfilter: level 6, sharpness 3, enabled 1, update 1, 6 deltas x (changed 1 + magnitude 6 + sign 1)
 *    26   encode_quantization: base_qindex 8, 3 x write_delta_q (1 + 4 + 1)
 *     1   encode_segmentation: enabled = 0
 *     2   write_tile_info: one column bit (present from 8 SB columns on), one row bit
 *    16   first_part_size (eb_vp9_pack_bitstream, :1385)
 *   216 bits = 27 bytes.
 *
 * Compressed header, write_compressed_header (:1292-1367): at most SVT_FRAME_COMPRESSED_MAX_BOOLS = 210 bools --
 *     3 tx_mode (literal 2, select 1), 4 update_coef_probs (one "no update" bit per transform size), 3 skip,
 *     21 inter mode (7 x 3), 4 intra/inter, 2 + 5 reference mode (REFERENCE_MODE_SELECT), 10 single ref, 5 comp ref,
 *     36 y mode (4 x 9), 48 partition (16 x 3), 69 + 4 eb_vp9_write_nmv_probs (joints 3, 2 x (sign 1, classes 10, class0 1, bits 10),
 *     2 x (class0_fp 2 x 3, fp 3), with allow_hp 2 x (class0_hp, hp)).
 *   Every one of them is a 0 at probability 128 or 252, or a 1 at probability 128: from a range r in 128 .. 255 the next range is
 *   split = 1 + ((r - 1) * p >> 8) >= 64 or r - split >= 64 (p = 128), so each bool shifts the low end by at most ONE bit; so do the 33
 *   framing bools.  With S <= 210 + 33 shifts the coder writes (S - 16) / 8 <= 28 bytes (boolcode_core.h) and at most one marker
 *   byte behind them: 29.
 */
#ifndef SVT_FRAME_CORE_H
#define SVT_FRAME_CORE_H

#include <stdint.h>
#include "boolcode_core.h"

#define SVT_FRAME_COMPRESSED_MAX_BOOLS 210 /* (SVT_FRAME_UNCOMPRESSED_MAX = 27 stands in include/svtvp9_hip.h: a descriptor holds that header) */
#define SVT_FRAME_COMPRESSED_MAX ((SVT_FRAME_COMPRESSED_MAX_BOOLS + 1 + SVT_BOOL_FRAME_TAIL - 16) / 8 + 1)
#if SVT_FRAME_UNCOMPRESSED_MAX + SVT_FRAME_COMPRESSED_MAX != SVT_FRAME_HEADER_MAX
#error "SVT_FRAME_HEADER_MAX does not follow from the syntax"
#endif

/* tile_size: what the bool coder left in *d_size */
SVT_HD uint32_t svt_frame_packet_size(uint32_t header_len, uint32_t trailer_len, uint32_t tile_size, uint32_t tile_capacity) {
    if (tile_size == SVT_BOOL_SIZE_OVERFLOW || tile_size > tile_capacity) return SVT_FRAME_SIZE_NONE;
    const uint64_t n = (uint64_t)header_len + tile_size + trailer_len;
    return n >= SVT_FRAME_SIZE_NONE ? SVT_FRAME_SIZE_NONE : (uint32_t)n;
}

/* sizes[0 .. n_pics): svt_frame_packet_size of every picture.  Returns the offset of picture `pic` (pic = n_pics: the total), the sum
 * of the sizes in front of it; *none = pictures without a packet among those.  Sums that leave 32 bits stay at 0xFFFFFFFF. */
SVT_HD uint32_t svt_frame_layout(const uint32_t *sizes, int pic, uint32_t *none) {
    uint64_t off = 0;
    uint32_t bad = 0;
    for (int i = 0; i < pic; i++) {
        if (sizes[i] == SVT_FRAME_SIZE_NONE) bad++;
        else off += sizes[i];
    }
    *none = bad;
    return off > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)off;
}

/* of the n bytes at arena position pos, how many lie below arena_capacity */
SVT_HD uint32_t svt_frame_span(uint64_t pos, uint32_t n, uint32_t arena_capacity) {
    if (pos >= arena_capacity) return 0;
    return arena_capacity - pos < n ? (uint32_t)(arena_capacity - pos) : n;
}

/* A packet of three parts (svt_frame_parts_packet): compressed_size is what the bool coder left in the header stream's *d_size.  It
 * must be a first_part_size a decoder accepts and the 16 bits can say: 1 .. 0xFFFF */
SVT_HD uint32_t svt_frame_parts_size(uint32_t header_len, uint32_t trailer_len, uint32_t compressed_size, uint32_t compressed_capacity, uint32_t tile_size,
                                     uint32_t tile_capacity) {
    if (tile_size == SVT_BOOL_SIZE_OVERFLOW || tile_size > tile_capacity) return SVT_FRAME_SIZE_NONE;
    if (compressed_size == SVT_BOOL_SIZE_OVERFLOW || compressed_size == 0 || compressed_size > compressed_capacity || compressed_size > 0xFFFFu) return SVT_FRAME_SIZE_NONE;
    const uint64_t n = (uint64_t)header_len + compressed_size + tile_size + trailer_len;
    return n >= SVT_FRAME_SIZE_NONE ? SVT_FRAME_SIZE_NONE : (uint32_t)n;
}

/* byte t of an uncompressed header whose bits [size_bit, size_bit + 16) (bit 0 = the most significant bit of byte 0) are to say `value`,
 * most significant bit first: the field's bits of `byte` are replaced, the others kept.  The field lies in the three bytes from
 * size_bit >> 3 on (in two when size_bit is a multiple of 8): seen as 24 bits it is value << (8 - phase) */
SVT_HD uint8_t svt_frame_size_field_byte(uint8_t byte, uint32_t t, uint32_t size_bit, uint32_t value) {
    const uint32_t j = t - (size_bit >> 3);
    if (j > 2u) return byte;
    const uint32_t up = 8u - (size_bit & 7u), at = 16u - 8u * j;
    const uint32_t mask = ((0xFFFFu << up) >> at) & 0xFFu, bits = (((value & 0xFFFFu) << up) >> at) & 0xFFu;
    return (uint8_t)((byte & ~mask) | bits);
}

#endif /* SVT_FRAME_CORE_H */

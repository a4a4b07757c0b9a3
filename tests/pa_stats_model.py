"""numpy restatement of the picture-analysis statistics of the reference (Source/Lib/Codec/EbPictureAnalysisProcess.c), written
from its loops: noise detection (detect_input_picture_noise :3512-3619, quarter_sample_detect_noise :3809-3928,
sub_sample_detect_noise :3930-4055 over eb_vp9_noise_extract_luma_weak :1653-1706), the histograms and averages
(:4237-4432, :4839-4886, calculate_histogram :128-150) and compute_chroma_block_mean (:1828-2109).

The quirks it keeps, each named where it is coded, are listed in DESIGN.md section 5 ("Picture statistics")."""
import numpy as np

FULL, HALF, QUARTER = 0, 1, 2
FLAT_MAX_VAR = 50                        # FLAT_MAX_VAR = FLAT_MAX_VAR_DECIM (:32-33)
NOISE_MIN_LEVEL = {0: 70000, 1: 120000}  # NOISE_MIN_LEVEL(_DECIM)_0 / _1 (:34-37)
CLASS_1, CLASS_2, CLASS_3, CLASS_3_1, CLASS_4 = 1, 2, 3, 4, 5  # PIC_NOISE_CLASS_*, Codec/EbDefinitions.h:860-871


def weak_filter(pic):
    """eb_vp9_noise_extract_luma_weak over a whole picture: (denoised, noise).  The strips of 64 rows the reference works in do not
    show: the filter reads the input picture, so a strip's first and last rows see their neighbours in the next strip."""
    p = pic.astype(np.int32)
    den = p.copy()
    den[1:-1, 1:-1] = (p[:-2, 1:-1] + p[1:-1, :-2] + 4 * p[1:-1, 1:-1] + p[1:-1, 2:] + p[2:, 1:-1]) // 8
    noise = np.clip(p - den, 0, 255)  # CLIP3EQ(0, 255, in - denoised); the border has den == in
    return den.astype(np.uint8), noise.astype(np.uint8)


def _sums8x8(blk, sub):
    """per 8x8 block of `blk` (a multiple of 8 each way): (mean << 8, mean of squares << 16).
    sub: rows 0, 2, 4, 6 only, sum << 3 and << 11 (eb_vp9_compute_sub_mean8x8_sse2_intrin, ..subd_mean_of_squared_values8x8.., the
    AVX2 four-8x8 kernel); else all rows, (sum << 8) / 64 and (sum << 16) / 64 (compute_mean, compute_mean_of_squared_values)."""
    h, w = blk.shape
    b = blk.astype(np.uint64).reshape(h // 8, 8, w // 8, 8)
    if sub:
        b = b[:, 0::2]
        return b.sum(axis=(1, 3)) << np.uint64(3), (b * b).sum(axis=(1, 3)) << np.uint64(11)
    return (b.sum(axis=(1, 3)) << np.uint64(8)) // np.uint64(64), ((b * b).sum(axis=(1, 3)) << np.uint64(16)) // np.uint64(64)


def _up(a):
    n, m = a.shape
    return a.reshape(n // 2, 2, m // 2, 2).sum(axis=(1, 3)) >> np.uint64(2)


def variance64x64(blk):
    """compute_variance64x64 (:408-1210): sub-sampled 8x8 sums, then >> 2 averages of four children per level."""
    m, q = _sums8x8(blk, True)
    for _ in range(3):
        m, q = _up(m), _up(q)
    return int(q[0, 0]) - int(m[0, 0]) ** 2


def variance16x16(blk):
    """compute_variance16x16 (:345-399): full 8x8 means."""
    m, q = _sums8x8(blk, False)
    m, q = _up(m), _up(q)
    return int(q[0, 0]) - int(m[0, 0]) ** 2


def variance32x32(blk):
    """compute_variance32x32 (:152-343).  Its 8x8 blocks are numbered row * 4 + col, its 16x16 level then sums {0,1,8,9}, {2,3,10,11},
    {4,5,12,13}, {6,7,14,15}: block rows 0 + 2 and 1 + 3 are paired (:301-329).  Kept as written, although no input can show it: the 8x8
    values are multiples of 4, so the 16x16 level is exact and only the total reaches the one truncating shift."""
    m, q = _sums8x8(blk, False)
    m, q = m.ravel(), q.ravel()
    groups = ((0, 1, 8, 9), (2, 3, 10, 11), (4, 5, 12, 13), (6, 7, 14, 15))
    m16 = [sum(int(m[i]) for i in g) >> 2 for g in groups]
    q16 = [sum(int(q[i]) for i in g) >> 2 for g in groups]
    return (sum(q16) >> 2) - (sum(m16) >> 2) ** 2


def noise_class(method, v, luma_height):
    if method == FULL:
        th = 25 if luma_height <= 720 else 0
        for lim, c in ((80, 11), (70, 10), (60, 9), (50, 8), (40, 7), (30, 6), (20, CLASS_4), (17, CLASS_3_1), (10, CLASS_3), (5, CLASS_2)):
            if v >= lim + th:
                break
        else:
            c = CLASS_1
        return CLASS_3_1 if c >= CLASS_4 else c  # the final clamp (:3615-3616)
    if method == HALF:
        th = 25 if luma_height <= 720 else 10 if luma_height <= 1080 else 0
        return CLASS_3_1 if v >= 55 + th else CLASS_3 if v >= 10 + th else CLASS_2 if v >= 5 + th else CLASS_1
    return CLASS_3_1 if v > 60 else CLASS_3 if v >= 10 else CLASS_2 if v >= 5 else CLASS_1


def detect_noise(method, plane, full_w, full_h, noise_detection_th, luma_height):
    """-> dict(flags [ceil(H/64) * ceil(W/64)] uint8, pic_noise_class, sb_count, variance_sum, den, noise, region (rows, cols) of den /
    noise the reference's loop filters).  `plane` is the full luma (FULL), the 1/16 (HALF) or the 1/4 (QUARTER) picture."""
    h, w = plane.shape
    pw, ph = (full_w + 63) // 64, (full_h + 63) // 64
    flags = np.zeros(pw * ph, np.uint8)
    den, noise = weak_filter(plane)
    tot, cnt = 0, 0
    if method == FULL:
        th = NOISE_MIN_LEVEL[0] if noise_detection_th == 1 else NOISE_MIN_LEVEL[1]
        for sb in range(pw * ph):
            y, x = (sb // pw) * 64, (sb % pw) * 64
            if x + 64 > w or y + 64 > h:  # is_complete_sb
                continue
            nv = variance64x64(noise[y:y + 64, x:x + 64])
            tot += nv >> 16                                   # accumulated >> 16 ...
            dv = variance64x64(den[y:y + 64, x:x + 64]) >> 16
            if dv < FLAT_MAX_VAR and nv > th:                 # ... compared in 16.16
                flags[sb] = 1
            cnt += 1
        region = (h, w)
    else:
        n, size, var = (4, 16, variance16x16) if method == HALF else (2, 32, variance32x32)
        if method == HALF:
            th = NOISE_MIN_LEVEL[0] if noise_detection_th == 1 else NOISE_MIN_LEVEL[1]
        else:
            th = NOISE_MIN_LEVEL[1] if noise_detection_th == 0 else NOISE_MIN_LEVEL[0]
        for v64 in range(h // 64):          # whole 64x64 blocks of the decimated picture only
            for h64 in range(w // 64):
                for vi in range(n):
                    for hi in range(n):
                        x, y = h64 * 64 + hi * size, v64 * 64 + vi * size
                        sb = (v64 * n + vi) * pw + h64 * n + hi
                        # the noise picture is a 64-row strip and noise_origin_index has no row term: always the strip's first rows
                        nv = var(noise[v64 * 64:v64 * 64 + size, x:x + size])
                        tot += nv >> 16
                        dv = var(den[y:y + size, x:x + size]) >> 16
                        if dv < FLAT_MAX_VAR and nv > th:
                            flags[sb] = 1
                        cnt += 1
        region = ((h // 64) * 64, (w // 64) * 64)
    v = tot // cnt if cnt else 0  # integer division by the count of visited SBs
    return dict(flags=flags, pic_noise_class=noise_class(method, v, luma_height), sb_count=cnt, variance_sum=tot, den=den, noise=noise,
                region=region)


def histograms(y16, cb, cr, full_w, full_h, regions_w, regions_h, scd_mode, full_padded=None):
    """-> hist uint32 [rw][rh][3][256], avg_region uint8 [rw][rh][3], avg [3] (None where the reference leaves the entry alone).
    cb / cr: the source chroma planes; full_padded: the padded full luma buffer (scd_mode 0 reads its first full_h x full_w bytes)."""
    hist = np.ones((regions_w, regions_h, 3, 256), np.uint64)  # bins start at 1
    avg_region = np.zeros((regions_w, regions_h, 3), np.uint8)
    tot = [0, 0, 0]
    for c, (pl, pw, ph) in enumerate(((y16, y16.shape[1], y16.shape[0]), (cb, full_w, full_h), (cr, full_w, full_h))):
        rw, rh = pw // regions_w, ph // regions_h
        for i in range(regions_w):
            for j in range(regions_h):
                wo = rw + (pw - regions_w * rw if i == regions_w - 1 else 0)  # the last region takes the remainder
                ho = rh + (ph - regions_h * rh if j == regions_h - 1 else 0)
                if c == 0:
                    a = pl[j * rh:j * rh + ho, i * rw:i * rw + wo]
                    s = int(a.sum(dtype=np.uint64))
                    avg_region[i, j, 0] = ((s + ((wo * ho) >> 1)) // (wo * ho)) & 255
                else:  # every 4th row and column of the region's chroma samples
                    a = pl[(j * rh) >> 1:((j * rh) >> 1) + (ho >> 1):4, (i * rw) >> 1:((i * rw) >> 1) + (wo >> 1):4]
                    s = int(a.sum(dtype=np.uint64)) << 4
                    avg_region[i, j, c] = ((s + ((wo * ho) >> 3)) // ((wo * ho) >> 2)) & 255
                hist[i, j, c] += np.bincount(a.ravel(), minlength=256).astype(np.uint64)
                tot[c] += s << 4 if c == 0 else s
    hist <<= np.uint64(4)
    wh = full_w * full_h
    if scd_mode == 0:
        # buffer_y is indexed without the origin (:4857-4860): the top-left full_h x full_w bytes of the padded buffer
        a = full_padded[0:(full_h >> 3) * 8:2, :(full_w >> 3) * 8]  # rows 0, 2, 4, 6 of every 8x8 block
        mean = int(a.sum(dtype=np.uint64)) << 3
        mean = (mean + (wh >> 7)) // (wh >> 6)
        avg = [((mean + 128) >> 8) & 255, None, None]
    else:
        avg = [((tot[0] + (wh >> 1)) // wh) & 255, ((tot[1] + (wh >> 3)) // (wh >> 2)) & 255, ((tot[2] + (wh >> 3)) // (wh >> 2)) & 255]
    return hist.astype(np.uint32), avg_region, avg


def chroma_means(cb, cr, width, height):
    """-> cb_mean, cr_mean uint8 [n_sb][21]: 0 = 64x64, 1-4 = 32x32, 5-20 = 16x16 (luma sizes), zero for incomplete SBs."""
    pw, ph = (width + 63) // 64, (height + 63) // 64
    out = [np.zeros((pw * ph, 21), np.uint8), np.zeros((pw * ph, 21), np.uint8)]
    for sb in range(pw * ph):
        y, x = (sb // pw) * 64, (sb % pw) * 64
        if x + 64 > width or y + 64 > height:
            continue
        for c, pl in enumerate((cb, cr)):
            m16, _ = _sums8x8(pl[y // 2:y // 2 + 32, x // 2:x // 2 + 32], True)
            m32 = _up(m16)
            m64 = (int(m32[0, 0]) + int(m32[0, 1]) + int(m32[1, 1]) + int(m32[1, 1])) >> 2  # block 3 twice, block 2 never (:2010-2015)
            out[c][sb] = np.concatenate([[m64], m32.ravel(), m16.ravel()]).astype(np.uint64) >> np.uint64(8)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# test pictures: flat areas with additive Gaussian noise next to textured areas, so that the flags and the classes vary
# ------------------------------------------------------------------------------------------------------------------------------
def gen_picture(w, h, seed, sigma, textured=0.25):
    """w x h uint8: level 128 + N(0, sigma), the right `textured` share of the columns replaced by a smooth wave of amplitude 100 and
    period 32 (a large denoised variance, next to no noise after the filter) so that flagged and unflagged SBs sit side by side and
    the picture's mean noise variance is set by sigma."""
    rng = np.random.default_rng(seed)
    p = 128.0 + rng.normal(0.0, sigma, (h, w)) if sigma > 0 else np.full((h, w), 128.0)
    x0 = int(w * (1 - textured))
    if x0 < w:
        p[:, x0:] = 128.0 + 100.0 * np.sin((np.arange(w - x0)[None, :] + np.arange(h)[:, None]) * (2 * np.pi / 32))
    return np.clip(np.rint(p), 0, 255).astype(np.uint8)


def gen_chroma(w, h, seed):
    rng = np.random.default_rng(seed)
    ramp = (np.arange(w)[None, :] * 200 // max(w - 1, 1) + np.arange(h)[:, None] * 40 // max(h - 1, 1)).astype(np.int32)
    return np.clip(ramp + rng.integers(-12, 13, (h, w)), 0, 255).astype(np.uint8)


# (method, analysed width, height, full width, height, noise_detection_th, luma_height): small pictures with incomplete SBs, a width
# that is not a multiple of 64, and decimated pictures whose last rows / columns the reference's loops never visit
SMALL_NOISE_CASES = ((FULL, 200, 136, 200, 136, 1, 1080), (HALF, 160, 136, 640, 544, 1, 2160), (QUARTER, 160, 136, 320, 272, 1, 1080),
                     (FULL, 200, 136, 200, 136, 0, 480), (HALF, 160, 136, 640, 544, 0, 1080), (QUARTER, 160, 136, 320, 272, 0, 1080))
SIGMAS = (0, 5, 8, 12, 25)  # flat level, flagged class 1, class 2, class 3, class 3_1 (checked by test_inputs_exercise_the_decision)


def noise_picture(w, h, sigma):
    return gen_picture(w, h, 100 + sigma, sigma)


# ------------------------------------------------------------------------------------------------------------------------------
# edge pictures: content at the ceilings of the arithmetic, and planes whose padding is not a copy of their edge
# ------------------------------------------------------------------------------------------------------------------------------
LUMA_KINDS = ("white", "black", "checker", "speck", "stripes_even", "stripes_odd", "halves", "random")
CHROMA_KINDS = ("saturated", "zero", "random")


def edge_luma(kind, w, h, seed=0):
    """white: 255; black: 0; checker: ((x + y) & 1) * 255 (every interior noise sample is 128 or 0); speck: 255 where x and y are both
    even; stripes_even / stripes_odd: 255 on even / odd rows (the 64x64 variance samples rows 0, 2, 4, 6 of a block only, so the two
    differ); halves: 0 | 255 split inside every 8x8 block (the largest 8x8 variance); random: uniform 0..255."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "white":
        p = np.full((h, w), 255)
    elif kind == "black":
        p = np.zeros((h, w))
    elif kind == "checker":
        p = ((x + y) & 1) * 255
    elif kind == "speck":
        p = ((x & 1) == 0) * ((y & 1) == 0) * 255
    elif kind == "stripes_even":
        p = ((y & 1) == 0) * 255
    elif kind == "stripes_odd":
        p = (y & 1) * 255
    elif kind == "halves":
        p = ((x >> 2) & 1) * 255
    elif kind == "random":
        p = np.random.default_rng(7000 + seed).integers(0, 256, (h, w))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, dtype=np.uint8)


def edge_chroma(kind, w, h, seed=0):
    if kind == "saturated":
        return np.full((h, w), 255, np.uint8)
    if kind == "zero":
        return np.zeros((h, w), np.uint8)
    if kind == "random":
        return np.random.default_rng(8000 + seed).integers(0, 256, (h, w), dtype=np.uint8)
    raise ValueError(kind)


def hostile_plane(pic, ox, oy, stride, seed):
    """`pic` at (oy, ox) of a (h + 2 * oy) x stride buffer whose every other byte is seeded noise: a read that ought to be clamped to
    the picture, or one with the wrong stride, does not return what the right read returns."""
    h, w = pic.shape
    assert stride >= w + ox
    buf = np.random.default_rng(9000 + seed).integers(0, 256, (h + 2 * oy, stride), dtype=np.uint8)
    buf[oy:oy + h, ox:ox + w] = pic
    return buf


# the ceiling pictures of noise detection: (method, analysed width, height, full width, height), each with both noise_detection_th and a
# luma_height on each side of 720 and of 1080 (the class ladders' offsets)
EDGE_NOISE_GEOMETRIES = ((FULL, 200, 196, 200, 196), (HALF, 136, 72, 544, 288), (QUARTER, 136, 72, 272, 144))
EDGE_LUMA_HEIGHTS = (720, 1080, 1088)
# (W, H, regions per width, per height): the reference's arrays end at 4 x 4 regions, the larger counts are the model's alone
EDGE_HIST_CASES = ((200, 136, 3, 2), (72, 40, 3, 2), (328, 200, 3, 2), (200, 136, 4, 4), (72, 40, 4, 4), (328, 200, 4, 4), (200, 136, 1, 1))
EDGE_HIST_MODEL_ONLY = ((200, 136, 8, 8), (328, 200, 5, 3))
# 1, 3, 6 and 24 SBs: 1, 3, 2 and 15 of them complete; the first three leave a last workgroup of four SBs partly filled
EDGE_SB_SIZES = ((64, 64), (192, 64), (136, 72), (328, 200))
EDGE_MEANVAR_KINDS = ("white", "halves", "checker", "random")


def edge_hist_planes(w, h, kind, seed):
    """-> (luma, padded full luma buffer, its (ox, oy), cb, cr): a random luma in a hostile buffer of odd stride, chroma of `kind`"""
    luma = edge_luma("random", w, h, seed)
    ox, oy = 20, 7
    return luma, hostile_plane(luma, ox, oy, w + 2 * ox + 5, seed), (ox, oy), edge_chroma(kind, w // 2, h // 2, seed + 1), edge_chroma(kind, w // 2, h // 2, seed + 2)


def edge_meanvar_plane(kind, w, h, seed):
    """-> (padded full luma buffer, origin_x, origin_y) of a block mean / variance case: the padding covers the partial SBs, which the
    reference reads, and it is noise, so every reader has to agree on the stride as well"""
    ox, oy = 68 + 3, 68
    return hostile_plane(edge_luma(kind, w, h, seed), ox, oy, w + 2 * ox + 5, 60 + seed), ox, oy

"""Pictures that put the ME kernels' packed sums at the ceiling of their fields (two or four 16-bit SAD sums per register, (sad << 16) | position
and (sad << 12) | position keys, the signed packed 16-bit half-pel filter): 8-bit pictures of 0 and 255 only, arranged so that a sum of N samples
reaches N * 255 -- 0.4 % below the capacity of the field that holds it -- while, in every kind but the all-tie ones, another position of the same
search area lies far below, so that a carry between two packed fields changes who wins.

content(kind, width, height, seed) -> [reference 0, current, reference 1], deterministic.  What each kind is for is asserted from numpy and the
oracle alone in tests/test_me_ceiling.py (the census), independently of the kernels under test."""
import numpy as np

KINDS = ("black_white", "pixel_checker", "row_stripes", "blocks", "one_match", "taps", "dented", "hme")
ALL_TIE = ("black_white", "dented")          # every search position of a PU has the same SAD: the first in raster order has to win
SIZES = ((200, 136), (192, 128))             # partial SBs both ways (the bottom SB row is 8 rows high); whole SBs
SIZE_FAST = (256, 328)                       # whole SB columns, six SB rows (the last one partial): the specialised 2160p instance serves it
# largest row-subsampled SAD (rows 0, 2, 4, .. doubled, the scale the full-pel search reports in dist0: oracle/oracle_me.c fullpel_position) of
# an N x N PU -- for 64 x 64 it equals the search's initial best SAD, MAX_SAD_VALUE
CEIL = {8: 8 * 8 * 255, 16: 16 * 16 * 255, 32: 32 * 32 * 255, 64: 64 * 64 * 255}
DENT = ((2, 2), (5, 3))                      # (x, y) inside every 64 x 64 source SB: one sample on an even row, one on an odd row, same 8 x 8 block


def content(kind, w, h, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    zero, full = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    if kind == "black_white":      # every sum at its ceiling, every position ties
        return [zero, full, zero.copy()]
    if kind == "dented":           # black_white two steps below MAX_SAD_VALUE: three of four 16x16 / 32x32 PUs stay at the ceiling
        cur = full.copy()
        for dx, dy in DENT:
            cur[dy::64, dx::64] = 254
        return [zero, cur, zero.copy()]
    if kind == "pixel_checker":    # 1-sample checkerboard against its inverse and its shift by one
        a = (((yy + xx) & 1) * 255).astype(np.uint8)
        return [a, 255 - a, np.roll(a, 1, 1)]
    if kind == "row_stripes":      # rows alternate: the row-subsampled SAD (rows 0, 2, 4, 6) and the full SAD disagree maximally
        a = ((yy & 1) * 255).astype(np.uint8)
        return [a, 255 - a, a.copy()]
    if kind == "blocks":           # random 0 / 255 blocks, 16x16 and (in alternate 64x64 tiles) 8x8, references displaced by (3, -3) and (-2, 5)
        H, W = h + 32, w + 32
        b16 = np.kron(rng.integers(0, 2, (H // 16 + 1, W // 16 + 1)), np.ones((16, 16), np.int64))[:H, :W]
        b8 = np.kron(rng.integers(0, 2, (H // 8 + 1, W // 8 + 1)), np.ones((8, 8), np.int64))[:H, :W]
        Y, X = np.mgrid[0:H, 0:W]
        big = (np.where((((Y - 16) // 64 + (X - 16) // 64) & 1) == 1, b8, b16) * 255).astype(np.uint8)
        return [np.ascontiguousarray(big[16 + dy:16 + dy + h, 16 + dx:16 + dx + w]) for dx, dy in ((3, -3), (0, 0), (-2, 5))]
    if kind == "one_match":        # the ceiling everywhere except around an isolated patch: far SBs have best SAD == MAX_SAD_VALUE
        ref = zero.copy()
        ref[h // 4:h // 4 + 70, w // 4:w // 4 + 70] = 255
        return [ref, full, 255 - ref]
    if kind == "taps":             # columns (rows in alternate 32x32 tiles) 255,0,0,255: both extremes of the half-pel filter
        a = (np.isin(xx & 3, (0, 3)) * 255).astype(np.uint8)
        b = (np.isin(yy & 3, (0, 3)) * 255).astype(np.uint8)
        ref = np.where(((xx // 32 + yy // 32) & 1).astype(bool), a, b).astype(np.uint8)
        return [ref, np.roll(ref, (1, 1), (0, 1)), np.roll(ref, (2, 1), (0, 1))]
    if kind == "hme":
        # 0 / 255 in blocks of 32x32 and 64x32 (a 32x32 checkerboard with random blocks flipped), displaced by multiples of 4: the point-decimated
        # 1/4 and 1/16 planes are themselves 0 / 255.  A 16x8 block of the 1/16 plane against the checkerboard shifted by 32 is all 255 against 0.
        # In every third 64x64 tile the current picture is 255 over references of 0: all HME levels tie there, at the ceiling of every level.
        H, W = h + 64, w + 64
        Y, X = np.mgrid[0:H, 0:W]
        chk = ((Y // 32 + X // 32) & 1)
        f32 = np.kron(rng.integers(0, 8, (H // 32 + 1, W // 32 + 1)) == 0, np.ones((32, 32), bool))[:H, :W]
        f64 = np.kron(rng.integers(0, 8, (H // 32 + 1, W // 64 + 1)) == 0, np.ones((32, 64), bool))[:H, :W]
        big = ((chk ^ f32 ^ f64) * 255).astype(np.uint8)
        out = [np.ascontiguousarray(big[32 + dy:32 + dy + h, 32 + dx:32 + dx + w]) for dx, dy in ((8, -4), (0, 0), (-12, 8))]
        flat = ((yy // 64) * 2 + xx // 64) % 3 == 2
        out[0][flat], out[1][flat], out[2][flat] = 0, 255, 0
        return out
    raise KeyError(kind)


def mixed_content(w, h, rng):
    """per 64x64 SB a random kind (or a smooth clip), so that ceiling SBs and ordinary SBs are neighbours (tools/me_fuzz.py ceil)"""
    import svt_testlib as T
    seed = int(rng.integers(1 << 20))
    srcs = [content(k, w, h, seed) for k in KINDS] + [T.gen_clip_subpel(w, h, 3, seed)]
    pick = rng.integers(0, len(srcs), ((h + 63) // 64, (w + 63) // 64))
    sel = np.kron(pick, np.ones((64, 64), np.int64))[:h, :w]
    return [np.choose(sel, [s[i] for s in srcs]).astype(np.uint8) for i in range(3)]

"""The open-loop intra search and the grid built from its records, restated on the host (test infrastructure):
  * oracle_ois: the records of svt_hip_intra_search_device, block by block from the oracle's reference-sample rule and predictors
    (svt_oracle_intra_ref_samples2 + svt_oracle_intra_predict, pinned against the reference by tests/test_intra_oracle.py) on the SOURCE;
  * model_grid: the decision svt_hip_md_intra_search_picture / _device state in include/svtvp9_hip.h, written bottom-up per SB (an
    independent formulation of the per-unit text in csrc/encdec_core.h);
  * random_ois: plausible random records (parents near the sum of their children, some UINT32_MAX parents)."""
import ctypes as C

import numpy as np

import svt_testlib as T

B = T.B
NONE = B.OIS_NONE
SIZES = ((32, 0), (16, 4), (8, 20), (4, 84))   # block size, first record of the size inside an SB


def zord(x, y):
    """z-order index: the bits of x in the even positions, of y in the odd ones"""
    v = 0
    for b in range(4):
        v |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
    return v


def unzord(z):
    x = y = 0
    for b in range(4):
        x |= ((z >> (2 * b)) & 1) << b
        y |= ((z >> (2 * b + 1)) & 1) << b
    return x, y


def inside_mask(W, H):
    """(n_sb, 340) bool: the block lies wholly inside the picture"""
    sb_cols, sb_rows = (W + 63) // 64, (H + 63) // 64
    out = np.zeros((sb_rows * sb_cols, B.OIS_PER_SB), bool)
    for sb in range(sb_rows * sb_cols):
        sx, sy = (sb % sb_cols) * 64, (sb // sb_cols) * 64
        for n, base in SIZES:
            for z in range((64 // n) ** 2):
                x, y = unzord(z)
                out[sb, base + z] = sx + n * (x + 1) <= W and sy + n * (y + 1) <= H
    return out


def random_ois(seed, W, H, none_share=0.1):
    rng = np.random.default_rng(seed)
    sb_cols, sb_rows = (W + 63) // 64, (H + 63) // 64
    n_sb = sb_cols * sb_rows
    o = np.zeros((n_sb, B.OIS_PER_SB), dtype=B.OIS_BLOCK_DTYPE)
    sad = np.zeros((n_sb, B.OIS_PER_SB), np.int64)
    uv = np.zeros((n_sb, B.OIS_PER_SB), np.int64)
    sad[:, 84:] = rng.integers(0, 500, (n_sb, 256))
    for n, base in SIZES[::-1][1:]:            # 8x8, 16x16, 32x32: near the sum of the four children
        cbase = {8: 84, 16: 20, 32: 4}[n]
        k = (64 // n) ** 2
        kids = sad[:, cbase:cbase + 4 * k].reshape(n_sb, k, 4).sum(axis=2)
        sad[:, base:base + k] = np.maximum(kids + rng.integers(-40 * n, 40 * n, (n_sb, k)), 0)
        if n == 8:
            uv[:, base:base + k] = rng.integers(0, 600, (n_sb, k))
        else:
            ukids = uv[:, cbase:cbase + 4 * k].reshape(n_sb, k, 4).sum(axis=2)
            uv[:, base:base + k] = np.maximum(ukids + rng.integers(-40 * n, 40 * n, (n_sb, k)), 0)
    o["sad"], o["uv_sad"] = sad, uv
    o["mode"], o["uv_mode"] = rng.integers(0, 10, (n_sb, B.OIS_PER_SB)), rng.integers(0, 10, (n_sb, B.OIS_PER_SB))
    o["uv_sad"][:, 84:], o["uv_mode"][:, 84:] = NONE, 0xFF
    off = ~inside_mask(W, H)
    gone = np.zeros_like(off)
    gone[:, :20] = rng.random((n_sb, 20)) < none_share       # some 16x16 / 32x32 parents inside the picture without a record
    for m in (off, gone):
        o["sad"][m], o["uv_sad"][m], o["mode"][m], o["uv_mode"][m] = NONE, NONE, 0xFF, 0xFF
    return o


def model_grid(ois, W, H, lam, level):
    """the grid of include/svtvp9_hip.h's decision rule, bottom-up per SB"""
    mi_rows, mi_cols, sb_cols, sb_rows = H // 8, W // 8, (W + 63) // 64, (H + 63) // 64
    lf = np.zeros((mi_rows, mi_cols), dtype=B.LF_MODE_INFO_DTYPE)
    for sb in range(sb_rows * sb_cols):
        sr, sc = sb // sb_cols, sb % sb_cols
        rec = ois[sb]
        sad, uv = rec["sad"].astype(np.int64), rec["uv_sad"].astype(np.int64)
        J = sad + uv + lam
        best8, as8 = {}, {}
        for r in range(8):
            for c in range(8):
                z = zord(c, r)
                j4 = int(sad[84 + 4 * z:88 + 4 * z].sum() + uv[20 + z] + lam)
                a = rec["sad"][20 + z] != NONE and int(J[20 + z]) <= j4
                as8[r, c], best8[r, c] = a, int(J[20 + z]) if a else j4
        best16, as16 = {}, {}
        for r16 in range(4):
            for c16 in range(4):
                s = sum(best8[2 * r16 + i, 2 * c16 + j] for i in (0, 1) for j in (0, 1))
                z = 4 + zord(c16, r16)
                fits = sr * 8 + 2 * r16 + 2 <= mi_rows and sc * 8 + 2 * c16 + 2 <= mi_cols
                a = fits and rec["sad"][z] != NONE and int(J[z]) <= s
                as16[r16, c16], best16[r16, c16] = a, int(J[z]) if a else s
        as32 = {}
        for r32 in range(2):
            for c32 in range(2):
                s = sum(best16[2 * r32 + i, 2 * c32 + j] for i in (0, 1) for j in (0, 1))
                z = zord(c32, r32)
                fits = sr * 8 + 4 * r32 + 4 <= mi_rows and sc * 8 + 4 * c32 + 4 <= mi_cols
                as32[r32, c32] = fits and rec["sad"][z] != NONE and int(J[z]) <= s
        for r in range(8):
            for c in range(8):
                ur, uc = sr * 8 + r, sc * 8 + c
                if ur >= mi_rows or uc >= mi_cols:
                    continue
                m = lf[ur, uc]
                m["filter_level"] = level
                if as32[r >> 2, c >> 2]:
                    b, st, tx = zord(c >> 2, r >> 2), 9, 3
                elif as16[r >> 1, c >> 1]:
                    b, st, tx = 4 + zord(c >> 1, r >> 1), 6, 2
                else:
                    b, st, tx = 20 + zord(c, r), (3 if as8[r, c] else 0), (1 if as8[r, c] else 0)
                m["sb_type"], m["tx_size"] = st, tx
                m["pad"][2] = rec["uv_mode"][b]
                if st:
                    m["pad"][1] = rec["mode"][b]
                else:
                    q = 84 + 4 * zord(c, r)
                    md = [int(rec["mode"][q + k]) & 15 for k in range(4)]
                    m["pad"][1], m["pad"][0] = md[0] | md[1] << 4, md[2] | md[3] << 4
    return lf


def host_grid(ois, W, H, lam, level, mi_stride=None):
    """the library's host form"""
    lf = np.zeros((H // 8, mi_stride or W // 8), dtype=B.LF_MODE_INFO_DTYPE)
    o = np.ascontiguousarray(ois)
    rc = B.load().svt_hip_md_intra_search_picture(o.ctypes.data_as(C.c_void_p), W, H, C.c_uint32(lam), level, lf.ctypes.data_as(C.c_void_p), lf.shape[1])
    assert rc == 0, rc
    return lf


_fns = None


def _oracle_fns():
    global _fns
    if _fns is None:
        lib = T.oracle()
        ref, pred = lib.svt_oracle_intra_ref_samples2, lib.svt_oracle_intra_predict
        ref.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        ref.restype = None
        pred.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        pred.restype = None
        _fns = ref, pred
    return _fns


def _block_sads(plane, x0, y0, n, have_right, bufs):
    """SAD of the ten predictions of the n x n block at (x0, y0) of a source plane (the oracle's reference samples of that plane)"""
    ref, pred = _oracle_fns()
    above, left, out = bufs[n]
    h, w = plane.shape
    ptr = plane.ctypes.data
    ref(ptr, w, x0, y0, n, have_right, above.ctypes.data, left.ctypes.data)
    for mode in range(10):
        pred(mode, n, int(x0 > 0), int(y0 > 0), above.ctypes.data + 1, left.ctypes.data, out.ctypes.data + mode * n * n, n)
    blk = plane[y0:y0 + n, x0:x0 + n].astype(np.int32)
    return np.abs(out.astype(np.int32) - blk).sum(axis=(1, 2))


def oracle_ois(src, sbs=None):
    """records of the SBs `sbs` (default: all) of the picture src = (Y, Cb, Cr) tight planes; other SBs are left zero"""
    H, W = src[0].shape
    planes = [np.ascontiguousarray(p) for p in src]
    sb_cols, sb_rows = (W + 63) // 64, (H + 63) // 64
    n_sb = sb_cols * sb_rows
    o = np.zeros((n_sb, B.OIS_PER_SB), dtype=B.OIS_BLOCK_DTYPE)
    bufs = {n: (np.zeros(2 * n + 1, np.uint8), np.zeros(n, np.uint8), np.zeros((10, n, n), np.uint8)) for n in (4, 8, 16, 32)}
    for sb in (range(n_sb) if sbs is None else sbs):
        sx, sy = (sb % sb_cols) * 64, (sb // sb_cols) * 64
        rec = o[sb]
        rec["sad"], rec["uv_sad"], rec["mode"], rec["uv_mode"] = NONE, NONE, 0xFF, 0xFF
        for n, base in SIZES:
            for z in range((64 // n) ** 2):
                bx, by = unzord(z)
                x0, y0 = sx + n * bx, sy + n * by
                if x0 + n > W or y0 + n > H:
                    continue
                s = _block_sads(planes[0], x0, y0, n, int(n == 4 and bx % 2 == 0), bufs)
                m = int(np.argmin(s))                       # (the first minimum: ties to the lowest mode)
                rec["sad"][base + z], rec["mode"][base + z] = s[m], m
                if n >= 8:
                    cs = sum(_block_sads(planes[k], x0 // 2, y0 // 2, n // 2, 0, bufs) for k in (1, 2))
                    m = int(np.argmin(cs))
                    rec["uv_sad"][base + z], rec["uv_mode"][base + z] = cs[m], m
    return o

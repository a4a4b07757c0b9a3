"""The mixed stand-in decision (svt_hip_md_mixed_picture / _batch_device) restated on the host (test infrastructure).

model(): the rule as include/svtvp9_hip.h states it, on whole-picture arrays: one cost plane per block size (64, 32, 16, 8) over the
picture rounded up to whole SBs, the merges as array comparisons from the 16x16 plane upwards, the chosen leaf spread back over the 8x8
units.  Nothing here walks a unit's tree the way the per-unit text of csrc/encdec_core.h does.
random_me(): ME records of the magnitude intra_search_model.random_ois gives its records, so that both sides win leaves.
host(): the library's host form."""
import ctypes as C

import numpy as np

import intra_search_model as S
import svt_testlib as T

B = T.B
NONE = B.OIS_NONE
# block size -> (first PU of the size, first OIS record of the size or None, sb_type, tx_size)
LEVELS = {64: (0, None, 12, 3), 32: (1, 0, 9, 3), 16: (5, 4, 6, 2), 8: (21, 20, 3, 1)}
_ZMAP = {k: np.array([[S.zord(x, y) for x in range(k)] for y in range(k)]) for k in (1, 2, 4, 8)}


def planes(per_sb, n, W, H):
    """(n_sb, blocks of size n in z-order) -> the plane of that size over the picture rounded up to whole SBs"""
    sb_cols, sb_rows, k = (W + 63) // 64, (H + 63) // 64, 64 // n
    a = per_sb.reshape(sb_rows, sb_cols, k * k)[:, :, _ZMAP[k]]                   # (sb_rows, sb_cols, y, x)
    return a.transpose(0, 2, 1, 3).reshape(sb_rows * k, sb_cols * k)


def fits(n, W, H):
    """the block of size n at every position of that plane lies wholly inside the picture"""
    sb_cols, sb_rows, k = (W + 63) // 64, (H + 63) // 64, 64 // n
    y, x = np.meshgrid(np.arange(sb_rows * k), np.arange(sb_cols * k), indexing="ij")
    return ((y + 1) * n <= H) & ((x + 1) * n <= W)


def quad_sum(a):
    return a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]


def up(a, f):
    return np.repeat(np.repeat(a, f, axis=0), f, axis=1)


def model(me, ois, W, H, lam, penalty, level):
    """-> (mc grid, lf grid, number of intra units)"""
    n_sb = me.shape[0]
    inter, intra, pu, rec = {}, {}, {}, {}
    for n, (p0, o0, _, _) in LEVELS.items():
        k2 = (64 // n) ** 2
        inter[n] = planes(me["dist0"][:, p0:p0 + k2].astype(np.int64), n, W, H)
        pu[n] = planes(np.arange(n_sb)[:, None] * 85 + p0 + np.arange(k2)[None, :], n, W, H)
        if o0 is None:
            intra[n] = np.full(inter[n].shape, 1 << 62, np.int64)                 # no intra 64x64
            rec[n] = np.zeros(inter[n].shape, np.int64)
        else:
            sad = planes(ois["sad"][:, o0:o0 + k2].astype(np.int64), n, W, H)
            intra[n] = np.where(sad == NONE, 1 << 62, sad + penalty)
            rec[n] = planes(np.arange(n_sb)[:, None] * B.OIS_PER_SB + o0 + np.arange(k2)[None, :], n, W, H)
    cost = {n: np.minimum(inter[n], intra[n]) for n in LEVELS}
    s16 = quad_sum(cost[16])
    merge32 = fits(32, W, H) & (cost[32] <= s16 + 3 * lam)
    val32 = np.where(merge32, cost[32] + lam, s16 + 4 * lam)
    merge64 = fits(64, W, H) & (cost[64] + lam <= quad_sum(val32))
    # the size of the leaf that covers every 8x8 unit (the plane of units over whole SBs)
    size = np.where(up(merge64, 8), 64, np.where(up(merge32, 4), 32, np.where(up(fits(16, W, H), 2), 16, 8)))
    mi_rows, mi_cols = H // 8, W // 8
    mc = np.zeros((mi_rows, mi_cols), dtype=B.MC_MODE_INFO_DTYPE)
    lf = np.zeros((mi_rows, mi_cols), dtype=B.LF_MODE_INFO_DTYPE)
    flat_me, flat_ois = me.reshape(-1), ois.reshape(-1)
    for n, (_, _, sb_type, tx) in LEVELS.items():
        sel = (size == n)[:mi_rows, :mi_cols]
        if not sel.any():
            continue
        f = n // 8
        is_intra = up(intra[n] < inter[n], f)[:mi_rows, :mi_cols][sel]
        m = flat_me[up(pu[n], f)[:mi_rows, :mi_cols][sel]]
        o = flat_ois[up(rec[n], f)[:mi_rows, :mi_cols][sel]]
        d = m["dir0"].astype(np.int64)
        g = np.zeros(int(sel.sum()), dtype=B.MC_MODE_INFO_DTYPE)
        g["bw8"] = g["bh8"] = f
        g["ref_list"][:, 0] = np.where(is_intra, -1, d == 1)
        g["ref_list"][:, 1] = np.where(~is_intra & (d == 2), 1, -1)
        g["mv_row"][:, 0] = np.where(is_intra, 0, 2 * np.where(d == 1, m["y_mv_l1"], m["y_mv_l0"]).astype(np.int32))
        g["mv_col"][:, 0] = np.where(is_intra, 0, 2 * np.where(d == 1, m["x_mv_l1"], m["x_mv_l0"]).astype(np.int32))
        g["mv_row"][:, 1] = np.where(~is_intra & (d == 2), 2 * m["y_mv_l1"].astype(np.int32), 0)
        g["mv_col"][:, 1] = np.where(~is_intra & (d == 2), 2 * m["x_mv_l1"].astype(np.int32), 0)
        mc[sel] = g
        h = np.zeros(int(sel.sum()), dtype=B.LF_MODE_INFO_DTYPE)
        h["sb_type"], h["tx_size"], h["is_inter"], h["filter_level"] = sb_type, tx, ~is_intra, level
        h["pad"][:, 1] = np.where(is_intra, o["mode"], 0)
        h["pad"][:, 2] = np.where(is_intra, o["uv_mode"], 0)
        lf[sel] = h
    return mc, lf, int((lf["is_inter"] == 0).sum())


def random_me(seed, W, H, scale=1.0):
    """ME records whose distortions have the magnitude of random_ois' SADs: 8x8 PUs random, every parent near the sum of its children"""
    rng = np.random.default_rng(seed)
    n_sb = ((W + 63) // 64) * ((H + 63) // 64)
    me = np.zeros((n_sb, 85), dtype=B.ME_RESULT_DTYPE)
    dist = np.zeros((n_sb, 85), np.int64)
    dist[:, 21:] = rng.integers(0, int(2000 * scale) + 1, (n_sb, 64))
    for p0, c0, k in ((5, 21, 16), (1, 5, 4), (0, 1, 1)):
        kids = dist[:, c0:c0 + 4 * k].reshape(n_sb, k, 4).sum(axis=2)
        spread = np.maximum(kids // 8, 1)
        dist[:, p0:p0 + k] = np.maximum(kids + rng.integers(-spread, spread + 1), 0)
    me["dist0"] = dist
    me["dir0"] = rng.integers(0, 3, (n_sb, 85))
    me["dist1"], me["dist2"] = dist + 7, dist + 11
    for f in ("x_mv_l0", "y_mv_l0", "x_mv_l1", "y_mv_l1"):
        me[f] = rng.integers(-200, 201, (n_sb, 85))
    me["total"] = 3
    return me


def host(me, ois, W, H, lam, penalty, level, mi_stride=None, fill=0):
    """the library's host form -> (mc grid, lf grid, count), grids mi_stride wide"""
    stride = mi_stride or W // 8
    mc = np.full((H // 8, stride * 12), fill, np.uint8).view(B.MC_MODE_INFO_DTYPE)
    lf = np.full((H // 8, stride * 8), fill, np.uint8).view(B.LF_MODE_INFO_DTYPE)
    n = C.c_int32(-1)
    me_c, ois_c = np.ascontiguousarray(me), np.ascontiguousarray(ois)
    rc = B.load().svt_hip_md_mixed_picture(me_c.ctypes.data_as(C.c_void_p), ois_c.ctypes.data_as(C.c_void_p), W, H, lam, penalty, level, mc.ctypes.data_as(C.c_void_p),
                                           lf.ctypes.data_as(C.c_void_p), stride, C.byref(n))
    assert rc == 0, rc
    return mc, lf, n.value


def host_default(me, W, H, lam, level):
    mc = np.zeros((H // 8, W // 8), dtype=B.MC_MODE_INFO_DTYPE)
    lf = np.zeros((H // 8, W // 8), dtype=B.LF_MODE_INFO_DTYPE)
    me_c = np.ascontiguousarray(me)
    assert B.load().svt_hip_md_default_picture(me_c.ctypes.data_as(C.c_void_p), W, H, C.c_uint32(lam), level, mc.ctypes.data_as(C.c_void_p), lf.ctypes.data_as(C.c_void_p),
                                               W // 8) == 0
    return mc, lf

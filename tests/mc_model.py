"""What an inter-prediction case makes svt_mc_kernel do: a plain numpy model of the per-unit derivation and of the work mapping.

Written from the contract in include/svtvp9_hip.h (svt_mc_mode_info, svt_mc_picture) and from the reference
(VPX/vp9_reconinter.c: eb_vp9_clamp_mv_to_umv_border_sb :68-87, build_inter_predictors :129-187; the edge distances of
Codec/EbEncDecProcess.c:3708-3719), not from the kernel.  It supplies coverage facts (which filter phases, load shifts, clamp
sides and wave modes a case reaches) and bounds (which bytes of the reference planes are read).  It never supplies expected
samples: those come from oracle/oracle_mc.c.

Work mapping (the mapping paragraph of csrc/mc_kernel.hip): a workgroup covers 32 units of one mode-info row; wave 0 holds the
luma lanes (two 4 x 8 tiles per unit), wave 1 the Cb lanes then the Cr lanes (one 4 x 4 tile per unit and plane).  A lane loads
NR + 7 rows of 16 bytes (NR = 8 luma, 4 chroma) that start `shift` bytes before sample x - 3 of its window, shift = (address of
that sample) & 3.  A wave in which no lane has a vertical phase loads only its NR rows; one in which no lane has a horizontal
phase skips the taps.  Both are decided per reference iteration k, among the lanes that take part in it.
"""
import collections

import numpy as np

# VP9 specification, subpel_filters[REGULAR] (= VPX/vp9_filter.c:32-47)
TAPS = np.array([[0, 0, 0, 128, 0, 0, 0, 0], [0, 1, -5, 126, 8, -3, 1, 0], [-1, 3, -10, 122, 18, -6, 2, 0], [-1, 4, -13, 118, 27, -9, 3, -1],
                 [-1, 4, -16, 112, 37, -11, 4, -1], [-1, 5, -18, 105, 48, -14, 4, -1], [-1, 5, -19, 97, 58, -16, 5, -1],
                 [-1, 6, -19, 88, 68, -18, 5, -1], [-1, 6, -19, 78, 78, -19, 6, -1], [-1, 5, -18, 68, 88, -19, 6, -1],
                 [-1, 5, -16, 58, 97, -19, 5, -1], [-1, 4, -14, 48, 105, -18, 5, -1], [-1, 4, -11, 37, 112, -16, 4, -1],
                 [-1, 3, -9, 27, 118, -13, 4, -1], [0, 2, -6, 18, 122, -10, 3, -1], [0, 1, -3, 8, 126, -5, 1, 0]], np.int64)

LANE_DTYPE = np.dtype([("plane", "i1"), ("k", "i1"), ("list", "i1"), ("mi_row", "i4"), ("mi_col", "i4"), ("x", "i4"), ("y", "i4"), ("wg", "i4"), ("wave", "i1"),
                       ("bw8", "u1"), ("bh8", "u1"), ("compound", "?"), ("mv_row", "i4"), ("mv_col", "i4"), ("lo_col", "i4"), ("hi_col", "i4"),
                       ("lo_row", "i4"), ("hi_row", "i4"), ("clamp_col", "i1"), ("clamp_row", "i1"), ("s_row", "i4"), ("s_col", "i4"), ("sx", "i1"), ("sy", "i1"),
                       ("shift", "i1"), ("any_sx", "?"), ("any_sy", "?")])
# mv_row / mv_col: the clamped MV in 1/16 sample of the plane; lo_* / hi_*: the clamp bounds in the same unit;
# clamp_col: -1 the left bound replaced the MV, +1 the right one, 0 the MV was inside (a MV equal to a bound is inside); clamp_row: -1 top, +1 bottom


def default_geometry(case):
    """{(list, plane): (address of sample (0, 0) mod 4, stride)} of the padded planes of the case when every buffer starts at a
    multiple of 4 (what svt_hip_inter_pred_frame makes of them)"""
    g, pad = {}, case["pad"]
    for l, planes in enumerate(case["refs"]):
        for p, a in enumerate(planes):
            o = pad if p == 0 else pad // 2
            g[(l, p)] = ((o * a.shape[1] + o) & 3, a.shape[1])
    return g


def clamp_bounds(mi_rows, mi_cols, mi_row, mi_col, bw8, bh8, plane):
    """((lo_col, hi_col, lo_row, hi_row), scale) of eb_vp9_clamp_mv_to_umv_border_sb for the block that holds unit (mi_row, mi_col):
    the bounds in 1/16 sample of the plane, and the factor that takes a MV of svt_mc_mode_info (1/8 luma sample) to that unit
    (2 for luma, 1 for chroma).  Scalars or arrays."""
    ss = 1 if plane else 0
    scale = 1 << (1 - ss)
    bc, br = mi_col - mi_col % bw8, mi_row - mi_row % bh8
    to_left, to_right = -(bc * 8) * 8, ((mi_cols - bw8 - bc) * 8) * 8          # mb_to_left_edge / mb_to_right_edge
    to_top, to_bottom = -(br * 8) * 8, ((mi_rows - bh8 - br) * 8) * 8
    bw, bh = (bw8 * 8) >> ss, (bh8 * 8) >> ss
    spel_left, spel_top = (4 + bw) << 4, (4 + bh) << 4                           # VP9_INTERP_EXTEND = 4, SUBPEL_BITS = 4
    spel_right, spel_bottom = spel_left - 16, spel_top - 16                      # SUBPEL_SHIFTS = 16
    return (to_left * scale - spel_left, to_right * scale + spel_right, to_top * scale - spel_top, to_bottom * scale + spel_bottom), scale


def mc_lanes(case, geometry=None):
    """one LANE_DTYPE record per lane and reference iteration that the kernel runs for the case"""
    geometry = geometry or default_geometry(case)
    mi, R, C = case["mi"], case["mi_rows"], case["mi_cols"]
    rr, cc = np.meshgrid(np.arange(R, dtype=np.int64), np.arange(C, dtype=np.int64), indexing="ij")
    bw8, bh8 = mi["bw8"].astype(np.int64), mi["bh8"].astype(np.int64)
    inter = (mi["ref_list"][:, :, 0] >= 0) & (bw8 >= 1) & (bh8 >= 1)
    compound = mi["ref_list"][:, :, 1] >= 0
    sbw, sbh = np.maximum(bw8, 1), np.maximum(bh8, 1)
    xblocks = (C + 31) // 32
    out = []
    for plane in range(3):
        ss = 1 if plane else 0
        (lo_c, hi_c, lo_r, hi_r), scale = clamp_bounds(R, C, rr, cc, sbw, sbh, plane)
        for k in range(2):
            on = inter & (compound if k else True)
            lst = (mi["ref_list"][:, :, k] != 0).astype(np.int64)
            # MV clamped_mv = {src_mv->row * (1 << (1 - ss_y)), ...}: an MV holds int16, so a luma MV beyond +-16383 wraps here
            raw_r = (mi["mv_row"][:, :, k].astype(np.int64) * scale).astype(np.int16).astype(np.int64)
            raw_c = (mi["mv_col"][:, :, k].astype(np.int64) * scale).astype(np.int16).astype(np.int64)
            mv_r, mv_c = np.clip(raw_r, lo_r, hi_r), np.clip(raw_c, lo_c, hi_c)
            if case["use_subpel"]:
                s_r, s_c = mv_r, mv_c
                sy, sx = s_r & 15, s_c & 15
            elif plane:    # vp9_reconinter.c:172-176: rounded to half samples, and only three bits of the phase are looked at
                s_r, s_c = (mv_r + 4) & ~7, (mv_c + 4) & ~7
                sy, sx = s_r & 7, s_c & 7
            else:
                s_r, s_c = (mv_r + 8) & ~15, (mv_c + 8) & ~15
                sy, sx = s_r & 15, s_c & 15
            for tile in range(1 if plane else 2):
                n = int(on.sum())
                a = np.zeros(n, LANE_DTYPE)
                x, y = (cc * 8 + 4 * tile if plane == 0 else cc * 4)[on], (rr * (4 if plane else 8))[on]
                a["plane"], a["k"], a["list"], a["mi_row"], a["mi_col"], a["x"], a["y"] = plane, k, lst[on], rr[on], cc[on], x, y
                a["wg"], a["wave"] = (rr * xblocks + cc // 32)[on], 1 if plane else 0
                a["bw8"], a["bh8"], a["compound"] = bw8[on], bh8[on], compound[on]
                a["mv_row"], a["mv_col"], a["lo_col"], a["hi_col"], a["lo_row"], a["hi_row"] = mv_r[on], mv_c[on], lo_c[on], hi_c[on], lo_r[on], hi_r[on]
                a["clamp_col"] = (raw_c[on] > hi_c[on]).astype(int) - (raw_c[on] < lo_c[on])
                a["clamp_row"] = (raw_r[on] > hi_r[on]).astype(int) - (raw_r[on] < lo_r[on])
                a["s_row"], a["s_col"], a["sx"], a["sy"] = s_r[on], s_c[on], sx[on], sy[on]
                sh = np.zeros(n, np.int64)
                for l in (0, 1):
                    base, stride = geometry[(l, plane)]
                    sh = np.where(lst[on] == l, (base + (y + (s_r[on] >> 4) - 3) * stride + x + (s_c[on] >> 4) - 3) & 3, sh)
                a["shift"] = sh
                out.append(a)
    a = np.concatenate(out)
    # the wave's ballots: over the lanes of one workgroup, wave and reference iteration
    key = (a["wg"].astype(np.int64) * 2 + a["wave"]) * 2 + a["k"]
    nk = int(key.max()) + 1 if len(key) else 0
    for name, ph in (("any_sx", "sx"), ("any_sy", "sy")):
        any_ = np.zeros(nk, bool)
        np.logical_or.at(any_, key, a[ph] != 0)
        a[name] = any_[key]
    return a


SIDES = {(0, 0): "", (-1, 0): "L", (1, 0): "R", (0, -1): "T", (0, 1): "B", (-1, -1): "TL", (1, -1): "TR", (-1, 1): "BL", (1, 1): "BR"}


def mc_census(case, geometry=None):
    """Counter of lanes per class (plane, any_sx, any_sy, sx == 0, sy == 0, shift, sx, sy, compound, clamp side, k); plane is
    0 luma / 1 chroma, the clamp side one of SIDES' values"""
    a = mc_lanes(case, geometry)
    cnt = collections.Counter()
    for t in zip(np.minimum(a["plane"], 1).tolist(), a["any_sx"].tolist(), a["any_sy"].tolist(), (a["sx"] == 0).tolist(), (a["sy"] == 0).tolist(),
                 a["shift"].tolist(), a["sx"].tolist(), a["sy"].tolist(), a["compound"].tolist(), a["clamp_col"].tolist(), a["clamp_row"].tolist(), a["k"].tolist()):
        cnt[t[:9] + (SIDES[(t[9], t[10])], t[11])] += 1
    return cnt


def mc_read_extent(case, geometry=None, origins=None):
    """{(list, plane): (lowest, highest)} byte offsets, relative to the first byte of the padded plane, that the lanes of the case
    read; planes nothing reads are left out.  origins: {(list, plane): offset of sample (0, 0)}, default the case's padding."""
    geometry = geometry or default_geometry(case)
    a = mc_lanes(case, geometry)
    ext, pad = {}, case["pad"]
    for (l, plane), (_, stride) in geometry.items():
        m = (a["list"] == l) & (a["plane"] == plane)
        if not m.any():
            continue
        b = a[m]
        nr = 4 if plane else 8
        o = pad if plane == 0 else pad // 2
        org = origins[(l, plane)] if origins else o * stride + o
        row0 = b["y"].astype(np.int64) + (b["s_row"] >> 4) - np.where(b["any_sy"], 3, 0)
        row1 = row0 + np.where(b["any_sy"], nr + 7, nr) - 1
        col0 = b["x"].astype(np.int64) + (b["s_col"] >> 4) - 3 - b["shift"]
        ext[(l, plane)] = (int((org + row0 * stride + col0).min()), int((org + row1 * stride + col0 + 15).max()))
    return ext


def mc_tile_sums(case, lane):
    """The filter sums of one lane (a LANE_DTYPE record) before rounding, as int64 convolutions of its own window of the case's
    reference plane: (horizontal sums [rows, 4] or None without a horizontal phase, the vertical pass's input [NR + 7, 4], vertical
    sums [NR, 4] or None).  Row i of the first two is row y - 3 + i of the window.  For coverage facts, not for expected samples."""
    plane, nr = int(lane["plane"]), 4 if lane["plane"] else 8
    ref = case["refs"][int(lane["list"])][plane]
    org = case["pad"] >> (1 if plane else 0)
    y0, x0 = org + int(lane["y"]) + (int(lane["s_row"]) >> 4) - 3, org + int(lane["x"]) + (int(lane["s_col"]) >> 4) - 3
    win = ref[y0:y0 + nr + 7, x0:x0 + 11].astype(np.int64)
    hs = vs = None
    mid = win[:, 3:7]
    if lane["sx"]:
        hs = sum(win[:, k:k + 4] * TAPS[lane["sx"], k] for k in range(8))
        mid = np.clip((hs + 64) >> 7, 0, 255)
    if lane["sy"]:
        vs = sum(mid[k:k + nr] * TAPS[lane["sy"], k] for k in range(8))
    return hs, mid, vs

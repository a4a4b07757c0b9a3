"""The model of what an inter-prediction case makes the kernel do (tests/mc_model.py) and the coverage each constructed case of
svt_testlib.MC_EDGE_CASES is built for.  CPU only.  The model is pinned to the oracle first; then every case carries its census, so
that a change to a generator cannot quietly empty the class it exists for; then the bytes the kernel reads are bounded."""
import collections

import numpy as np
import pytest

import mc_model as M
import svt_testlib as T

B = T.B


def _census(name):
    return sum((M.mc_census(c) for c in T.make_mc_edge_case(name)), collections.Counter())


# census key fields
PLANE, ANY_SX, ANY_SY, SX0, SY0, SHIFT, SX, SY, COMPOUND, SIDE, K = range(11)


# ---- the model against the oracle ------------------------------------------------------------------------------------------
def _impulse_case(mv_row, mv_col, use_subpel, pos):
    """64x64, one 8x8 inter block at unit (3, 4) on list 0; the reference planes are 0 but for one sample of 255 at `pos` (luma) and
    pos / 2 (chroma)"""
    refs = [tuple(np.zeros((64 + 160 >> s, 64 + 160 >> s), np.uint8) for s in (0, 1, 1)) for _ in range(2)]
    for s, a in zip((0, 1, 1), refs[0]):
        a[(80 >> s) + (pos[0] >> s), (80 >> s) + (pos[1] >> s)] = 255
    mi = np.zeros((8, 8), dtype=B.MC_MODE_INFO_DTYPE)
    mi["ref_list"] = -1
    mi[3, 4]["bw8"], mi[3, 4]["bh8"] = 1, 1
    mi["ref_list"][3, 4] = (0, -1)
    mi["mv_row"][3, 4, 0], mi["mv_col"][3, 4, 0] = mv_row, mv_col
    return dict(mi=mi, mi_rows=8, mi_cols=8, refs=refs, pad=80, use_subpel=use_subpel, width=64, height=64)


@pytest.mark.parametrize("use_subpel,mvs", [
    (1, [(0, 0), (8, -8), (5, -3), (-13, 26), (16, 7), (-1, -1), (33, -40)]),
    # full-sample rounding: luma to the nearest sample, halves up; chroma to the nearest half sample, of which only three bits are
    # tested, so a chroma position that rounds to a half sample is copied from the sample below it (4 -> 8 -> sample 0, no phase)
    (0, [(0, 0), (3, 4), (4, 3), (-4, -5), (11, 12), (-12, 20), (7, -9), (28, -11), (-3, 36)]),
])
def test_model_positions_reproduce_the_oracle(use_subpel, mvs):
    """an impulse in the reference appears in the prediction where the model's (s_row, s_col) say, with the taps of its phases"""
    for (mv_row, mv_col) in mvs:
        case = _impulse_case(mv_row, mv_col, use_subpel, (30, 38))
        out = T.oracle_mc_frame(case)
        lanes = M.mc_lanes(case)
        assert len(lanes) == 4 and not lanes["clamp_col"].any() and not lanes["clamp_row"].any()
        hit = False
        for lane in lanes:
            nr = 4 if lane["plane"] else 8
            _, mid, vs = M.mc_tile_sums(case, lane)
            exp = mid[3:3 + nr] if vs is None else np.clip((vs + 64) >> 7, 0, 255)
            got = out[lane["plane"]][lane["y"]:lane["y"] + nr, lane["x"]:lane["x"] + 4]
            assert np.array_equal(got, exp), (mv_row, mv_col, int(lane["plane"]), got, exp)
            hit |= bool(exp.any())
        assert hit  # the impulse is inside the block's window: a wrong position would not go unseen
    if not use_subpel:
        quirk = M.mc_lanes(_impulse_case(3, 4, 0, (30, 38)))
        c = quirk[quirk["plane"] == 1][0]
        assert (c["s_col"], c["sx"], c["s_row"], c["sy"]) == (8, 0, 0, 0)       # half a sample kept in the position, not in the phase
        l = quirk[quirk["plane"] == 0][0]
        assert (l["s_col"], l["s_row"]) == (16, 0)                               # 2 * 4 = 8 sixteenths rounds up to a sample, 2 * 3 down


def test_model_wraps_luma_mvs_like_the_reference():
    """the reference scales a MV into int16 fields: +-32768 / 32767 eighths become 0 / -2 sixteenths of a luma sample, and are
    clamped only in chroma"""
    case = _impulse_case(-32768, 32767, 1, (30, 38))
    lanes = M.mc_lanes(case)
    l, c = lanes[lanes["plane"] == 0][0], lanes[lanes["plane"] == 1][0]
    assert (l["mv_row"], l["mv_col"], l["clamp_row"], l["clamp_col"]) == (0, -2, 0, 0)
    assert (c["clamp_row"], c["clamp_col"]) == (-1, 1)


# ---- the bytes read ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.MC_EDGE_CASES)
def test_reads_stay_inside_planes_padded_by_80(name):
    """svt_mc_picture promises the kernel 80 luma samples of padding (40 in chroma), and svt_hip_inter_pred_frame accepts no less.
    Every 16-byte row a lane loads lies inside such a plane, whatever the plane's base address is modulo 4."""
    for case in T.make_mc_edge_case(name):
        assert case["pad"] == 80
        for base in range(4):
            geo = {k: ((b + base) & 3, s) for k, (b, s) in M.default_geometry(case).items()}
            for (l, p), (lo, hi) in M.mc_read_extent(case, geo).items():
                assert 0 <= lo and hi < case["refs"][l][p].size, (case["key"], l, p, base, lo, hi)


def test_read_window_of_the_padding_contract():
    """what include/svtvp9_hip.h states beside svt_mc_picture: rows -(bh + 7) .. H + bh + 6 and, in those rows, bytes
    -(bw + 10) .. W + bw + 11 around a plane of W x H samples with blocks of bw x bh: the bounds are reached and never passed"""
    ext = collections.defaultdict(lambda: [0, 0, 0, 0])
    for case in T.make_mc_edge_case("clamps"):
        for base in range(4):
            geo = {k: ((b + base) & 3, s) for k, (b, s) in M.default_geometry(case).items()}
            a = M.mc_lanes(case, geo)
            ss = (a["plane"] > 0).astype(int)
            nr = 8 >> ss
            bw, bh = (a["bw8"].astype(int) * 8) >> ss, (a["bh8"].astype(int) * 8) >> ss
            W, H = case["width"] >> ss, case["height"] >> ss
            top = a["y"] + (a["s_row"] >> 4) - np.where(a["any_sy"], 3, 0)
            bot = top + np.where(a["any_sy"], nr + 7, nr) - 1
            left = a["x"] + (a["s_col"] >> 4) - 3 - a["shift"]
            for key, v in zip(zip(bw.tolist(), bh.tolist()), zip((-top - bh).tolist(), (bot - H - bh).tolist(), (-left - bw).tolist(), (left + 15 - W - bw).tolist())):
                ext[key] = [max(x, y) for x, y in zip(ext[key], v)]
    assert len(ext) == len(T.MC_BLOCK_SIZES) + 3        # the luma sizes and, below 8x8, chroma's 4x4, 4x8 and 8x4
    for key, v in ext.items():
        assert v == [7, 6, 10, 11], (key, v)


# ---- what each case reaches --------------------------------------------------------------------------------------------------
def test_phases_case_has_every_phase_pair_at_every_load_shift():
    cen = _census("phases")
    assert {k[SIDE] for k in cen} == {""} and not any(k[COMPOUND] for k in cen)
    chroma = {(k[SX], k[SY], k[SHIFT]) for k in cen if k[PLANE] == 1}
    luma = {(k[SX], k[SY], k[SHIFT]) for k in cen if k[PLANE] == 0}
    assert chroma == {(sx, sy, sh) for sx in range(16) for sy in range(16) for sh in range(4)}
    assert luma == {(sx, sy, sh) for sx in range(0, 16, 2) for sy in range(0, 16, 2) for sh in range(4)}


def test_wave_modes_case_reaches_every_wave_mode():
    sub1, sub0 = T.make_mc_edge_case("wave_modes")
    assert sub1["width"] == 256 and sub1["use_subpel"] == 1 and sub0["use_subpel"] == 0 and sub0["mi"] is sub1["mi"]
    cen = M.mc_census(sub1)
    lanes_per_mode = collections.Counter()
    for k, n in cen.items():
        lanes_per_mode[(k[PLANE], k[K], k[ANY_SX], k[ANY_SY])] += n
    for plane in (0, 1):
        for it in (0, 1):
            for mode in ((False, False), (False, True), (True, False), (True, True)):
                assert lanes_per_mode[(plane, it) + mode] >= 64, (plane, it, mode, lanes_per_mode)
    for plane in (0, 1):
        assert any(k[PLANE] == plane and k[ANY_SX] and k[SX0] for k in cen)    # a phase-0 lane among lanes that filter horizontally
        assert any(k[PLANE] == plane and k[ANY_SY] and k[SY0] for k in cen)    # ... vertically
        # the horizontal-only and vertical-only waves see every phase at every load shift, the copying ones every shift
        ph = range(1, 16) if plane else range(2, 16, 2)
        assert {(k[SX], k[SHIFT]) for k in cen if k[PLANE] == plane and k[ANY_SX] and not k[ANY_SY]} >= {(p, s) for p in ph for s in range(4)}
        assert {(k[SY], k[SHIFT]) for k in cen if k[PLANE] == plane and k[ANY_SY] and not k[ANY_SX]} >= {(p, s) for p in ph for s in range(4)}
        assert {k[SHIFT] for k in cen if k[PLANE] == plane and not k[ANY_SX] and not k[ANY_SY]} == {0, 1, 2, 3}
    # the lone lanes: one unit (its two luma tiles, resp. its Cb and Cr tile) has the phase and the other 62 lanes of the wave none
    a = M.mc_lanes(sub1)
    for band, ph, other in (("one_horz", "sx", "sy"), ("one_vert", "sy", "sx")):
        (row,) = sub1["bands"][band]
        for wave in (0, 1):
            w = a[(a["mi_row"] == row) & (a["wave"] == wave)]
            assert len(w) == 64 and int((w[ph] != 0).sum()) == 2 and not w[other].any()
    (row,) = sub1["bands"]["reverse"]
    for wave in (0, 1):
        w = a[(a["mi_row"] == row) & (a["wave"] == wave)]
        assert len(w) == 64 and int(((w["sx"] == 0) & (w["sy"] == 0)).sum()) == 2 and int(((w["sx"] != 0) & (w["sy"] != 0)).sum()) == 62
    # without sub-sample motion every wave copies
    assert {(k[ANY_SX], k[ANY_SY]) for k in M.mc_census(sub0)} == {(False, False)}


def test_wave_modes_references_are_not_flat_under_the_shortcuts():
    """in every single-list band, nearly every tile with a phase differs from the unfiltered window at its position: a shortcut
    taken wrongly, or a phase dropped, changes samples"""
    case = T.make_mc_edge_case("wave_modes")[0]
    out = T.oracle_mc_frame(case)
    a = M.mc_lanes(case)
    for band, rows in case["bands"].items():
        if band.startswith("c_") or band == "copy":
            continue
        for wave in (0, 1):
            w = a[np.isin(a["mi_row"], rows) & (a["wave"] == wave) & ((a["sx"] != 0) | (a["sy"] != 0))]
            differ = 0
            for lane in w:
                nr, org = (4, 40) if lane["plane"] else (8, 80)
                ref = case["refs"][lane["list"]][lane["plane"]]
                y0, x0 = org + lane["y"] + (lane["s_row"] >> 4), org + lane["x"] + (lane["s_col"] >> 4)
                differ += not np.array_equal(out[lane["plane"]][lane["y"]:lane["y"] + nr, lane["x"]:lane["x"] + 4], ref[y0:y0 + nr, x0:x0 + 4])
            assert len(w) >= 2 and differ == len(w), (band, wave, differ, len(w))


def test_ceilings_case_reaches_the_largest_and_smallest_filter_sums():
    (case,) = T.make_mc_edge_case("ceilings")
    for l in (0, 1):
        for a in case["refs"][l]:
            assert set(np.unique(a)) == {0, 255}
    top = 255 * np.where(M.TAPS > 0, M.TAPS, 0).sum(axis=1)
    bottom = 255 * np.where(M.TAPS < 0, M.TAPS, 0).sum(axis=1)
    assert top[8] == 42840 and bottom[8] == -10200
    hmax, hmin, vmax, vmin = ({} for _ in range(4))
    fed_by_clip = set()
    for lane in M.mc_lanes(case):
        pk, sx, sy = min(int(lane["plane"]), 1), int(lane["sx"]), int(lane["sy"])
        hs, mid, vs = M.mc_tile_sums(case, lane)
        if hs is not None:
            hmax[(pk, sx)], hmin[(pk, sx)] = max(hmax.get((pk, sx), 0), int(hs.max())), min(hmin.get((pk, sx), 0), int(hs.min()))
        if vs is not None:
            vmax[(pk, sy)], vmin[(pk, sy)] = max(vmax.get((pk, sy), 0), int(vs.max())), min(vmin.get((pk, sy), 0), int(vs.min()))
            if hs is not None:
                r = (hs + 64) >> 7
                for (i, j) in np.argwhere((vs == top[sy]) | (vs == bottom[sy])):
                    if (r[i:i + 8, j] > 255).any() and (r[i:i + 8, j] < 0).any():
                        fed_by_clip.add((pk, "top" if vs[i, j] == top[sy] else "bottom"))
    for pk, phases in ((0, range(2, 16, 2)), (1, range(1, 16))):
        for p in phases:
            assert (hmax[(pk, p)], hmin[(pk, p)]) == (top[p], bottom[p]), ("horizontal", pk, p)
            assert (vmax[(pk, p)], vmin[(pk, p)]) == (top[p], bottom[p]), ("vertical", pk, p)
    # vertical extremes whose inputs are horizontal results that were clipped at 255 and at 0
    assert fed_by_clip == {(0, "top"), (0, "bottom"), (1, "top"), (1, "bottom")}


def test_flat_case_restores_the_flat_value_under_every_phase_pair():
    cen = _census("flat")
    assert {(k[SX], k[SY]) for k in cen if k[PLANE] == 1} == {(x, y) for x in range(16) for y in range(16)}
    assert {(k[SX], k[SY]) for k in cen if k[PLANE] == 0} == {(x, y) for x in range(0, 16, 2) for y in range(0, 16, 2)}
    assert {k[COMPOUND] for k in cen} == {False, True}
    cases = T.make_mc_edge_case("flat")
    assert [c["flat"] for c in cases] == [0, 255, 127, 128]
    for case in cases:
        for a in T.oracle_mc_frame(case):
            assert (a == case["flat"]).all()


def test_clamps_case_decides_every_size_at_every_side():
    cases = T.make_mc_edge_case("clamps")
    assert {(c["width"], c["height"]) for c in cases} == {(128, 128), (64, 192)} and {c["use_subpel"] for c in cases} == {0, 1}
    decided, at_bound, one_inside = (collections.Counter() for _ in range(3))
    for case in cases:
        a = M.mc_lanes(case)
        pk = np.minimum(a["plane"], 1)
        for side, comp, sign, bound in (("L", "col", -1, "lo_col"), ("R", "col", 1, "hi_col"), ("T", "row", -1, "lo_row"), ("B", "row", 1, "hi_row")):
            step = np.where(pk == 0, 2, 1)      # one MV step (1/8 luma sample) in 1/16 sample of the plane
            for cnt, m in ((decided, a["clamp_" + comp] == sign), (at_bound, (a["clamp_" + comp] == 0) & (a["mv_" + comp] == a[bound])),
                           (one_inside, a["mv_" + comp] == a[bound] - sign * step)):
                for key in zip(a["bw8"][m].tolist(), a["bh8"][m].tolist(), pk[m].tolist(), a["compound"][m].tolist(), a["k"][m].tolist()):
                    cnt[(side, case["use_subpel"]) + key[:3]] += 1
                    cnt[(side, "compound" if key[3] else "single", key[4])] += 1
    for (bw8, bh8) in T.MC_BLOCK_SIZES:
        for side in "LRTB":
            for sub in (0, 1):
                for pk in (0, 1):
                    for cnt in (decided, at_bound, one_inside):
                        assert cnt[(side, sub, bw8, bh8, pk)] > 0, (side, sub, bw8, bh8, pk)
    for side in "LRTB":
        for kind in (("single", 0), ("compound", 0), ("compound", 1)):
            assert decided[(side,) + kind] > 0
        assert at_bound[(side, "single", 0)] > 0 and one_inside[(side, "single", 0)] > 0
    # corners: both components decided by the clamp in one block, for every size
    corners = {(k[SIDE]) for k in _census("clamps")}
    assert corners >= {"TL", "TR", "BL", "BR"}
    raw = np.concatenate([np.concatenate([c["mi"]["mv_row"].ravel(), c["mi"]["mv_col"].ravel()]) for c in cases])
    assert raw.min() == -32768 and raw.max() == 32767


def test_thin_case_clamps_in_all_four_directions():
    cases = T.make_mc_edge_case("thin")
    sides = collections.defaultdict(set)
    for case in cases:
        a = M.mc_lanes(case)
        assert a["clamp_col"].all() and a["clamp_row"].all()       # every MV is far outside
        sides[(case["width"], case["height"])] |= set(zip(a["clamp_col"].tolist(), a["clamp_row"].tolist()))
    assert set(sides) == {(8, 8), (8, 64), (64, 8), (16, 16)}
    for dims, s in sides.items():
        assert s == {(-1, -1), (1, 1), (-1, 1), (1, -1)}, dims

"""CPU: motion estimation at the ceilings of the kernels' packed arithmetic (tests/me_ceiling.py).

Census: the pictures prove, from numpy and the oracle alone, that they reach the values they are for -- N * N * 255 in a PU of every size class,
a ceiling position and a position below half of it inside one search area, both extremes of the half-pel filter, the HME block sums.
Parity: the host emulation of the kernel (tests/emu) equals the oracle run one call per SB (svt_testlib.oracle_me_picture_per_sb: the product's
model, no state crosses an SB), and the oracle equals the reference's own motion_estimate_sb where oracle/_ref is built."""
import numpy as np
import pytest

import me_ceiling as K
import me_configs as MC
import svt_testlib as T

LISTS_LAYERS = ((1, 0), (2, 1), (2, 3))
PARAM_SETS = tuple(MC.PRESETS) + ("c5", "full_sad_all_pus")
needs_ref = pytest.mark.skipif(not T.have_ref("ref_me_sb"), reason="oracle/_ref/ref_me_sb not built (reference absent)")


def params(name, nl, tl):
    if name == "c5":
        return MC.preset_c5(nl, tl)
    if name == "c5_sad":             # C5 with the sub-sampled-SAD fractional search: the form the reference built from C can run
        p = MC.preset_c5(nl, tl)
        p.fractional_search_method = 0
        return p
    if name == "full_sad_all_pus":
        return MC.variant_full_sad_all_pus(nl, tl)
    return MC.preset(name, nl, tl)


def size_for(name):
    return K.SIZES[1] if name == "c3_2160p_m8" else K.SIZES[0]


def pics_of(kind, size, seed=7):
    return [T.PaPic(f) for f in K.content(kind, size[0], size[1], seed)]


def report(a, b, nl):
    """names of the fields that differ, with the first few places: a failing case says where"""
    bad = T.me_results_equal(a, b, nl)
    if not bad:
        return None
    idx = np.argwhere(a[bad[0]] != b[bad[0]])
    return bad, len(idx), [(int(sb), int(pu), a[sb, pu].tolist()[:11], b[sb, pu].tolist()[:11]) for sb, pu in idx[:4]]


# ---- census -------------------------------------------------------------------------------------------------------------------------------------
def _class(dist, n):
    """dist0 of the PUs of size class n: [n_sb][PUs]"""
    return dist[:, {64: slice(0, 1), 32: slice(1, 5), 16: slice(5, 21), 8: slice(21, 85)}[n]]


def test_generator_is_deterministic_and_binary():
    for kind in K.KINDS:
        for w, h in K.SIZES + (K.SIZE_FAST,):
            a, b = K.content(kind, w, h, 7), K.content(kind, w, h, 7)
            assert len(a) == 3 and all(f.shape == (h, w) and f.dtype == np.uint8 and f.flags.c_contiguous for f in a)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), kind
            vals = set(np.unique(np.stack(a)).tolist())
            assert vals <= ({0, 254, 255} if kind == "dented" else {0, 255}) and {0, 255} <= vals, (kind, vals)
    assert not np.array_equal(K.content("blocks", 200, 136, 1)[1], K.content("blocks", 200, 136, 2)[1])


@pytest.mark.parametrize("name", tuple(MC.PRESETS) + ("c5",))
def test_census_all_tie_kinds_report_the_ceiling_of_every_size_class(name):
    """black_white: every PU of every size class wins with dist0 == N * N * 255 (the scale of the full-pel search: rows 0, 2, 4, .. doubled,
    oracle/oracle_me.c fullpel_position) -- the 64x64 one with the search's own initial value MAX_SAD_VALUE.  dented: the 64x64 PU of every SB
    lies below that value, by at most 510, so that its vector is defined; three of the four 32x32 PUs and 15 of the 16 16x16 PUs stay at the
    ceiling."""
    size = size_for(name)
    p = params(name, 1, 0)
    pics = pics_of("black_white", size)
    o, _ = T.oracle_me_picture_per_sb(pics[1], pics[0], None, p)
    for n in (8, 16, 32, 64):
        assert (_class(o["dist0"], n) == K.CEIL[n]).all(), (name, n)
    assert (o["x_mv_l0"][:, 0] == 0).all() and (o["y_mv_l0"][:, 0] == 0).all()      # nothing beat the initial value: a fresh context's vector
    pics = pics_of("dented", size)
    o, _ = T.oracle_me_picture_per_sb(pics[1], pics[0], None, p)
    d64 = _class(o["dist0"], 64)[:, 0].astype(np.int64)
    assert (d64 < K.CEIL[64]).all() and (d64 >= K.CEIL[64] - 510).all(), d64
    assert ((_class(o["dist0"], 32) == K.CEIL[32]).sum(1) == 3).all() and ((_class(o["dist0"], 16) == K.CEIL[16]).sum(1) == 15).all()
    assert ((_class(o["dist0"], 8) == K.CEIL[8]).sum(1) == 63).all()


def test_census_one_match_far_sbs_sit_at_max_sad_value():
    pics = pics_of("one_match", K.SIZES[0])
    o, _ = T.oracle_me_picture_per_sb(pics[1], pics[0], None, params("c1_360p_m9", 1, 0))
    assert (o["dist0"][8:12, 0] == K.CEIL[64]).all() and (o["dist0"][:8, 0] < K.CEIL[64]).all()
    for n in (8, 16, 32):
        assert (_class(o["dist0"], n) == K.CEIL[n]).any() and (_class(o["dist0"], n) == 0).any(), n


def subsampled_sads(cur, ref, n, area):
    """row-subsampled SAD (rows 0, 2, .. of the PU, doubled) of every n x n PU of the picture's whole SBs rows / columns against the reference
    displaced by every (dx, dy) of `area` = (x0, y0, w, h): [positions][PU rows][PU columns], plain numpy on the edge-padded reference"""
    h, w = cur.shape
    pad = 16
    rp = np.pad(ref, pad, mode="edge").astype(np.int32)
    c = cur.astype(np.int32)
    x0, y0, aw, ah = area
    out = []
    for dy in range(y0, y0 + ah):
        for dx in range(x0, x0 + aw):
            d = np.abs(c - rp[pad + dy:pad + dy + h, pad + dx:pad + dx + w])[0::2]
            d = d[:(h // n) * (n // 2), :(w // n) * n]
            out.append(2 * d.reshape(h // n, n // 2, w // n, n).sum((1, 3)))
    return np.stack(out)


def smallest_search_area():
    """the positions every preset searches around a centre: the intersection of the presets' search areas, placed as the search places them"""
    ps = [params(n, 1, 0) for n in PARAM_SETS]
    w, h = min(p.search_area_width for p in ps), min(p.search_area_height for p in ps)
    return (-(w >> 1), -(h >> 1), w, h)


LOW = {16: 32768, 8: 8192}      # half the 16-bit field a 16x16 sum lives in, and the same share of an 8x8 sum's
COMPETE = {"pixel_checker": (16,), "row_stripes": (16,), "taps": (16,), "blocks": (16, 8), "one_match": (8,), "hme": (8,)}


@pytest.mark.parametrize("kind", [k for k in K.KINDS if k not in K.ALL_TIE])
def test_census_ceiling_positions_compete_with_low_positions(kind):
    """Every kind but the all-tie ones holds a PU with one full-pel position at the ceiling of its class (16x16: 65 280, 8x8: 16 320) and another
    below half the field (32 768 / 8 192) inside one search area: a carry between packed sums must be able to change who wins.  A carry that
    hits every position alike (black_white) leaves the argmin where it was.  Checked within the c1 preset's area (16 x 7) around the zero
    vector of list 0, and for the 16x16 classes of the periodic kinds within the area common to all presets as well."""
    ref0, cur, _ = K.content(kind, *K.SIZES[0], 7)
    p = params("c1_360p_m9", 1, 0)
    areas = [(-(p.search_area_width >> 1), -(p.search_area_height >> 1), p.search_area_width, p.search_area_height)]
    if kind in ("pixel_checker", "row_stripes", "taps"):
        areas.append(smallest_search_area())
    for area in areas:
        for n in COMPETE[kind]:
            s = subsampled_sads(cur, ref0, n, area)
            both = (s.max(0) == K.CEIL[n]) & (s.min(0) < LOW[n])
            assert s.max() == K.CEIL[n] and both.any(), (kind, n, area, int(s.max()), int(s.min()))


def test_census_all_tie_kinds_do_not_compete():
    """the reason the other kinds exist: in black_white all positions of a PU carry the same sum"""
    ref0, cur, _ = K.content("black_white", *K.SIZES[0], 7)
    s = subsampled_sads(cur, ref0, 16, smallest_search_area())
    assert (s == K.CEIL[16]).all()


def test_census_taps_hold_both_extremes_of_the_half_pel_filter():
    """(-2, 18, 18, -2) over (255, 0, 0, 255) is -1020 (+ 16, >> 5: clipped to 0), over (0, 255, 255, 0) it is 9180 (clipped to 255): the packed
    signed 16-bit filter's smallest and largest sums.  The windows lie along rows and along columns inside SB 0's search area, and the J plane
    (the filter over the filtered rows) meets them too where the tiles of vertical stripes are filtered vertically."""
    ref0 = K.content("taps", *K.SIZES[0], 7)[0].astype(np.int32)
    reg = ref0[0:64 + 8, 0:64 + 8]
    lo, hi = np.array([255, 0, 0, 255]), np.array([0, 255, 255, 0])
    rows = np.lib.stride_tricks.sliding_window_view(reg, 4, axis=1)
    cols = np.lib.stride_tricks.sliding_window_view(reg, 4, axis=0)
    for win in (rows, cols):
        assert (win == lo).all(-1).any() and (win == hi).all(-1).any()
    taps = np.array([-2, 18, 18, -2])
    b = (rows * taps).sum(-1)
    assert b.min() == -1020 and b.max() == 9180
    bc = np.clip((b + 16) >> 5, 0, 255)
    j = (np.lib.stride_tricks.sliding_window_view(bc, 4, axis=0) * taps).sum(-1)
    assert j.min() == -1020 and j.max() == 9180


def test_census_hme_planes_are_binary_and_reach_the_level_ceilings():
    """1/16 plane: a 16x8 block pair (the SB's 16 x 16 samples, every other row) with SAD 32 640 beside a position below half of it inside
    +-8 / +-4 of the SB, which every preset's level-0 area contains; 1/4 and full planes: 32x16 and 64x32 sums of 130 560 and 522 240."""
    w, h = K.SIZES[0]
    ref0, cur, _ = K.content("hme", w, h, 7)
    for p in (params(n, 1, 0) for n in PARAM_SETS):
        assert p.hme_level0_total_search_area_width >= 16 and p.hme_level0_total_search_area_height >= 8
    c16, r16 = cur[::4, ::4].astype(np.int32), np.pad(ref0[::4, ::4], 16, mode="edge").astype(np.int32)
    assert set(np.unique(c16)) == {0, 255} and set(np.unique(cur[::2, ::2])) == {0, 255}
    found = False
    for sy in range(h // 64):
        for sx in range(w // 64):
            blk = c16[sy * 16:sy * 16 + 16:2, sx * 16:sx * 16 + 16]
            s = np.array([np.abs(blk - r16[16 + sy * 16 + dy:16 + sy * 16 + dy + 16:2, 16 + sx * 16 + dx:16 + sx * 16 + dx + 16]).sum()
                          for dy in range(-4, 4) for dx in range(-8, 8)])
            found |= bool(s.max() == 16 * 8 * 255 and s.min() < 16384)
    assert found
    # the tiles where the current picture is 255 over references of 0: every level at its ceiling at the zero vector
    flat = [(sx, sy) for sy in range(h // 64) for sx in range(w // 64) if (cur[sy * 64:sy * 64 + 64, sx * 64:sx * 64 + 64] == 255).all()
            and (ref0[sy * 64:sy * 64 + 64, sx * 64:sx * 64 + 64] == 0).all()]
    assert flat
    sx, sy = flat[0]
    d = np.abs(cur.astype(np.int32) - ref0)[sy * 64:sy * 64 + 64, sx * 64:sx * 64 + 64]
    assert d[::4, ::4][::2].sum() == 32640 and d[::2, ::2][::2].sum() == 130560 and d[::2].sum() == 522240


@pytest.mark.parametrize("kind", ["taps", "pixel_checker", "blocks"])
@pytest.mark.parametrize("name", ["c5", "full_sad_all_pus"])
def test_census_fractional_vectors_and_three_candidates(kind, name):
    pics = pics_of(kind, K.SIZES[0])
    o, _ = T.oracle_me_picture_per_sb(pics[1], pics[0], pics[2], params(name, 2, 1))
    x, y = o["x_mv_l0"], o["y_mv_l0"]
    assert (((x & 3) == 2) | ((y & 3) == 2)).any(), "no half-pel vector"
    assert (((x & 1) == 1) | ((y & 1) == 1)).any(), "no quarter-pel vector"
    assert (o["total"] == 3).any()


def test_census_sad_loop_jobs_sit_at_the_ceiling():
    """the stand-alone SAD search's ceiling jobs: 16x8 / 32x16 / 64x32 sums of 32 640 / 130 560 / 522 240 at every position (the first one wins),
    or everywhere but at a planted exact match, the last position in raster order"""
    case, want = T.make_sad_loop_ceiling_case()
    assert sorted(set(want[:, 0].tolist())) == [0, 32640, 130560, 522240]
    assert np.array_equal(T.oracle_sad_loop_case(case), want)
    if T.have_ref("libsvtref_kernels.so"):
        assert np.array_equal(T.ref_sad_loop_case(case), want)


# ---- what "equal" means where the reference is order-dependent -----------------------------------------------------------------------------------
def _diff_places(a, b):
    return {f: {(int(s), int(u)) for s, u in np.argwhere(a[f] != b[f])} for f in a.dtype.names if f != "pad" and (a[f] != b[f]).any()}


@pytest.mark.parametrize("name", tuple(MC.PRESETS) + ("c5_sad",))
@pytest.mark.parametrize("nl,tl", LISTS_LAYERS)
def test_whole_picture_and_per_sb_oracle_differ_only_at_max_sad(name, nl, tl):
    """one_match 200x136: list 0 of the far SBs (8..11: the bottom SB row, 8 rows high) finds no position below 64 * 64 * 255, the search's
    initial best SAD, in the 64x64 PU.  A whole-picture run returns the vector its context held from the SB before, a run per SB (and the
    kernel) the zero vector; nothing else differs but, with two lists, the distortion of PU 0's bi-prediction, which is built from that vector.
    With the c1 preset all four SBs are affected."""
    pics = pics_of("one_match", K.SIZES[0])
    p = params(name, nl, tl)
    r1 = pics[2] if nl == 2 else None
    whole, _ = T.oracle_me_picture(pics[1], pics[0], r1, p)
    per_sb, _ = T.oracle_me_picture_per_sb(pics[1], pics[0], r1, p)
    d = _diff_places(whole, per_sb)
    far = {(sb, 0) for sb in range(8, 12)}
    assert d and set(d) <= {"x_mv_l0", "y_mv_l0", "dist1", "dist2"} and "x_mv_l0" in d, d
    assert all(v <= far for v in d.values()), d
    if name == "c1_360p_m9":
        assert d["x_mv_l0"] | d["y_mv_l0"] == far
    if nl == 1:
        assert set(d) <= {"x_mv_l0", "y_mv_l0"}
    for sb, pu in set().union(*d.values()):
        r = per_sb[sb, pu]
        l0 = [int(r["dist%d" % i]) for i in range(int(r["total"])) if int(r["dir%d" % i]) == 0]
        assert l0 == [K.CEIL[64]] and r["x_mv_l0"] == 0 and r["y_mv_l0"] == 0, (sb, r)
        assert whole[sb, pu]["dist0"] == r["dist0"] and whole[sb, pu]["dir0"] == r["dir0"]
    if T.have_ref("ref_me_sb"):
        ref, _ = T.ref_me_picture(pics[1], pics[0], r1, p)
        assert not T.me_results_equal(ref, whole, nl)


@needs_ref
@pytest.mark.parametrize("nl,tl", LISTS_LAYERS)
def test_reference_per_sb_equals_per_sb_oracle_at_max_sad(nl, tl):
    """the reference's own motion_estimate_sb started on each SB alone (a fresh context per SB) returns what the per-SB oracle returns"""
    pics = pics_of("one_match", K.SIZES[0])
    p = params("c1_360p_m9", nl, tl)
    r1 = pics[2] if nl == 2 else None
    per_sb, _ = T.oracle_me_picture_per_sb(pics[1], pics[0], r1, p)
    for sb in range(T.n_sb(*K.SIZES[0])):
        ref, _ = T.ref_me_picture(pics[1], pics[0], r1, p, sb, sb + 1)
        assert not T.me_results_equal(ref[sb:sb + 1], per_sb[sb:sb + 1], nl), sb


# ---- parity ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl,tl", LISTS_LAYERS)
@pytest.mark.parametrize("name", PARAM_SETS)
@pytest.mark.parametrize("kind", K.KINDS)
def test_kernel_emulation_vs_per_sb_oracle_at_the_ceiling(kind, name, nl, tl):
    pics = pics_of(kind, size_for(name))
    p = params(name, nl, tl)
    r1 = pics[2] if nl == 2 else None
    o, orc = T.oracle_me_picture_per_sb(pics[1], pics[0], r1, p)
    e, erc = T.emu_me_picture(pics[1], pics[0], r1, p)
    assert report(o, e, nl) is None, report(o, e, nl)
    assert np.array_equal(orc, erc)


# one_match with the 64x64 refinement on (fractional_search64x64, only the full_sad_all_pus variant has it) is left out of the whole-picture
# runs: the reference refines the stale vector of the SB before, which points outside its search region, and its driver dies reading there
REF_CASES = [(k, n) for k in K.KINDS for n in tuple(MC.PRESETS) + ("c5_sad", "full_sad_all_pus") if (k, n) != ("one_match", "full_sad_all_pus")]


@needs_ref
@pytest.mark.parametrize("nl,tl", LISTS_LAYERS)
@pytest.mark.parametrize("kind,name", REF_CASES)
def test_oracle_vs_reference_me_at_the_ceiling(kind, name, nl, tl):
    """the oracle against the reference's own motion_estimate_sb, both over the whole picture in SB order (the reference's context carries over,
    and so does the oracle's in that mode: equal also where the 64x64 vector is order-dependent); rate-control SADs included"""
    pics = pics_of(kind, size_for(name))
    p = params(name, nl, tl)
    r1 = pics[2] if nl == 2 else None
    r, rrc = T.ref_me_picture(pics[1], pics[0], r1, p)
    o, orc = T.oracle_me_picture(pics[1], pics[0], r1, p)
    assert report(r, o, nl) is None, report(r, o, nl)
    if p.rate_control_mode:
        assert np.array_equal(rrc, orc)

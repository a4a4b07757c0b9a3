"""CPU: the mode-info syntax of inter pictures (csrc/modeinfo_inter_core.h through the host form svt_hip_modes_inter_picture) against the
reference's own tile bytes (tests/golden/modes_inter_reference.npz, written by tests/gen_golden_modes_inter.py) and, record for record,
against a serial Python model that carries the context arrays and block pointers a serial coder carries (tests/modes_inter_model.py).
Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import boolcode_model as BM
import modes_inter_model as IM
import modes_model as MM
import svt_testlib as T

B = T.B
NAMES = IM.NAMES


def test_abi_symbols_and_struct_sizes():
    lib = B.load()
    for s in ("svt_hip_modes_inter_set_tables", "svt_hip_modes_inter_batch_device", "svt_hip_modes_inter_picture", "svt_hip_modes_inter_bools_capacity"):
        assert hasattr(lib, s) and s in B.EXPORTS, s
    assert B.MODES_INTER_TABLES_DTYPE.itemsize == 291 and B.MI_INTER_EXT_DTYPE.itemsize == 12 and C.sizeof(B.ModesInterPicture) == 88
    # 3 x SPLIT + NONE, skip, is_inter, compound flag + reference, 3 mode bools, two MVs of 3 + 2 x (1 + 7 + 10 + 3 + 1)
    assert B.MODES_INTER_UNIT_BOOLS == 3 * 3 + 1 + 2 + 2 + 3 + 2 * (3 + 2 * 22) == 111
    assert lib.svt_hip_modes_inter_bools_capacity(72, 40) == 45 * B.MODES_INTER_UNIT_BOOLS
    assert lib.svt_hip_modes_inter_bools_capacity(70, 64) == 0 and lib.svt_hip_modes_inter_bools_capacity(0, 64) == 0


def test_fixture_holds_what_the_tests_need():
    g, tabs = IM.fixture(), IM.tables()[0]
    assert [str(n) for n in g["names"]] == NAMES and np.all(g["seconds"] > 0)
    for n, shape in IM.TABLE_SHAPES:
        assert tabs[n].shape == shape and tabs[n].min() >= 1, n
    cov = {}
    for name, W, H, kind, seed, fr, p_intra in IM.PICTURES:
        p, made = IM.fixture_picture(name), IM.make_picture(W, H, kind, seed, fr, p_intra)
        assert (p["W"], p["H"]) == (W, H) and p["frame"] == fr
        for k in ("lf_mi", "mc_mi", "ext", "qcoeff", "eob_map"):
            assert np.array_equal(p[k], made[k]), (name, k)
        IM.serial_walk(p, tabs, cov)
        assert len(p["tile"]) > len(p["modes"]) > 0
    # together the pictures reach every context and symbol: the model's notes, and the reference's own, which the generator stored
    assert not IM.coverage_complete(cov)
    ref_cov = {k: {b + (10 if k == "mode" else 0) for b in range(32) if (int(w) >> b) & 1} for k, w in zip(IM.COVER_KEYS, g["coverage"])}
    assert not IM.coverage_complete(ref_cov) and ref_cov == cov
    kinds = {(int(p["frame"]["reference_mode"]), int(p["frame"]["allow_hp"])) for p in map(IM.fixture_picture, NAMES)}
    assert kinds == {(IM.SINGLE, 0), (IM.SELECT, 0), (IM.SELECT, 1)}
    mix = IM.fixture_picture("mix_136x136_select")
    assert (mix["lf_mi"]["sb_type"] == 0).any() and (mix["lf_mi"]["is_inter"] == 0).any() and (mix["ext"]["ref_frame"][..., 1] > 0).any()
    assert {int(v) for v in np.unique(IM.fixture_picture("mix_136x136_single")["ext"]["ref_frame"][..., 0])} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", NAMES)
def test_host_chain_equals_the_reference_tile(name):
    """host tokeniser -> host mode-info stage -> host bool coder over its segments = the reference's tile; its bools alone = the
    reference's mode-info bytes"""
    p = IM.fixture_picture(name)
    tile, only, m = IM.host_chain(name)
    assert only == p["modes"]
    assert tile == p["tile"]
    assert np.all(m["guard"] == 0xA5A5) and np.all(m["seg_guard"] == 0x5A5A5A5A)


def check_against_model(p, tok, m):
    W, H = p["W"], p["H"]
    recs, leaves = IM.serial_walk(p, IM.tables()[0])
    assert m["rc"] == 0 and m["n_bools"] == len(recs) <= B.load().svt_hip_modes_inter_bools_capacity(W, H) and np.array_equal(m["bools"], recs)
    assert np.all(m["guard"] == 0xA5A5) and np.all(m["seg_guard"] == 0x5A5A5A5A)
    # the list without its empty slots is the serial walk's: per leaf its bools, then its Y, Cb, Cr runs from the tokeniser's offsets
    runs = MM.leaf_runs(p["lf_mi"], tok["tok_off"], p["eob_map"], W, H)
    order = MM.coding_order_segments(leaves, runs)
    seg = m["segments"]
    assert len(seg) == T.n_sb(W, H) * 256
    assert [s for s in zip(seg["first"].tolist(), seg["count"].tolist(), seg["kind"].tolist()) if s[1]] == order
    empty = seg[seg["count"] == 0]
    assert not empty["first"].any() and not empty["kind"].any()
    return recs, order


@pytest.mark.parametrize("name", NAMES)
def test_host_records_equal_the_serial_model(name):
    p, tok = IM.fixture_picture(name), IM.host_tokens(name)
    recs, order = check_against_model(p, tok, IM.host_of(name))
    # the model's own bytes, through the model of the bool coder
    assert BM.serial_write(BM.expand(tok["tokens"], recs, order, BM.tables()[0])) == p["tile"]


@pytest.mark.parametrize("name", [b[0] for b in IM.BIG])
def test_big_picture_host_form_equals_the_serial_model(name):
    """1080x1080: 289 SBs, partial on both edges"""
    p, h = next(p for p in IM.big_pictures() if p["name"] == name), IM.big_host(name)
    assert T.n_sb(p["W"], p["H"]) == 289
    check_against_model(p, h["tok"], h["modes"])


def test_capacity_exact_one_short_and_zero():
    name = "mix_136x136_select"
    p, tok, full = IM.fixture_picture(name), IM.host_tokens(name), IM.host_of(name)
    exact = IM.host_modes(p, tok["tok_off"], capacity=full["n_bools"])
    assert exact["rc"] == 0 and np.array_equal(exact["bools"], full["bools"]) and np.all(exact["guard"] == 0xA5A5) and len(exact["guard"]) == 64
    short = IM.host_modes(p, tok["tok_off"], capacity=full["n_bools"] - 1)
    assert short["rc"] == 0 and short["n_bools"] == full["n_bools"] and np.array_equal(short["bools"], full["bools"][:-1])
    assert np.all(short["guard"] == 0xA5A5) and len(short["guard"]) == 64 and np.array_equal(short["segments"], full["segments"])
    none = IM.host_modes(p, tok["tok_off"], capacity=0)
    assert none["rc"] == 0 and none["n_bools"] == full["n_bools"] and np.all(none["guard"] == 0xA5A5) and np.array_equal(none["segments"], full["segments"])


def worst_unit_picture():
    """a 64x64 picture of 8x8 compound NEWMV leaves under REFERENCE_MODE_SELECT with high-precision MVs: both differences of every leaf
    have two components of class 10 (10 integer bits) with a three-bool fraction, against reference MVs below the threshold.  Every leaf
    is skipped: no tokens"""
    fr = IM.frame(allow_hp=1, **IM.B_PICTURE)
    p = IM.make_picture(64, 64, 3, 7, fr, 0.0)
    p["lf_mi"]["skip"] = 1
    p["qcoeff"][:], p["eob_map"][:] = 0, 0
    p["ext"]["ref_frame"], p["ext"]["mode"] = (IM.LAST, IM.ALTREF), IM.NEWMV
    p["mc_mi"]["ref_list"] = (0, 1)
    p["ext"]["ref_mv_row"], p["ext"]["ref_mv_col"] = (-63, 5), (63, 0)
    p["mc_mi"]["mv_row"], p["mc_mi"]["mv_col"] = (-63 + 16383, 5 - 16383), (63 - 16383, 16383)
    return p


def test_bound_is_reached_by_the_worst_unit():
    p = worst_unit_picture()
    tok_off = np.full(p["eob_map"].size, 0xFFFFFFFF, np.uint32)
    m = IM.host_modes(p, tok_off)
    assert m["rc"] == 0
    counts = m["segments"]["count"][m["segments"]["kind"] == 1]
    assert counts[0] == counts.max() == B.MODES_INTER_UNIT_BOOLS == 111          # only the SB's origin has all four partition symbols
    assert sorted(set(counts.tolist())) == [102, 105, 108, 111]                  # the leaf's 101 + NONE, and + 1, 2, 3 SPLITs above it
    recs, _ = IM.serial_walk(p, IM.tables()[0])
    assert np.array_equal(m["bools"], recs)


def malformed_pictures():
    """(what is wrong, picture, frame override or None): a 64x64 picture of 16x16 (or 8x8) inter leaves under REFERENCE_MODE_SELECT with
    one record changed; the last entries are well formed (answer: not SVT_MODES_BAD_GRID)"""
    fr = IM.frame(**IM.B_PICTURE)
    base16, base8 = IM.make_picture(64, 64, 6, 5, fr, 0.0), IM.make_picture(64, 64, 3, 6, fr, 0.0)
    out = []

    def copy(base):
        p = dict(base)
        for k in ("lf_mi", "mc_mi", "ext"):
            p[k] = base[k].copy()
        return p

    def case(what, base=base16, area=None, lf=None, mc=None, ext=None, frame=None, good=False):
        p = copy(base)
        for grid, changes in (("lf_mi", lf), ("mc_mi", mc), ("ext", ext)):
            for field, value in (changes or {}).items():
                p[grid][area][field] = value
        out.append((what, p, frame, good))

    def block_with(base, pred):
        """origin (r, c) of the first leaf whose extension record satisfies pred, as an area of the leaf's units"""
        n = IM.UNITS[int(base["lf_mi"][0, 0]["sb_type"])]
        for r in range(0, 8, n):
            for c in range(0, 8, n):
                if pred(base["ext"][r, c], base["mc_mi"][r, c]):
                    return (slice(r, r + n), slice(c, c + n))
        raise AssertionError("no such leaf")
    single = block_with(base16, lambda e, m: e["ref_frame"][1] == 0)
    comp = block_with(base16, lambda e, m: e["ref_frame"][1] > 0)
    newmv = block_with(base16, lambda e, m: e["mode"] == IM.NEWMV)
    one = (slice(2, 3), slice(2, 3))
    # what the key-frame check rejects
    case("rectangular sb_type", area=one, lf=dict(sb_type=7))
    case("sb_type above 12", area=(slice(0, 1), slice(0, 1)), lf=dict(sb_type=13))
    case("tx_size smaller than the block", area=(slice(0, 1), slice(2, 3)), lf=dict(tx_size=1))
    case("tx_size larger than the block", area=(slice(6, 7), slice(0, 1)), lf=dict(tx_size=3))
    p = copy(base16)
    p["lf_mi"][:4, :4]["sb_type"], p["lf_mi"][:4, :4]["tx_size"] = 9, 3
    p["lf_mi"][1, 1]["sb_type"], p["lf_mi"][1, 1]["tx_size"] = 3, 1
    out.append(("a block inside another", p, None, False))
    intra = dict(lf=dict(is_inter=0), mc=dict(ref_list=(-1, -1)), ext=dict(ref_frame=(0, 0)))
    case("an intra block (well formed)", area=single, lf=dict(is_inter=0, pad=(0, 9, 9)), mc=intra["mc"], ext=intra["ext"], good=True)
    case("an intra block whose ref_list[1] is not -1 (well formed: ref_list[0] < 0 says it all)", area=single, lf=dict(is_inter=0, pad=(0, 3, 4)), mc=dict(ref_list=(-1, 0)),
         ext=intra["ext"], good=True)
    case("luma mode above 9", area=single, lf=dict(is_inter=0, pad=(0, 10, 0)), mc=intra["mc"], ext=intra["ext"])
    case("chroma mode above 9", area=single, lf=dict(is_inter=0, pad=(0, 0, 12)), mc=intra["mc"], ext=intra["ext"])
    case("four 4x4 intra blocks (well formed)", base=base8, area=one, lf=dict(is_inter=0, sb_type=0, tx_size=0, pad=(0x98, 0x12, 3)), mc=intra["mc"], ext=intra["ext"], good=True)
    case("4x4 mode above 9", base=base8, area=one, lf=dict(is_inter=0, sb_type=0, tx_size=0, pad=(0xA3, 0x12, 3)), mc=intra["mc"], ext=intra["ext"])
    # what only inter pictures can get wrong
    case("an inter block below 8x8", base=base8, area=one, lf=dict(sb_type=0, tx_size=0))
    case("is_inter = 0 over an inter record", area=single, lf=dict(is_inter=0))
    case("is_inter = 1 over ref_frame[0] = 0", area=single, ext=dict(ref_frame=(0, 0)))
    case("ref_list[0] < 0 in an inter block", area=single, mc=dict(ref_list=(-1, -1)))
    case("ref_list[1] >= 0 in a single-reference block", area=single, mc=dict(ref_list=(0, 1)))
    case("ref_list[1] < 0 in a compound block", area=comp, mc=dict(ref_list=(0, -1)))
    case("ref_frame[1] > 0 in an intra block", area=single, lf=dict(is_inter=0), mc=dict(ref_list=(-1, 1)), ext=dict(ref_frame=(0, 3)))
    case("ref_frame above 3", area=single, ext=dict(ref_frame=(4, 0)))
    case("a compound block under SINGLE_REFERENCE", frame=IM.frame(IM.SINGLE, 0, (0, 0, 0, 1)))
    case("a compound block without comp_fixed_ref", area=comp, ext=dict(ref_frame=(1, 2)))
    case("a compound block whose variable reference is the fixed one", area=comp, ext=dict(ref_frame=(3, 3)))
    case("a compound block with its references the other way round", area=comp, ext=dict(ref_frame=(3, 1)))
    p = copy(base16)
    p["ext"]["ref_frame"][..., 1] = 0
    p["mc_mi"]["ref_list"][..., 1] = -1
    out.append(("single references alone under REFERENCE_MODE_SELECT (well formed)", p, None, True))
    out.append(("a single-reference block under COMPOUND_REFERENCE", p, IM.frame(IM.COMPOUND, 0, (0, 0, 0, 1)), False))
    case("inter mode 9", area=(slice(0, 1), slice(0, 1)), ext=dict(mode=9))
    case("inter mode 14", area=(slice(4, 5), slice(4, 5)), ext=dict(mode=14))
    case("mode_context 7", area=(slice(2, 3), slice(6, 7)), ext=dict(mode_context=7))
    case("mode 14 off a leaf's origin (well formed: read at the origin only)", area=(slice(1, 2), slice(1, 2)), ext=dict(mode=14, mode_context=9), good=True)
    r0, c0 = newmv[0].start, newmv[1].start
    origin = (slice(r0, r0 + 1), slice(c0, c0 + 1))
    case("MV row difference 16384", area=origin, mc=dict(mv_row=(16384, 0), mv_col=(0, 0)), ext=dict(ref_mv_row=(0, 0), ref_mv_col=(0, 0), mode=IM.NEWMV))
    case("MV column difference -16384", area=origin, mc=dict(mv_row=(0, 0), mv_col=(-16000, 0)), ext=dict(ref_mv_row=(0, 0), ref_mv_col=(384, 0), mode=IM.NEWMV))
    case("MV differences +-16383 (well formed)", area=origin, mc=dict(mv_row=(16383, 0), mv_col=(-16000, 0)),
         ext=dict(ref_mv_row=(0, 0), ref_mv_col=(383, 0), mode=IM.NEWMV), good=True)
    case("MV difference 16384 of a ZEROMV block (well formed: not coded)", area=origin, mc=dict(mv_row=(16384, 0), mv_col=(0, 0)),
         ext=dict(ref_mv_row=(0, 0), ref_mv_col=(0, 0), mode=IM.ZEROMV), good=True)
    if base16["ext"][origin]["ref_frame"][0, 0, 1] > 0:
        case("second MV difference 16384 of a compound block", area=origin, mc=dict(mv_row=(0, 16384), mv_col=(0, 0)),
             ext=dict(ref_mv_row=(0, 0), ref_mv_col=(0, 0), mode=IM.NEWMV))
    return out


def edge_crossing_picture():
    """72x40: a 16x16 leaf at the unit column 8, of which only one column is inside the picture"""
    p = dict(IM.fixture_picture("edge_72x40_b"))
    lf = p["lf_mi"].copy()
    lf[0:2, 8]["sb_type"], lf[0:2, 8]["tx_size"] = 6, 2
    p["lf_mi"] = lf
    return p


MALFORMED = malformed_pictures() + [("a block crossing the picture edge", edge_crossing_picture(), None, False)]


@pytest.mark.parametrize("k", range(len(MALFORMED)))
def test_malformed_grids_answer_the_named_value(k):
    what, p, fr, good = MALFORMED[k]
    tok_off = np.full(p["eob_map"].size, 0xFFFFFFFF, np.uint32)
    p = dict(p, eob_map=np.zeros_like(p["eob_map"]))
    p["lf_mi"] = p["lf_mi"].copy()
    p["lf_mi"]["skip"] = 1                                   # no token runs: the grids alone are under test
    m = IM.host_modes(p, tok_off, frame_override=fr)
    assert m["rc"] == 0 and np.all(m["guard"] == 0xA5A5) and np.all(m["seg_guard"] == 0x5A5A5A5A), what
    if good:
        assert m["n_bools"] != B.MODES_BAD_GRID and m["segments"]["count"].any(), what
        recs, _ = IM.serial_walk(dict(p, frame=fr or p["frame"]), IM.tables()[0])
        assert np.array_equal(m["bools"], recs), what
    else:
        assert m["n_bools"] == B.MODES_BAD_GRID == 0xFFFFFFFF and not m["segments"]["count"].any(), what


def test_the_malformed_list_names_every_case():
    names = " | ".join(w for w, _, _, good in MALFORMED if not good)
    for must in ("rectangular", "inside another", "crossing the picture edge", "tx_size", "luma mode above 9", "chroma mode above 9", "4x4 mode above 9", "below 8x8",
                 "is_inter = 0", "is_inter = 1", "ref_list[0]", "ref_list[1] >= 0", "ref_list[1] < 0", "under SINGLE_REFERENCE", "without comp_fixed_ref",
                 "variable reference", "inter mode 9", "inter mode 14", "mode_context 7", "row difference 16384", "column difference -16384"):
        assert must in names, must


def test_bad_arguments():
    lib, p, tok = B.load(), IM.fixture_picture("sb64_leaf6"), IM.host_tokens("sb64_leaf6")
    assert IM.host_modes(dict(p, H=60), tok["tok_off"], capacity=100)["rc"] != 0                                      # height no multiple of 8
    assert IM.host_modes(p, tok["tok_off"], frame_override=dict(p["frame"], reference_mode=3))["rc"] != 0
    assert IM.host_modes(p, tok["tok_off"], frame_override=dict(p["frame"], comp_fixed_ref=0))["rc"] != 0
    assert IM.host_modes(p, tok["tok_off"], frame_override=dict(p["frame"], comp_var_ref=(1, 4)))["rc"] != 0
    assert lib.svt_hip_modes_inter_picture(None, None, 64, 64, 8) != 0
    t = IM.tables()[1]
    assert lib.svt_hip_modes_inter_picture(t.ctypes.data_as(C.c_void_p), C.byref(B.ModesInterPicture()), 64, 64, 8) != 0      # null fields
    # the batch entry point refuses on its arguments alone, before any use of the context
    fake_ctx = C.create_string_buffer(1 << 20)
    arr = (B.ModesInterPicture * 1)(B.ModesInterPicture())
    assert lib.svt_hip_modes_inter_batch_device(fake_ctx, 1, arr, 64, 64, 8) != 0 and lib.svt_hip_modes_inter_batch_device(fake_ctx, 33, arr, 64, 64, 8) != 0
    assert lib.svt_hip_modes_inter_batch_device(None, 1, arr, 64, 64, 8) != 0 and lib.svt_hip_modes_inter_set_tables(None, None) != 0


@pytest.mark.parametrize("name", ("edge_72x40_b", "mix_136x136_select", "big_select_hp"))
def test_host_form_on_a_wider_grid(name):
    """mi_stride = mi_cols + 9, random bytes in the records behind the picture in all three grids: every output as on the tight grids"""
    if name.startswith("big"):
        p, h = next(p for p in IM.big_pictures() if p["name"] == name), IM.big_host(name)
        tok, tight = h["tok"], h["modes"]
    else:
        p, tok, tight = IM.fixture_picture(name), IM.host_tokens(name), IM.host_of(name)
    wide = IM.with_stride(p, 9, 2)
    assert wide["lf_mi"].shape[1] == wide["ext"].shape[1] == p["W"] // 8 + 9 and wide["lf_mi"][:, p["W"] // 8:]["sb_type"].max() > 12
    got = IM.host_modes(wide, tok["tok_off"])
    assert got["rc"] == tight["rc"] == 0 and got["n_bools"] == tight["n_bools"] != B.MODES_BAD_GRID
    assert np.array_equal(got["bools"], tight["bools"]) and np.array_equal(got["segments"], tight["segments"])
    assert np.all(got["guard"] == 0xA5A5) and np.all(got["seg_guard"] == 0x5A5A5A5A)

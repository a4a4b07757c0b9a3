"""CPU: inter mode labelling (csrc/md_inter_core.h through the host form svt_hip_md_inter_modes_picture) against the Python statement
of the rule (tests/md_inter_model.py over the find_mv_refs model that tests/golden/mvrefs_reference.npz pins to the reference): the
pictures of the MV-reference and inter mode-info fixtures with ref_frame and mode erased, seeded pictures, constructed cases of the
rule's order; closure under the existing svt_hip_mvrefs_picture (no contradiction, the same records byte for byte); the decoder-side
replay against the count of unfaithful leaves; wider grids, optional outputs, ref_mask, every refusal; and the host chain tokeniser ->
labelling -> inter mode info -> bool coder against the records and tile bytes the reference gave (tests/golden/md_inter_reference.npz,
written by tests/gen_golden_md_inter.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import boolcode_model as BM
import md_inter_model as D
import modes_inter_model as IM
import mvrefs_model as M
import svt_testlib as T
import tokenize_model as TM

B = T.B
FIXTURE = D.fixture_inputs()
SELECT_ALT = IM.frame(reference_mode=IM.SELECT, sign_bias=M.ALT_BIAS)
SELECT_ALT_HP = IM.frame(reference_mode=IM.SELECT, allow_hp=1, sign_bias=M.ALT_BIAS)
# (name, arguments of md_inter_model.seeded)
SEEDED = (
    ("sb64_leaf3", dict(W=64, H=64, seed=301, fr=SELECT_ALT, kind=3, p_intra=0.1, odd=0.1, far=0.1)),
    ("sb64_leaf6", dict(W=64, H=64, seed=302, fr=SELECT_ALT_HP, kind=6, p_intra=0.1, odd=0.2)),
    ("sb64_leaf9", dict(W=64, H=64, seed=303, fr=IM.frame(), kind=9, p_intra=0.0, restrict=1)),
    ("sb64_leaf12", dict(W=64, H=64, seed=304, fr=IM.frame(), kind=12, p_intra=0.0)),
    ("edge_72x40", dict(W=72, H=40, seed=311, fr=SELECT_ALT, odd=0.15, far=0.1)),
    ("edge_72x40_restrict", dict(W=72, H=40, seed=312, fr=SELECT_ALT_HP, restrict=1, odd=0.2)),
    ("mix_136x72", dict(W=136, H=72, seed=321, fr=SELECT_ALT, p_intra=0.25, odd=0.1, far=0.1)),
    ("mix_136x72_hp", dict(W=136, H=72, seed=322, fr=SELECT_ALT_HP, p_intra=0.1, odd=0.3)),
    ("mix_136x72_zero_bias", dict(W=136, H=72, seed=323, fr=IM.frame(reference_mode=IM.SELECT), lrf=(IM.GOLDEN, IM.ALTREF), odd=0.1)),
    ("mix_136x72_last_golden", dict(W=136, H=72, seed=324, fr=IM.frame(sign_bias=(0, 0, 1, 0)), lrf=(IM.LAST, IM.GOLDEN), far=0.2)),
    ("compound_only_72x40", dict(W=72, H=40, seed=331, fr=IM.frame(reference_mode=IM.COMPOUND, sign_bias=M.ALT_BIAS), p_intra=0.1)),
    ("big_192x192", dict(W=192, H=192, seed=341, fr=SELECT_ALT, p_leaf=M.BIG_LEAVES, odd=0.05, far=0.05)),
)
_seeded = {}


def seeded(name):
    if name not in _seeded:
        _seeded[name] = D.seeded(**dict(SEEDED)[name])
    return _seeded[name]


def test_exports():
    lib = B.load()
    for s in ("svt_hip_md_inter_modes_batch_device", "svt_hip_md_inter_modes_picture"):
        assert hasattr(lib, s) and s in B.EXPORTS, s
    assert C.sizeof(B.MdInterPicture) == 56


def same(got, want):
    assert got["rc"] == 0 and got["guards"]
    assert got["status"] == want["status"]
    assert np.array_equal(got["ext_out"], want["ext_out"])
    assert np.array_equal(got["cand"], want["cand"])


def check_picture(p):
    """the host form against the model, record for record; closure; the replay's count (label_picture asserts what the replay may get wrong)"""
    want = D.label_picture(p)
    got = D.host_md_inter(p)
    same(got, want)
    status, equal, again = D.closure(p, got)
    assert status == (0, want["status"][0]) and equal
    assert np.array_equal(again["cand"], got["cand"])
    assert got["status"][2] == len(want["unfaithful"]) and got["status"][3] == 0
    return want


@pytest.mark.parametrize("name", [n for n, _ in FIXTURE])
def test_fixture_grids_erased_equal_the_model(name):
    p = dict(FIXTURE)[name]
    want = check_picture(p)
    assert want["status"][0] > 0


@pytest.mark.parametrize("name", [n for n, _ in SEEDED])
def test_seeded_grids_equal_the_model(name):
    check_picture(seeded(name))


def test_the_seeded_grids_reach_every_branch_of_the_rule():
    modes, comp_modes, unfaithful, intra, counts = set(), set(), 0, 0, set()
    for name, _ in SEEDED:
        p = seeded(name)
        want = D.label_picture(p)
        comp = p["mc_mi"]["ref_list"][..., 1] >= 0
        for (r, c), m in want["labels"].items():
            modes.add(m)
            if comp[r, c]:
                comp_modes.add(m)
        unfaithful += len(want["unfaithful"])
        intra += int((p["lf_mi"]["is_inter"] == 0).sum())
        origins = want["cand"]["count"][..., 0] != 0xFF
        counts |= {int(v) for v in want["cand"]["count"][origins].ravel()}
    assert modes == {10, 11, 12, 13} and comp_modes == {10, 11, 12, 13} and unfaithful > 10 and intra > 0 and counts == {0, 1, 2}
    hp = D.label_picture(seeded("mix_136x72_hp"))              # odd differences: some coded with the high-precision bit, some not
    assert 0 < len(hp["unfaithful"]) < hp["status"][1]


def uniform(W, H, fr, lrf=(IM.LAST, IM.ALTREF)):
    """every unit an 8x8 inter leaf of list 0 with a zero MV"""
    shape = (H // 8, W // 8)
    lf, mc = np.zeros(shape, B.LF_MODE_INFO_DTYPE), np.zeros(shape, B.MC_MODE_INFO_DTYPE)
    lf["sb_type"], lf["tx_size"], lf["skip"], lf["is_inter"], lf["filter_level"] = 3, 1, 1, 1, 12
    mc["ref_list"], mc["bw8"], mc["bh8"] = (0, -1), 1, 1
    return dict(W=W, H=H, frame=fr, restrict=0, lrf=lrf, lf_mi=lf, mc_mi=mc)


def put(p, at, mv0, mv1=None):
    p["mc_mi"][at]["mv_row"][0], p["mc_mi"][at]["mv_col"][0] = mv0
    if mv1 is not None:
        p["mc_mi"][at]["ref_list"] = (0, 1)
        p["mc_mi"][at]["mv_row"][1], p["mc_mi"][at]["mv_col"][1] = mv1


def constructed():
    """[(what, picture, unit, expected mode)]"""
    out = []
    a = uniform(64, 64, IM.frame())
    out.append(("the MV is candidate 0 and also zero", a, (1, 1), 10))
    out.append(("no candidate at all and a zero MV", a, (0, 0), 12))
    b = uniform(64, 64, IM.frame())
    put(b, (0, 1), (8, 8)), put(b, (1, 0), (16, -8)), put(b, (1, 1), (16, -8))
    out.append(("the MV is candidate 1 only", b, (1, 1), 11))
    c = uniform(64, 64, IM.frame())
    put(c, (0, 1), (8, 8)), put(c, (1, 0), (16, -8))
    out.append(("a zero MV with two non-zero candidates", c, (1, 1), 12))
    d = uniform(64, 64, SELECT_ALT)
    put(d, (0, 1), (8, 8), (4, 4)), put(d, (1, 1), (8, 8), (6, 6))
    out.append(("candidate 0 for one reference of a compound leaf but not the other", d, (1, 1), 13))
    e = uniform(64, 64, SELECT_ALT)
    put(e, (0, 1), (8, 8), (4, 4)), put(e, (1, 1), (8, 8), (4, 4))
    out.append(("candidate 0 for both references of a compound leaf", e, (1, 1), 10))
    f = uniform(64, 64, IM.frame())
    put(f, (0, 1), (8, 8)), put(f, (1, 1), (9, 8))
    out.append(("one eighth beside candidate 0, no high-precision bit", f, (1, 1), 13))
    return out


def test_constructed_cases_of_the_order():
    for what, p, at, mode in constructed():
        want, got = D.label_picture(p), D.host_md_inter(p)
        same(got, want)
        assert int(got["ext_out"][at]["mode"]) == mode, what
    p = constructed()[-1][1]
    assert D.host_md_inter(p)["status"][2] == 1 and D.host_md_inter(p, allow_hp=1)["status"][2] == 0     # |ref_mv| < 64: the bit is coded


def test_the_difference_bound_and_the_clamp():
    """a leaf whose MV lies 16383 / 16384 from its reference MV in a component, on a picture wide enough that the candidate is not clamped"""
    for delta, count in ((16383, 1), (16384, 1), (16382, 0), (-16382, 0), (-16384, 1)):
        p = uniform(8192, 64, IM.frame())
        put(p, (0, 0), (0, 100)), put(p, (0, 1), (0, 100 + delta))
        got = D.host_md_inter(p)
        same(got, D.label_picture(p))
        assert int(got["ext_out"][0, 1]["mode"]) == 13 and got["status"][2] == count, delta
    p = uniform(64, 64, IM.frame())                      # the candidate is clamped: the MV equals the unclamped value and is not NEARESTMV
    put(p, (0, 0), (0, 3000)), put(p, (0, 1), (0, 3000))
    got = D.host_md_inter(p)
    same(got, D.label_picture(p))
    assert int(got["ext_out"][0, 1]["mode"]) == 13 and int(got["ext_out"][0, 1]["ref_mv_col"][0]) < 3000


@pytest.mark.parametrize("name", ("edge_72x40", "mix_136x72"))
def test_wider_grid_equals_the_tight_result(name):
    """mi_stride = mi_cols + 7 with random bytes behind every row of both grids; the outputs' records behind a row stay untouched"""
    p = seeded(name)
    got = D.host_md_inter(D.with_stride(p, 7, 9))
    same(got, D.label_picture(p))
    cols = p["W"] // 8
    for raw, size, fill in ((got["raw_ext"], 12, 0xA5), (got["raw_cand"], 32, 0x5A)):
        assert (raw[:-D.GUARD].reshape(p["H"] // 8, (cols + 7) * size)[:, cols * size:] == fill).all()


def test_optional_candidates_and_ref_mask():
    p = seeded("mix_136x72")
    want = D.label_picture(p)
    got = D.host_md_inter(p, want_cand=False)
    assert got["rc"] == 0 and got["guards"] and got["status"] == want["status"] and np.array_equal(got["ext_out"], want["ext_out"])
    assert (got["raw_cand"] == 0x5A).all()
    for mask in (0, 2, 8, 10):
        got = D.host_md_inter(p, ref_mask=mask)
        assert got["rc"] == 0 and np.array_equal(got["ext_out"], want["ext_out"]) and np.array_equal(got["cand"], M.mask_cand(want["cand"], mask))


def test_parameters_decide_the_result():
    p = seeded("mix_136x72")
    base = D.label_picture(p)
    for over in (dict(restrict=1), dict(frame=dict(p["frame"], sign_bias=M.ZERO_BIAS, comp_fixed_ref=3, comp_var_ref=(1, 2)), lrf=(IM.LAST, IM.ALTREF))):
        q = dict(p, **over)
        if "frame" in over:             # (the compound pair's order follows the sign bias: keep the grid acceptable)
            q["mc_mi"] = p["mc_mi"].copy()
            comp = q["mc_mi"]["ref_list"][..., 1] >= 0
            q["mc_mi"]["ref_list"][comp] = (1, 0)
        want = D.label_picture(q)
        same(D.host_md_inter(q), want)
        assert not np.array_equal(want["ext_out"], base["ext_out"])


def malformed():
    """[(what, picture, keyword overrides of the call)]: every one answers SVT_MODES_BAD_GRID four times"""
    out = []
    a, e = seeded("mix_136x72"), seeded("edge_72x40")

    def find(p, comp=None, origin=True, intra=False):
        for r in range(p["H"] // 8):
            for c in range(p["W"] // 8):
                lf, mc = p["lf_mi"][r, c], p["mc_mi"][r, c]
                n = M.UNITS[int(lf["sb_type"])]
                if intra:
                    if not lf["is_inter"]:
                        return r, c
                elif lf["is_inter"] and (r % n == 0 and c % n == 0) == origin and (comp is None or (mc["ref_list"][1] >= 0) == comp):
                    return r, c
        raise AssertionError

    def case(what, p, grid, at, field, value, index=None, **over):
        q = dict(p, **{grid: p[grid].copy()})
        if index is None:
            q[grid][at][field] = value
        else:
            q[grid][at][field][index] = value
        out.append((what, q, over))
    for p in (a, e):
        o, os_, oc, u, i = find(p), find(p, comp=False), find(p, comp=True), find(p, origin=False), find(p, intra=True)
        case("rectangular sb_type", p, "lf_mi", o, "sb_type", 4)
        case("sb_type 13", p, "lf_mi", u, "sb_type", 13)
        case("sb_type 255", p, "lf_mi", u, "sb_type", 255)
        case("an origin claims a larger block", p, "lf_mi", (0, 0), "sb_type", 12 if p["lf_mi"][0, 0]["sb_type"] < 12 else 9)
        case("is_inter without a list", p, "mc_mi", u, "ref_list", -1, 0)
        case("a list without is_inter", p, "mc_mi", i, "ref_list", 0, 0)
        case("is_inter cleared on a unit with a list", p, "lf_mi", u, "is_inter", 0)
        case("an inter block below 8x8", p, "lf_mi", o, "sb_type", 0)
        case("ref_list 2", p, "mc_mi", o, "ref_list", 2, 0)
        case("second ref_list 2", p, "mc_mi", oc, "ref_list", 2, 1)
        case("a compound leaf of one list twice", p, "mc_mi", oc, "ref_list", int(p["mc_mi"][oc]["ref_list"][1]), 0)
        case("a compound leaf in the other order", p, "mc_mi", oc, "ref_list", tuple(int(v) for v in p["mc_mi"][oc]["ref_list"][::-1]))
        out.append(("a compound leaf under SINGLE_REFERENCE", p, dict(reference_mode=IM.SINGLE)))
        out.append(("a single leaf under COMPOUND_REFERENCE", p, dict(reference_mode=IM.COMPOUND)))
        out.append(("a compound pair the frame does not know", p, dict(comp_fixed_ref=2, comp_var_ref=(1, 3))))
        out.append(("list_ref_frame[0] = 0", p, dict(list_ref_frame=(0, 3))))
        out.append(("list_ref_frame[1] = 4", p, dict(list_ref_frame=(1, 4))))
        out.append(("list_ref_frame[1] = 255", p, dict(list_ref_frame=(1, 255))))
    case("a block across the picture edge", e, "lf_mi", (4, 8), "sb_type", 6)
    return out


MALFORMED = malformed()


def test_malformed_grids_answer_the_named_value():
    assert len(MALFORMED) >= 35
    for what, p, over in MALFORMED:
        got = D.host_md_inter(p, **over)
        assert got["rc"] == 0 and got["guards"] and got["status"] == D.BAD, what
    single = seeded("sb64_leaf9")               # an unused list's frame is still looked at
    assert D.host_md_inter(single, list_ref_frame=(1, 0))["status"] == D.BAD


def test_entry_point_refusals():
    lib = B.load()
    p = seeded("sb64_leaf6")
    mi, mc = np.ascontiguousarray(p["lf_mi"]), np.ascontiguousarray(p["mc_mi"])
    eo, ca, st = np.zeros(64 * 12, np.uint8), np.zeros(64 * 32, np.uint8), np.full(4, 0x77777777, np.uint32)

    def desc(**over):
        d = B.MdInterPicture()
        d.d_lf_mi, d.d_mc_mi, d.d_ext_out, d.d_cand, d.d_status = mi.ctypes.data, mc.ctypes.data, eo.ctypes.data, ca.ctypes.data, st.ctypes.data
        D.fill_picture(d, p, **{k: v for k, v in over.items() if not k.startswith("d_")})
        for k, v in over.items():
            if k.startswith("d_"):
                setattr(d, k, v)
        return d

    def rc(d, W=64, H=64, stride=8):
        return lib.svt_hip_md_inter_modes_picture(C.byref(d), W, H, stride)
    assert lib.svt_hip_md_inter_modes_picture(None, 64, 64, 8) != 0
    for field in ("d_lf_mi", "d_mc_mi", "d_ext_out", "d_status"):
        assert rc(desc(**{field: None})) != 0, field
    for mask in (1, 0x10, 0x80, 0xF):
        assert rc(desc(ref_mask=mask)) != 0, mask
    assert rc(desc(reference_mode=3)) != 0 and rc(desc(comp_fixed_ref=0)) != 0 and rc(desc(comp_var_ref=(1, 4))) != 0
    assert rc(desc(), W=60) != 0 and rc(desc(), H=0) != 0 and rc(desc(), W=8200) != 0 and rc(desc(), stride=7) != 0
    assert not eo.any() and not ca.any() and (st == 0x77777777).all()          # nothing ran
    assert rc(desc()) == 0 and tuple(int(v) for v in st) == D.label_picture(p)["status"]
    assert rc(desc(reference_mode=IM.SINGLE, comp_fixed_ref=0)) == 0             # (compound references are not looked at where none can occur)


GOLDEN = [g[0] for g in D.GOLDEN]


def test_the_seeds_give_the_stored_grids():
    pics = D.build_golden_pictures()
    assert [str(n) for n in D.golden()["names"]] == GOLDEN == list(pics)
    for name in GOLDEN:
        p, g = pics[name], D.golden_picture(name)
        for k in ("lf_mi", "mc_mi", "qcoeff", "eob_map"):
            assert np.array_equal(p[k], g[k]), (name, k)
        assert (p["frame"], p["restrict"], p["lrf"]) == (g["frame"], g["restrict"], g["lrf"])
    assert os.path.getsize(D.GOLD) < os.path.getsize(IM.GOLD) // 2


@pytest.mark.parametrize("name", GOLDEN)
def test_host_chain_equals_the_reference_tile(name):
    """svt_hip_tokenize_picture -> svt_hip_md_inter_modes_picture -> svt_hip_modes_inter_picture -> svt_hip_boolcode_host: the records are
    those the reference's eb_vp9_find_mv_refs and the four-way comparison gave, the tile is the one the reference wrote for them; the
    same picture labelled all-NEWMV has the recorded byte count"""
    p = D.golden_picture(name)
    tok = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], counts=False)
    got = D.host_md_inter(p, ref_mask=0, want_cand=False)
    assert got["rc"] == 0 and got["guards"] and np.array_equal(got["ext_out"], p["ext"])
    assert got["status"][0] == int((p["ext"]["mode"] >= 10).sum()) and got["status"][1] == int((p["ext"]["mode"] == 13).sum()) and got["status"][2:] == (0, 0)
    assert {int(v) for v in p["ext"]["mode"][p["ext"]["mode"] >= 10]} == {10, 11, 12, 13}
    sizes = []
    for ext in (got["ext_out"], D.all_newmv(p, got["ext_out"])):
        m = IM.host_modes(dict(p, ext=ext), tok["tok_off"])
        assert m["rc"] == 0 and m["n_bools"] != B.MODES_BAD_GRID
        tile = BM.host_code(tokens=tok["tokens"], bools=m["bools"], segments=[tuple(int(v) for v in s) for s in m["segments"]])[0]
        sizes.append(len(tile))
        if not len(sizes) - 1:
            assert tile == p["tile"]
    print(f"{name}: labelled {sizes[0]} bytes, all-NEWMV {sizes[1]} bytes")
    assert sizes[1] == p["all_newmv_bytes"]

"""CPU: the MV-reference derivation (csrc/mvrefs_core.h through the host form svt_hip_mvrefs_picture) against what the reference's
eb_vp9_find_mv_refs derived (tests/golden/mvrefs_reference.npz, written by tests/gen_golden_mvrefs.py) and against the serial Python
model (tests/mvrefs_model.py): every fixture picture on plain and wider grids, optional outputs left out, subsets of the reference
frames, the status words, malformed grids, refusals, and the host chain tokeniser -> MV references -> inter mode info -> bool coder
against the reference's tile bytes, with extension records whose reference MVs and mode contexts no host code computed."""
import ctypes as C

import numpy as np
import pytest

import boolcode_model as BM
import modes_inter_model as IM
import mvrefs_model as M
import svt_testlib as T
import tokenize_model as TM

B = T.B
NAMES = M.names()
CONSISTENT = M.names(1)


def test_exports():
    lib = B.load()
    for s in ("svt_hip_mvrefs_batch_device", "svt_hip_mvrefs_picture"):
        assert hasattr(lib, s) and s in B.EXPORTS, s
    assert C.sizeof(B.MvrefsPicture) == 56


def test_the_fixture_is_what_the_issue_names():
    g = M.fixture()
    sizes = {tuple(int(v) for v in g[f"size|{n}"]) for n in NAMES}
    assert {(64, 64), (72, 40), (136, 136), (8192, 64)} <= sizes
    for shape in [s[0] for s in M.SHAPES]:
        pp = [tuple(int(v) for v in g[f"params|{shape}_{tag}"]) for tag in "abcd"]
        assert {p[0] for p in pp} == {0, 1} and {p[1:5] for p in pp} == {M.ZERO_BIAS, M.ALT_BIAS} and {p[5] for p in pp} == {IM.SINGLE, IM.SELECT}
    assert len(CONSISTENT) == len(NAMES) - 5 and all(M.fixture_picture(n)["status"][0] == 0 for n in CONSISTENT)
    assert all(M.fixture_picture(n)["status"][0] > 0 for n in ("pert_72x40", "pert_136x136"))
    for n in CONSISTENT:        # a consistent picture's extension records hold exactly what is derived
        assert np.array_equal(M.fixture_picture(n)["ext_out"], M.fixture_picture(n)["ext"]), n


def same(got, p, ref_mask=M.ALL_REFS):
    assert got["rc"] == 0 and got["guards"]
    assert got["status"] == p["status"]
    assert np.array_equal(got["ext_out"], p["ext_out"])
    assert np.array_equal(got["cand"], M.mask_cand(p["cand"], ref_mask))


@pytest.mark.parametrize("name", NAMES)
def test_host_form_equals_the_reference(name):
    """plain grids, and mi_stride = mi_cols + 9 with random bytes behind each row (which must stay as they are)"""
    p = M.fixture_picture(name)
    same(M.host_mvrefs(p), p)
    wide = M.with_stride(p, 9, 5)
    got = M.host_mvrefs(wide)
    same(got, p)
    cols = p["W"] // 8
    for raw, size, fill in ((got["raw_ext"], 12, 0xA5), (got["raw_cand"], 32, 0x5A)):
        rows = raw[:-M.GUARD].reshape(p["H"] // 8, (cols + 9) * size)
        assert (rows[:, cols * size:] == fill).all()


def test_model_equals_the_reference_and_meets_the_coverage():
    """the serial model on the stored grids: leaf by leaf the reference's records, and its notes reach everything coverage_complete names"""
    cov = M.new_cover()
    for name in NAMES:
        p = M.fixture_picture(name)
        m = M.derive_picture(p, cov)
        assert np.array_equal(m["cand"], p["cand"]) and np.array_equal(m["ext_out"], p["ext_out"]) and m["status"] == p["status"], name
    assert not M.coverage_complete(cov)


def test_the_seeds_give_the_stored_grids():
    pics = M.build_pictures()
    assert list(pics) == NAMES
    for name in ("sb64_leaf3_b", "mix_136x136_d", "big_192x192_a", "ceil_136x136", "pert_136x136"):
        for k in ("lf_mi", "mc_mi", "ext"):
            assert np.array_equal(pics[name][k], M.fixture_picture(name)[k]), (name, k)


def test_ceilings_are_in_the_fixture():
    for name in ("ceil_64x64", "ceil_136x136", "ceil_8192x64"):
        p = M.fixture_picture(name)
        mv = np.concatenate([p["mc_mi"]["mv_row"].ravel(), p["mc_mi"]["mv_col"].ravel()])
        assert (mv == 32767).any() and (mv == -32768).any()
    wide = M.fixture_picture("ceil_8192x64")["cand"]
    assert (wide["mv_col"] == 32767).any() and (wide["mv_col"] == -32768).any()       # the column clamp's bounds lie beyond int16 there


def test_optional_outputs_may_be_left_out():
    p = M.fixture_picture("mix_136x136_b")
    for want_ext, want_cand in ((False, True), (True, False), (False, False)):
        got = M.host_mvrefs(p, want_ext=want_ext, want_cand=want_cand)
        assert got["rc"] == 0 and got["guards"] and got["status"] == p["status"]
        assert np.array_equal(got["ext_out"], p["ext_out"]) if want_ext else (got["raw_ext"] == 0xA5).all()
        assert np.array_equal(got["cand"], p["cand"]) if want_cand else (got["raw_cand"] == 0x5A).all()


@pytest.mark.parametrize("ref_mask", (0, 2, 4, 8, 6, 10, 12))
def test_ref_mask_subsets(ref_mask):
    for name in ("mix_136x136_b", "pert_136x136", "big_192x192_c"):
        p = M.fixture_picture(name)
        got = M.host_mvrefs(p, ref_mask=ref_mask)
        same(got, p, ref_mask)
        origins = p["cand"]["count"][..., 0] != 0xFF
        for ref in (1, 2, 3):
            assert ((got["cand"]["count"][..., ref - 1][origins] == 0xFF).all()) == (not (ref_mask >> ref) & 1)


def test_parameters_decide_the_result():
    """the restrict flag and the sign biases of the call, not the picture's own, are what the derivation follows"""
    p = M.fixture_picture("mix_136x136_b")
    for restrict, bias in ((1, M.ALT_BIAS), (0, M.ZERO_BIAS), (0, (0, 1, 0, 1))):
        q = dict(p, restrict=restrict, frame=dict(p["frame"], sign_bias=bias))
        want = M.derive_picture(q)
        got = M.host_mvrefs(p, restrict=restrict, bias=bias)
        assert np.array_equal(got["cand"], want["cand"]) and np.array_equal(got["ext_out"], want["ext_out"]) and got["status"] == want["status"]
        assert not np.array_equal(got["cand"], p["cand"])


def _malformed():
    """[(what, picture, well formed?)]: one record of a fixture picture changed"""
    out = []
    a, e = M.fixture_picture("mix_136x136_b"), M.fixture_picture("edge_72x40_b")

    def inter_origin(p, comp=None, non_origin=False):
        for r in range(p["H"] // 8):
            for c in range(p["W"] // 8):
                n = M.UNITS[int(p["lf_mi"][r, c]["sb_type"])]
                at_origin = r % n == 0 and c % n == 0
                if p["lf_mi"][r, c]["is_inter"] and at_origin != non_origin and (comp is None or (p["ext"][r, c]["ref_frame"][1] > 0) == comp):
                    return r, c
        raise AssertionError

    def intra_unit(p):
        r, c = np.argwhere(p["lf_mi"]["is_inter"] == 0)[0]
        return int(r), int(c)

    def case(what, p, good, grid, at, field, value, index=None):
        q = dict(p, **{grid: p[grid].copy()})
        if index is None:
            q[grid][at][field] = value
        else:
            q[grid][at][field][index] = value
        out.append((what, q, good))
    for p in (a, e):
        o, os_, oc, u, i = inter_origin(p), inter_origin(p, comp=False), inter_origin(p, comp=True), inter_origin(p, non_origin=True), intra_unit(p)
        case("rectangular sb_type", p, False, "lf_mi", o, "sb_type", 4)
        case("sb_type 13", p, False, "lf_mi", u, "sb_type", 13)
        case("sb_type 255", p, False, "lf_mi", u, "sb_type", 255)
        case("an origin claims a larger block", p, False, "lf_mi", (0, 0), "sb_type", 12 if p["lf_mi"][0, 0]["sb_type"] < 12 else 9)
        case("reference frame 4", p, False, "ext", u, "ref_frame", 4, 0)
        case("second reference frame 4", p, False, "ext", u, "ref_frame", 4, 1)
        case("is_inter without a reference", p, False, "ext", u, "ref_frame", 0, 0)
        case("a reference without is_inter", p, False, "lf_mi", u, "is_inter", 0)
        case("an intra unit with a reference", p, False, "ext", i, "ref_frame", 1, 0)
        case("an intra unit with a second reference", p, False, "ext", i, "ref_frame", 2, 1)
        case("an intra unit that the prediction grid calls inter", p, False, "mc_mi", i, "ref_list", 0, 0)
        case("an inter unit that the prediction grid calls intra", p, False, "mc_mi", u, "ref_list", -1, 0)
        case("single by ref_frame, compound by ref_list", p, False, "mc_mi", os_, "ref_list", 1, 1)
        case("compound by ref_frame, single by ref_list", p, False, "mc_mi", oc, "ref_list", -1, 1)
        case("an inter block below 8x8", p, False, "lf_mi", o, "sb_type", 0)
        case("inter mode 9", p, False, "ext", o, "mode", 9)
        case("inter mode 14", p, False, "ext", o, "mode", 14)
        # what the stage behind this one checks, and what is not read at all
        case("mode context 7", p, True, "ext", o, "mode_context", 7)
        case("another transform size", p, True, "lf_mi", o, "tx_size", 0)
        case("a mode away from the origin", p, True, "ext", u, "mode", 99)
        case("reference MVs", p, True, "ext", o, "ref_mv_row", -12345, 1)
        case("an intra unit's second list", p, True, "mc_mi", i, "ref_list", 1, 1)
    case("a block across the picture edge", e, False, "lf_mi", (4, 8), "sb_type", 6)
    return out


MALFORMED = _malformed()


def test_malformed_grids_answer_the_named_value():
    assert sum(1 for _, _, good in MALFORMED if not good) >= 30
    for what, p, good in MALFORMED:
        got = M.host_mvrefs(p)
        assert got["rc"] == 0 and got["guards"], what
        if good:
            want = M.derive_picture(p)
            assert got["status"] == want["status"] and np.array_equal(got["cand"], want["cand"]) and np.array_equal(got["ext_out"], want["ext_out"]), what
        else:
            assert got["status"] == (B.MODES_BAD_GRID, B.MODES_BAD_GRID), what


def test_entry_point_refusals():
    lib = B.load()
    p = M.fixture_picture("sb64_leaf6_b")
    mi, mc, ex = (np.ascontiguousarray(p[k]) for k in ("lf_mi", "mc_mi", "ext"))
    eo, ca, st = np.zeros(64 * 12, np.uint8), np.zeros(64 * 32, np.uint8), np.full(2, 0x77777777, np.uint32)

    def desc(**over):
        d = B.MvrefsPicture()
        d.d_lf_mi, d.d_mc_mi, d.d_ext, d.d_ext_out, d.d_cand, d.d_status = mi.ctypes.data, mc.ctypes.data, ex.ctypes.data, eo.ctypes.data, ca.ctypes.data, st.ctypes.data
        M.fill_picture(d, p, M.ALL_REFS)
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def rc(d, W=64, H=64, stride=8):
        return lib.svt_hip_mvrefs_picture(C.byref(d), W, H, stride)
    assert lib.svt_hip_mvrefs_picture(None, 64, 64, 8) != 0
    for field in ("d_lf_mi", "d_mc_mi", "d_ext", "d_status"):
        assert rc(desc(**{field: None})) != 0, field
    for mask in (1, 0x10, 0x80, 0xF):
        assert rc(desc(ref_mask=mask)) != 0, mask
    assert rc(desc(d_ext_out=ex.ctypes.data)) != 0
    assert rc(desc(), W=60) != 0 and rc(desc(), H=0) != 0 and rc(desc(), W=8200) != 0 and rc(desc(), stride=7) != 0
    assert not eo.any() and not ca.any() and (st == 0x77777777).all()          # nothing ran
    assert rc(desc()) == 0 and tuple(int(v) for v in st) == p["status"]


def stripped(p):
    """the picture with extension records that hold ref_frame and the leaf origins' modes only"""
    ext = np.zeros_like(p["ext"])
    ext["ref_frame"], ext["mode"] = p["ext"]["ref_frame"], p["ext"]["mode"]
    return dict(p, ext=ext)


@pytest.mark.parametrize("name", CONSISTENT)
def test_host_chain_equals_the_reference_tile(name):
    """svt_hip_tokenize_picture -> svt_hip_mvrefs_picture -> svt_hip_modes_inter_picture -> svt_hip_boolcode_host: the inter stage's
    extension records are the new stage's output"""
    p = M.fixture_picture(name)
    tok = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], counts=False)
    refs = M.host_mvrefs(stripped(p), ref_mask=0, want_cand=False)
    assert refs["rc"] == 0 and refs["status"] == p["status"]
    m = IM.host_modes(dict(p, ext=refs["ext_out"]), tok["tok_off"])
    assert m["rc"] == 0 and m["n_bools"] != B.MODES_BAD_GRID
    tile = BM.host_code(tokens=tok["tokens"], bools=m["bools"], segments=[tuple(int(v) for v in s) for s in m["segments"]])[0]
    assert tile == p["tile"]

"""CPU: the host form of the mixed stand-in decision (svt_hip_md_mixed_picture, the text the device kernel compiles too) against the
NumPy statement of the rule (md_mixed_model.model), its forced corners, and its equality with svt_hip_md_default_picture when the
intra side is priced out."""
import numpy as np
import pytest

import intra_search_model as S
import md_mixed_model as X
import svt_testlib as T

B = T.B
NONE = B.OIS_NONE
SIZES = [(64, 64), (136, 72), (200, 136)]        # one SB; partial SBs both ways with 8x8 leaves at both edges; 4 x 3 SBs, partial both ways


def inputs(W, H, seed):
    return X.random_me(seed, W, H), S.random_ois(seed + 100, W, H)


def same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("lam,penalty", [(0, 0), (150, 300), (600, 0), (37, 5000)])
def test_host_form_equals_the_model(W, H, lam, penalty):
    me, ois = inputs(W, H, W + H)
    mc, lf, n = X.host(me, ois, W, H, lam, penalty, 17)
    mc_m, lf_m, n_m = X.model(me, ois, W, H, lam, penalty, 17)
    assert same(lf, lf_m), np.argwhere(lf != lf_m)[:8].tolist()
    assert same(mc, mc_m), np.argwhere(mc != mc_m)[:8].tolist()
    assert n == n_m


@pytest.mark.parametrize("W,H", SIZES)
def test_share_of_intra_units_of_the_constructed_inputs(W, H):
    """the inputs every other test uses exercise both sides: established with the model alone, then the host form agrees"""
    me, ois = inputs(W, H, W + H)
    units = (W // 8) * (H // 8)
    _, lf_m, n_m = X.model(me, ois, W, H, 150, 300, 17)
    assert 0.10 * units < n_m < 0.90 * units, (n_m, units)
    if W > 64:                                                                   # (one SB has too few leaves for a variety of sizes)
        assert len(np.unique(lf_m["sb_type"][lf_m["is_inter"] == 0])) >= 2 and len(np.unique(lf_m["sb_type"][lf_m["is_inter"] == 1])) >= 2
    assert X.host(me, ois, W, H, 150, 300, 17)[2] == n_m


@pytest.mark.parametrize("W,H", SIZES)
def test_count_grids_and_record_index_agree(W, H):
    me, ois = inputs(W, H, W + H)
    mc, lf, n = X.host(me, ois, W, H, 150, 300, 9)
    assert n == int((lf["is_inter"] == 0).sum()) and n > 0
    sb_cols = (W + 63) // 64
    seen_sizes = set()
    for ur, uc in np.argwhere(lf["is_inter"] == 0):
        m, g = lf[ur, uc], mc[ur, uc]
        w8 = {3: 1, 6: 2, 9: 4}[int(m["sb_type"])]                               # square, never 64x64, never a unit of 4x4 blocks
        seen_sizes.add(w8)
        assert int(m["tx_size"]) == {1: 1, 2: 2, 4: 3}[w8] and m["skip"] == 0 and m["pad"][0] == 0 and m["filter_level"] == 9
        assert g["bw8"] == w8 and g["bh8"] == w8 and g["ref_list"].tolist() == [-1, -1] and not g["mv_row"].any() and not g["mv_col"].any()
        r0, c0 = ur - ur % w8, uc - uc % w8                                      # aligned to its size, inside the picture, one record all over
        assert r0 + w8 <= H // 8 and c0 + w8 <= W // 8
        assert same(lf[r0:r0 + w8, c0:c0 + w8], np.broadcast_to(m, (w8, w8)).copy())
        # the PU of the leaf from its position: p = first PU of the size + z-order index inside the SB; its record is ois[p - 1]
        n_ = 8 * w8
        p = {8: 21, 16: 5, 32: 1}[n_] + S.zord((c0 % 8) // w8, (r0 % 8) // w8)
        o = ois[(r0 // 8) * sb_cols + c0 // 8, p - 1]
        assert o["sad"] != NONE and (int(m["pad"][1]), int(m["pad"][2])) == (int(o["mode"]), int(o["uv_mode"]))
    assert len(seen_sizes) >= (2 if W > 64 else 1)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("lam", [0, 150, 4000])
def test_priced_out_intra_equals_md_default(W, H, lam):
    me, ois = inputs(W, H, W + H)
    mc, lf, n = X.host(me, ois, W, H, lam, 1 << 24, 23)
    mc_d, lf_d = X.host_default(me, W, H, lam, 23)
    assert n == 0 and same(mc, mc_d) and same(lf, lf_d)


def test_refusals_of_the_host_form():
    import ctypes as C
    lib = B.load()
    me, ois = inputs(64, 64, 1)
    mc, lf = np.zeros((8, 8), dtype=B.MC_MODE_INFO_DTYPE), np.zeros((8, 8), dtype=B.LF_MODE_INFO_DTYPE)
    n = C.c_int32(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [p(me), p(ois), 64, 64, 10, 10, 5, p(mc), p(lf), 8, C.byref(n)]
    for i, bad in [(0, None), (1, None), (7, None), (8, None), (10, None), (2, 60), (3, 4), (9, 7), (6, 64), (6, -1)]:
        a = list(good)
        a[i] = bad
        assert lib.svt_hip_md_mixed_picture(*a) == B.ERR_BAD_PARAMETER, i
    assert n.value == -5 and not mc.view(np.uint8).any() and not lf.view(np.uint8).any()
    assert lib.svt_hip_md_mixed_picture(*good) == 0 and n.value >= 0


# ---- forced corners, on one 64x64 SB ----
def flat(dist8=1000, sad8=5000):
    """one SB in which every PU costs exactly the sum of its children on both sides (ME dist8 per 8x8, OIS sad8 per 8x8)"""
    me = np.zeros((1, 85), dtype=B.ME_RESULT_DTYPE)
    ois = np.zeros((1, B.OIS_PER_SB), dtype=B.OIS_BLOCK_DTYPE)
    for p0, k, f in ((0, 1, 64), (1, 4, 16), (5, 16, 4), (21, 64, 1)):
        me["dist0"][0, p0:p0 + k] = dist8 * f
    for o0, k, f in ((0, 4, 16), (4, 16, 4), (20, 64, 1)):
        ois["sad"][0, o0:o0 + k] = sad8 * f
    ois["mode"], ois["uv_mode"] = 3, 7
    ois["sad"][0, 84:], ois["uv_sad"][0, 84:] = 77, NONE
    return me, ois


def both(me, ois, W, H, lam, penalty):
    got, want = X.host(me, ois, W, H, lam, penalty, 5), X.model(me, ois, W, H, lam, penalty, 5)
    assert same(got[0], want[0]) and same(got[1], want[1]) and got[2] == want[2]
    return got


def test_a_leaf_whose_two_sides_tie_is_inter():
    me, ois = flat()
    me["dist0"][0, 5:21] = 10 ** 6                       # 16x16 PUs far too dear for a merge: the four 32x32 areas split into 16x16 leaves
    me["dist0"][0, 1:5] = 4 * 10 ** 7
    me["dist0"][0, 0] = 4 * 10 ** 8
    ois["sad"][0, 4:20] = 10 ** 6 - 300                  # intra = sad + 300 = inter on every 16x16 PU
    ois["sad"][0, 0:4] = NONE
    mc, lf, n = both(me, ois, 64, 64, 10, 300)
    assert n == 0 and (lf["sb_type"] == 6).all() and (lf["is_inter"] == 1).all()
    ois["sad"][0, 4 + 5] -= 1                            # one below: that leaf alone turns intra
    mc, lf, n = both(me, ois, 64, 64, 10, 300)
    assert n == 4 and (lf["sb_type"] == 6).all()
    x, y = S.unzord(5)
    assert (lf["is_inter"][2 * y:2 * y + 2, 2 * x:2 * x + 2] == 0).all()


def test_a_merge_that_ties_goes_to_the_parent():
    lam = 40
    me, ois = flat()
    ois["sad"][:] = NONE                                 # inter costs only
    me["dist0"][0, 1] = int(me["dist0"][0, 5:9].sum()) + 3 * lam          # 32x32 area 0: exactly on the bound -> merged
    me["dist0"][0, 2] = int(me["dist0"][0, 9:13].sum()) + 3 * lam + 1     # area 1: one above -> its four 16x16
    me["dist0"][0, 0] = 10 ** 9
    mc, lf, n = both(me, ois, 64, 64, lam, 0)
    assert n == 0 and (lf["sb_type"][:4, :4] == 9).all() and (lf["sb_type"][:4, 4:] == 6).all()
    mc_d, lf_d = X.host_default(me, 64, 64, lam, 5)
    assert same(mc, mc_d) and same(lf, lf_d)
    # the 64x64 merge on its bound: cost(0) + lambda == sum of the areas at their best
    me, ois = flat()
    ois["sad"][:] = NONE
    me["dist0"][0, 0] = int(me["dist0"][0, 1:5].sum()) + 4 * lam - lam    # each area merged: p32 + lambda
    mc, lf, n = both(me, ois, 64, 64, lam, 0)
    assert (lf["sb_type"] == 12).all() and (mc["bw8"] == 8).all()
    me["dist0"][0, 0] += 1
    assert (both(me, ois, 64, 64, lam, 0)[1]["sb_type"] == 9).all()
    # the same ties with the intra side as the cheaper one of parent and children
    me, ois = flat(dist8=10 ** 6, sad8=100)
    ois["sad"][0, 0] = int(ois["sad"][0, 4:8].sum()) + 4 * 7 + 3 * lam - 7   # intra(1) = sum intra(children) + 3 lambda, penalty 7
    mc, lf, n = both(me, ois, 64, 64, lam, 7)
    assert (lf["sb_type"][:4, :4] == 9).all() and (lf["is_inter"] == 0).all() and n == 64


def test_records_without_a_block_are_never_intra():
    W, H = 136, 72
    me, ois = X.random_me(5, W, H, scale=50.0), S.random_ois(6, W, H, none_share=0.3)     # ME dear everywhere: intra wherever it exists
    mc, lf, n = both(me, ois, W, H, 20, 0)
    inside = S.inside_mask(W, H)
    assert (ois["sad"][~inside] == NONE).all() and n > 0
    sb_cols = (W + 63) // 64
    n_inter = 0
    for ur in range(H // 8):
        for uc in range(W // 8):
            m = lf[ur, uc]
            w8 = {3: 1, 6: 2, 9: 4, 12: 8}[int(m["sb_type"])]
            p = {1: 21, 2: 5, 4: 1, 8: 0}[w8] + S.zord((uc % 8) // w8, (ur % 8) // w8)
            has_record = p >= 1 and ois[(ur // 8) * sb_cols + uc // 8, p - 1]["sad"] != NONE
            if not has_record:
                assert m["is_inter"] == 1, (ur, uc)
                n_inter += 1
    assert n_inter > 0
    assert (lf["sb_type"][-1, :] == 3).all() and (lf["sb_type"][:, -1] == 3).all()        # 8x8 leaves at both edges (72 = 64 + 8, 136 = 128 + 8)


def test_sums_of_the_largest_distortions_do_not_wrap():
    me, ois = flat()
    ois["sad"][:] = NONE
    me["dist0"][0, 5:21] = 0xFFFFFFFF                    # four children of 2^32 - 1 each: the sum needs 34 bits
    me["dist0"][0, 1:5] = 0xFFFFFFFF                     # parent <= sum + 3 lambda holds only without a wrap (a wrapped sum is ~2^32 - 4)
    me["dist0"][0, 0] = 0xFFFFFFFF
    mc, lf, n = both(me, ois, 64, 64, 0xFFFFFFFF, 0)
    assert (lf["sb_type"] == 12).all()                   # 2^32 - 1 + lambda <= 4 (2^32 - 1 + lambda)
    me["dist0"][0, 1:5] = 0xFFFFFFFF
    me["dist0"][0, 5:21] = 0x50000000                    # 4 x 0x50000000 = 0x1_4000_0000: wraps to 0x40000000 in 32 bits, below the parent
    mc, lf, n = both(me, ois, 64, 64, 0, 0)
    assert (lf["sb_type"] == 12).all() or (lf["sb_type"] == 9).all()
    assert (lf["sb_type"] != 6).all()                    # parent 0xFFFFFFFF <= 0x140000000: merged
    # the intra side: sad + penalty beyond 32 bits stays above every ME distortion
    me, ois = flat(dist8=0x03FFFFFF, sad8=100)
    ois["sad"][0, 0:84] = 0xFFFFFFFE
    mc, lf, n = both(me, ois, 64, 64, 0, 0xFFFFFFFF)
    assert n == 0


@pytest.mark.parametrize("lam,penalty", [(0, 0), (0, 900), (250, 0)])
def test_lambda_and_penalty_of_zero(lam, penalty):
    me, ois = inputs(200, 136, 77)
    mc, lf, n = both(me, ois, 200, 136, lam, penalty)
    assert 0 < n < lf.size
    if lam == 0:                                         # no price on a split: a parent is taken only when it is no dearer than its children
        _, lf1, _ = both(me, ois, 200, 136, 1000, penalty)
        assert (lf1["sb_type"] >= lf["sb_type"]).all() and (lf1["sb_type"] > lf["sb_type"]).any()

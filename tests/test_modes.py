"""CPU: the key-frame mode-info syntax (csrc/modeinfo_core.h through the host form svt_hip_modes_kf_picture) against the reference's
own tile bytes (tests/golden/modes_reference.npz, written by tests/gen_golden_modes.py) and, record for record, against a serial Python
model that carries the context arrays the reference carries (tests/modes_model.py).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import boolcode_model as BM
import modes_model as MM
import svt_testlib as T
import tokenize_model as TM

B = T.B
NAMES = MM.NAMES


def test_abi_symbols_and_struct_sizes():
    lib = B.load()
    for s in ("svt_hip_modes_set_tables", "svt_hip_modes_kf_batch_device", "svt_hip_modes_kf_picture", "svt_hip_modes_segments", "svt_hip_modes_bools_capacity"):
        assert hasattr(lib, s) and s in B.EXPORTS, s
    assert B.MODES_TABLES_DTYPE.itemsize == 1041 and C.sizeof(B.ModesPicture) == 56
    # four segment slots per 8x8 unit of every SB; 4 partition symbols x 3 + skip + 5 modes x 7 bools per unit of the picture
    assert lib.svt_hip_modes_segments(136, 136) == 9 * 64 * 4 and lib.svt_hip_modes_segments(64, 64) == 256
    assert B.MODES_UNIT_BOOLS == 4 * 3 + 1 + 5 * 7 and lib.svt_hip_modes_bools_capacity(72, 40) == 45 * B.MODES_UNIT_BOOLS
    assert lib.svt_hip_modes_segments(70, 64) == 0 and lib.svt_hip_modes_bools_capacity(0, 64) == 0


def test_fixture_holds_what_the_tests_need():
    g, tabs = MM.fixture(), MM.tables()[0]
    assert [str(n) for n in g["names"]] == NAMES
    assert tabs["kf_y_mode_prob"].shape == (10, 10, 9) and tabs["kf_uv_mode_prob"].shape == (10, 9) and tabs["kf_partition_probs"].shape == (16, 3)
    assert all(t.min() >= 1 for t in tabs.values()) and list(tabs["skip_probs"]) == [192, 128, 64]
    assert np.all(g["seconds"] > 0)
    # the pictures are the seeded ones, and together they reach every context (the generator's own assertion, on the committed file)
    cov, types = {}, set()
    for name, W, H, kind, seed in MM.PICTURES:
        p = MM.fixture_picture(name)
        lf, q, emap = MM.make_picture(W, H, kind, seed)
        assert (p["W"], p["H"]) == (W, H) and np.array_equal(lf, p["lf_mi"]) and np.array_equal(q, p["qcoeff"]) and np.array_equal(emap, p["eob_map"])
        MM.serial_walk(lf, W, H, tabs, cov)
        types |= {int(t) for t in np.unique(lf["sb_type"][lf["skip"] == 0])}
        assert len(p["tile"]) > len(p["modes"]) > 0
    classes = ("missing", "4x4", "larger")
    assert cov["partition"] == set(range(16)) and cov["skip"] == {0, 1, 2} and cov["pairs"] == {(a, b) for a in classes for b in classes}
    assert types == set(MM.LEAF_TYPES)


@pytest.mark.parametrize("name", NAMES)
def test_host_chain_equals_the_reference_tile(name):
    """host tokeniser -> host mode-info stage -> host bool coder over its segments = the reference's tile; its bools alone = the
    reference's mode-info bytes"""
    p = MM.fixture_picture(name)
    tile, only, m = MM.host_chain(name)
    assert only == p["modes"]
    assert tile == p["tile"]
    assert np.all(m["guard"] == 0xA5A5) and np.all(m["seg_guard"] == 0x5A5A5A5A)


@pytest.mark.parametrize("name", NAMES)
def test_host_records_equal_the_serial_model(name):
    p, tok = MM.fixture_picture(name), MM.host_tokens(name)
    W, H = p["W"], p["H"]
    recs, leaves = MM.serial_walk(p["lf_mi"], W, H, MM.tables()[0])
    m = MM.host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], W, H)
    assert m["rc"] == 0 and m["n_bools"] == len(recs) and np.array_equal(m["bools"], recs)
    assert m["n_bools"] <= B.load().svt_hip_modes_bools_capacity(W, H)
    # the list without its empty slots is the serial walk's: per leaf its bools, then its Y, Cb, Cr runs from the tokeniser's offsets
    runs = MM.leaf_runs(p["lf_mi"], tok["tok_off"], p["eob_map"], W, H)
    got = [tuple(int(v) for v in s) for s in m["segments"] if s["count"]]
    assert got == MM.coding_order_segments(leaves, runs)
    # the model's own bytes, through the model of the bool coder
    bools = BM.expand(tok["tokens"], recs, MM.coding_order_segments(leaves, runs), BM.tables()[0])
    assert BM.serial_write(bools) == p["tile"]


@pytest.mark.parametrize("name", NAMES)
def test_segment_list_length_slots_and_token_cover(name):
    p, tok = MM.fixture_picture(name), MM.host_tokens(name)
    W, H = p["W"], p["H"]
    m = MM.host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], W, H)
    seg = m["segments"]
    assert len(seg) == B.load().svt_hip_modes_segments(W, H) == T.n_sb(W, H) * 256
    # slot 0 of a unit holds bools, slots 1 .. 3 tokens; empty slots are all zero
    slots = seg.reshape(-1, 4)
    assert np.all(slots["kind"][:, 0][slots["count"][:, 0] > 0] == 1) and not slots["kind"][:, 1:].any()
    empty = seg[seg["count"] == 0]
    assert not empty["first"].any() and not empty["kind"].any()
    # the token segments cover every token of the picture exactly once, the bool segments every bool
    for kind, total in ((0, len(tok["tokens"])), (1, m["n_bools"])):
        seen = np.zeros(total, np.int32)
        for s in seg[(seg["kind"] == kind) & (seg["count"] > 0)]:
            seen[int(s["first"]):int(s["first"]) + int(s["count"])] += 1
        assert np.all(seen == 1), kind
    # a leaf's origin has bools; a unit that is no leaf's origin, or lies outside the picture, has nothing
    sb_cols = (W + 63) // 64
    for i, s in enumerate(slots):
        sb, z = divmod(i, 64)
        c = (sb % sb_cols) * 8 + ((z & 1) | (z >> 1 & 2) | (z >> 2 & 4))
        r = (sb // sb_cols) * 8 + ((z >> 1 & 1) | (z >> 2 & 2) | (z >> 3 & 4))
        origin = False
        if r < H // 8 and c < W // 8:
            n = MM.UNITS[int(p["lf_mi"][r, c]["sb_type"])]
            origin = r % n == 0 and c % n == 0
        assert (s["count"][0] > 0) == origin, (r, c)
        if not origin:
            assert not s["count"].any()


def test_unit_bound_and_capacity_guard():
    name = "sbs_136x136_a"
    p, tok = MM.fixture_picture(name), MM.host_tokens(name)
    W, H = p["W"], p["H"]
    full = MM.host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], W, H)
    # per unit: no slot holds more than the bound the capacity is built from; the bound is reached by nothing less than its derivation
    assert full["segments"]["count"][full["segments"]["kind"] == 1].max() <= B.MODES_UNIT_BOOLS
    short = MM.host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], W, H, capacity=full["n_bools"] - 1)
    assert short["rc"] == 0 and short["n_bools"] == full["n_bools"] and np.array_equal(short["bools"], full["bools"][:-1])
    assert np.all(short["guard"] == 0xA5A5) and len(short["guard"]) == 64
    assert np.array_equal(short["segments"], full["segments"])
    none = MM.host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], W, H, capacity=0)
    assert none["n_bools"] == full["n_bools"] and np.all(none["guard"] == 0xA5A5)


def worst_unit_grid():
    """a 64x64 picture of units of four 4x4 blocks with the longest modes (D153 / D207): at the SB's origin all four nodes are SPLIT"""
    lf = np.zeros((8, 8), B.LF_MODE_INFO_DTYPE)
    lf["sb_type"], lf["tx_size"], lf["filter_level"] = 0, 0, 12
    lf["pad"] = (6 | 7 << 4, 7 | 6 << 4, 7)
    return lf


def test_bound_is_reached_by_the_worst_unit():
    lf = worst_unit_grid()
    W = H = 64
    emap = np.zeros(MM.eob_offsets(W, H)[3], np.uint16)
    tok_off = np.full(emap.size, 0xFFFFFFFF, np.uint32)
    lf["skip"] = 1
    m = MM.host_modes(lf, emap, tok_off, W, H)
    assert m["rc"] == 0
    counts = m["segments"]["count"][m["segments"]["kind"] == 1]
    assert counts[0] == B.MODES_UNIT_BOOLS and counts.max() == B.MODES_UNIT_BOOLS        # 4 x SPLIT + skip + 5 modes of 7 bools
    recs, _ = MM.serial_walk(lf, W, H, MM.tables()[0])
    assert np.array_equal(m["bools"], recs)


def malformed_grids():
    """(what is wrong, grid) for a 64x64 picture of 16x16 leaves with one record changed"""
    base = MM.make_picture(64, 64, 6, 5)[0]
    out = []

    def case(what, r, c, **kw):
        lf = base.copy()
        for k, v in kw.items():
            if k == "pad":
                lf[r, c]["pad"][v[0]] = v[1]
            else:
                lf[r, c][k] = v
        out.append((what, lf))
    case("rectangular sb_type", 2, 2, sb_type=7)
    case("sb_type above 12", 0, 0, sb_type=13)
    case("is_inter", 4, 6, is_inter=1)
    case("luma mode above 9", 7, 7, pad=(1, 10))
    case("chroma mode above 9", 3, 0, pad=(2, 12))
    case("tx_size smaller than the block", 0, 2, tx_size=1)
    case("tx_size larger than the block", 6, 0, tx_size=3)
    lf = base.copy()
    lf[0, 0]["sb_type"], lf[0, 0]["tx_size"] = 0, 0
    lf[0, 0]["pad"][0] = 0xA3                       # block 3 of a 4x4 unit: mode 10
    out.append(("4x4 mode above 9 (and a unit inside a 16x16 leaf)", lf))
    lf = base.copy()
    lf[:4, :4]["sb_type"], lf[:4, :4]["tx_size"] = 9, 3
    lf[1, 1]["sb_type"], lf[1, 1]["tx_size"] = 3, 1
    out.append(("a block inside another", lf))
    return out


def edge_crossing_grid():
    """72x40: a 16x16 leaf at the unit column 8, of which only one column is inside the picture"""
    lf = MM.make_picture(72, 40, "random", 21)[0].copy()
    lf[0:2, 8]["sb_type"], lf[0:2, 8]["tx_size"] = 6, 2
    return lf


@pytest.mark.parametrize("k", range(len(malformed_grids()) + 1))
def test_malformed_grids_answer_the_named_value(k):
    cases = malformed_grids()
    what, lf, W, H = (*cases[k], 64, 64) if k < len(cases) else ("a block crossing the picture edge", edge_crossing_grid(), 72, 40)
    emap = np.zeros(MM.eob_offsets(W, H)[3], np.uint16)
    tok_off = np.full(emap.size, 0xFFFFFFFF, np.uint32)
    m = MM.host_modes(lf, emap, tok_off, W, H)
    assert m["rc"] == 0 and m["n_bools"] == B.MODES_BAD_GRID == 0xFFFFFFFF, what
    assert not m["segments"]["count"].any() and np.all(m["guard"] == 0xA5A5) and np.all(m["seg_guard"] == 0x5A5A5A5A), what


def test_bad_arguments():
    lib, p = B.load(), MM.fixture_picture("sb64_leaf6")
    tok = MM.host_tokens("sb64_leaf6")
    assert MM.host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], 64, 60)["rc"] != 0          # height no multiple of 8
    assert lib.svt_hip_modes_kf_picture(None, None, 64, 64, 8) != 0
    t = MM.tables()[1]
    assert lib.svt_hip_modes_kf_picture(t.ctypes.data_as(C.c_void_p), C.byref(B.ModesPicture()), 64, 64, 8) != 0      # null fields
    # the batch entry point refuses on its arguments alone, before any use of the context
    fake_ctx = C.create_string_buffer(1 << 20)
    arr = (B.ModesPicture * 1)(B.ModesPicture())
    assert lib.svt_hip_modes_kf_batch_device(fake_ctx, 1, arr, 64, 64, 8) != 0 and lib.svt_hip_modes_kf_batch_device(fake_ctx, 33, arr, 64, 64, 8) != 0
    assert lib.svt_hip_modes_kf_batch_device(None, 1, arr, 64, 64, 8) != 0 and lib.svt_hip_modes_set_tables(None, None) != 0


# ---- past the first pass of the scans, and on wider grids (the host forms pinned by the serial models here; the device is compared with
# the host forms in test_gpu_modes.py) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [b[0] for b in MM.BIG])
def test_big_picture_host_chain_equals_the_serial_models(name):
    """289 SBs (more than the 256 lanes of the SB scans, odd, partial on both edges); the all-4x4 picture has more tokens + bools than
    one pass of the bool coder's scan over 256 tiles of 1024 items takes"""
    p, h = next(p for p in MM.big_pictures() if p["name"] == name), MM.big_host(name)
    W, H, tok, m = p["W"], p["H"], h["tok"], h["modes"]
    assert T.n_sb(W, H) == 289 and len(m["segments"]) == 289 * 256
    if name == "big_4x4":
        assert len(tok["tokens"]) + m["n_bools"] > 256 * 1024
    recs, leaves = MM.serial_walk(p["lf_mi"], W, H, MM.tables()[0])
    assert m["n_bools"] == len(recs) <= B.load().svt_hip_modes_bools_capacity(W, H) and np.array_equal(m["bools"], recs)
    assert np.all(m["guard"] == 0xA5A5) and np.all(m["seg_guard"] == 0x5A5A5A5A)
    runs = MM.leaf_runs(p["lf_mi"], tok["tok_off"], p["eob_map"], W, H)
    order = MM.coding_order_segments(leaves, runs)
    assert [s for s in h["segs"] if s[1]] == order
    assert BM.serial_write(BM.expand(tok["tokens"], recs, order, BM.tables()[0])) == h["tile"]


@pytest.mark.parametrize("name", ("edge_72x40_a", "sbs_136x136_a", "big_random"))
def test_host_form_on_a_wider_grid(name):
    """mi_stride = mi_cols + 9, random bytes in the records behind the picture: every output as on the tight grid"""
    if name.startswith("big"):
        p, h = next(p for p in MM.big_pictures() if p["name"] == name), MM.big_host(name)
        tok, tight = h["tok"], h["modes"]
    else:
        p, tok = MM.fixture_picture(name), MM.host_tokens(name)
        tight = MM.host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], p["W"], p["H"])
    wide = TM.with_stride(p["lf_mi"], 9, 2)
    assert wide.shape[1] == p["W"] // 8 + 9 and wide[:, p["W"] // 8:]["sb_type"].max() > 12
    got = MM.host_modes(wide, p["eob_map"], tok["tok_off"], p["W"], p["H"])
    assert got["rc"] == tight["rc"] == 0 and got["n_bools"] == tight["n_bools"] != B.MODES_BAD_GRID
    assert np.array_equal(got["bools"], tight["bools"]) and np.array_equal(got["segments"], tight["segments"])
    assert np.all(got["guard"] == 0xA5A5) and np.all(got["seg_guard"] == 0x5A5A5A5A)

"""CPU: the coefficient tokeniser's rules (csrc/tokenize_core.h through the host entry points) against an independent numpy model
(tests/tokenize_model.py), against the reference's coeff_rate_estimate by the cost identity (tests/golden/rate_reference.npz) and
against the reference's own eb_vp9_tokenize_sb (tests/golden/tokens_reference.npz, written by tests/gen_golden_tokens.py)."""
import ctypes as C

import numpy as np
import pytest

import gen_golden_tokens as G
import modes_model as MM
import svt_testlib as T
import tokenize_model as TM

B = T.B
RATE_KEYS = [k for k in np.load(T.RATE_GOLD).files if k.startswith("bits|")]


def test_scan_tables_equal_the_reference_tables():
    """svt_hip_vp9_scan_tables (inverse scans + the neighbour rule) == the reference's {scan, neighbors} tables, entry for entry"""
    offs, total = T.rate_scan_offsets()
    got_offs, got = TM.product_scan_tables()
    ref = np.load(T.RATE_GOLD)["scan"]
    assert got.size == total == ref.size
    assert got_offs == [offs[(ts, tt)] for ts in range(4) for tt in range(4)]
    assert np.array_equal(got, ref)
    assert np.array_equal(TM.scan_tables()[1], ref)          # the model's own construction


@pytest.mark.parametrize("key", RATE_KEYS)
def test_cost_identity_host_form_and_model(key):
    """the token stream of every block, priced with the reference's tables, is the reference's coeff_rate_estimate of that block"""
    _, seed, w, h, ext = key.split("|")
    case = T.make_rate_case(int(seed), int(w), int(h), extreme=bool(int(ext)))
    want = np.load(T.RATE_GOLD)[key]
    tables = T.rate_tables()[0]
    m_tok, m_off, m_cnt = TM.tokenize_blocks(case)
    h_tok, h_off, h_cnt, guard = TM.host_tokenize_blocks(case)
    assert np.array_equal(m_off, h_off) and np.array_equal(m_tok, h_tok) and np.array_equal(m_cnt, h_cnt)
    assert np.all(guard == 0xA5A5A5A5)
    assert len(want) == len(case["blocks"])
    for i, b in enumerate(case["blocks"]):
        n = 16 << (2 * int(b["tx_size"]))
        t = h_tok[int(h_off[i]):int(h_off[i + 1])]
        assert len(t) == int(b["eob"]) + (int(b["eob"]) < n)
        assert TM.cost_of(t, tables) == int(want[i]), i


def test_class_boundaries():
    case, expect = TM.boundary_case()
    for tokens, tok_off in (TM.tokenize_blocks(case)[:2], TM.host_tokenize_blocks(case)[:2]):
        TM.check_boundary(case, expect, tokens, tok_off)
    assert np.array_equal(TM.tokenize_blocks(case)[0], TM.host_tokenize_blocks(case)[0])


def test_block_form_capacity_and_bad_blocks():
    case, _ = TM.boundary_case()
    full, off, _, _ = TM.host_tokenize_blocks(case)
    cut, off2, _, guard = TM.host_tokenize_blocks(case, capacity=len(full) - 5)
    assert np.array_equal(off, off2) and np.array_equal(cut, full[:-5]) and np.all(guard == 0xA5A5A5A5)
    bad = dict(case, blocks=case["blocks"].copy())
    bad["blocks"]["scan_off"][0] += 2                        # not a table of the canonical layout
    nb = len(bad["blocks"])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = B.load().svt_hip_tokenize_blocks_host(vp(bad["qcoeff"]), C.c_size_t(bad["qcoeff"].size), vp(bad["blocks"]), nb, vp(np.zeros(8, np.uint32)), C.c_uint32(0),
                                               vp(np.zeros(nb + 1, np.uint32)), None)
    assert rc != 0


def test_reference_fixture_covers_the_cases():
    """the generator's own assertion, repeated on the committed file"""
    W, H, pics = TM.fixture_pictures()
    assert (W, H) == (G.W, G.H) and len(pics) == 3
    G.check_coverage(G.coverage(pics))


@pytest.mark.parametrize("k", range(3))
def test_host_form_equals_model_equals_reference(k):
    W, H, pics = TM.fixture_pictures()
    p = pics[k]
    model = TM.tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], W, H)
    host = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], W, H)
    for name in ("tokens", "tok_off", "sb_off", "counts"):
        assert np.array_equal(model[name], host[name]), name
    assert np.all(host["guard"] == 0xA5A5A5A5)
    TM.check_against_fixture(p, host, W, H)
    TM.check_against_fixture(p, model, W, H)


def test_host_picture_capacity_and_optional_counts():
    W, H, pics = TM.fixture_pictures()
    p = pics[2]
    full = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], W, H)
    total = int(full["sb_off"][-1])
    assert 0 < total <= B.load().svt_hip_tokenize_capacity(W, H) == W * H * 3 // 2 + W * H * 3 // 32
    cut = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], W, H, capacity=total - 1, counts=False)
    assert int(cut["sb_off"][-1]) == total and np.array_equal(cut["tokens"], full["tokens"][:-1]) and np.all(cut["guard"] == 0xA5A5A5A5)
    assert np.array_equal(cut["tok_off"], full["tok_off"])


def test_all_skip_picture_emits_nothing():
    W, H, pics = TM.fixture_pictures()
    p = pics[0]
    lf = p["lf_mi"].copy()
    lf["skip"] = 1
    got = TM.host_tokenize_picture(lf, np.zeros_like(p["qcoeff"]), np.zeros_like(p["eob_map"]), W, H)
    assert int(got["sb_off"][-1]) == 0 and np.all(got["tok_off"] == TM.NO_OFFSET) and not got["counts"].any()


def test_tok_picture_layout():
    assert C.sizeof(B.TokPicture) == 64
    import os, subprocess, tempfile
    src = '#include <stdio.h>\n#include "svtvp9_hip.h"\nint main(void){printf("%zu", sizeof(svt_tok_picture));return 0;}'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", f"{T.ROOT}/include", os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        assert int(subprocess.check_output([os.path.join(td, "s")])) == 64


# ---- past the first pass of the scans, at the ceilings of the emit kernel's staging arrays, on wider grids (the host form pinned by the
# model here; the device is compared with the host form in test_gpu_tokenize.py) -------------------------------------------------------
PICTURE_OUTPUTS = ("tokens", "tok_off", "sb_off", "counts")


@pytest.mark.parametrize("name", [b[0] for b in MM.BIG])
def test_big_picture_host_form_equals_model(name):
    """289 SBs: every lane of the SB scan takes two entries, the last ones none"""
    p = next(p for p in MM.big_pictures() if p["name"] == name)
    W, H = p["W"], p["H"]
    assert T.n_sb(W, H) == 289
    host = MM.big_host(name)["tok"]
    model = TM.tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], W, H)
    for out in PICTURE_OUTPUTS:
        assert np.array_equal(model[out], host[out]), out
    assert np.all(host["guard"] == 0xA5A5A5A5) and len(host["tokens"]) == int(host["sb_off"][-1]) > 65536


def coded_blocks_per_sb(tok_off, W, H):
    """entries of tok_off that hold an offset, per SB"""
    w4, h4 = W // 4, H // 4
    eoff = MM.eob_offsets(W, H)
    sb_cols = (W + 63) // 64
    n = np.zeros(T.n_sb(W, H), np.int64)
    for plane, (pw, ph, u) in enumerate(((w4, h4, 16), (w4 // 2, h4 // 2, 8), (w4 // 2, h4 // 2, 8))):
        m = tok_off[eoff[plane]:eoff[plane + 1]].reshape(ph, pw) != TM.NO_OFFSET
        for y, x in zip(*np.nonzero(m)):
            n[(y // u) * sb_cols + x // u] += 1
    return n


@pytest.mark.parametrize("k", range(len(MM.DENSE)))
def test_dense_pictures_fill_every_sb(k):
    """6144 tokens in every SB (49 152 in the emit kernel's run of 8 SBs); for units of four 4x4 blocks all 384 block slots of an SB"""
    W, H, t, seed, kw = MM.DENSE[k]
    lf, q, emap = MM.dense_picture(W, H, t, seed, **kw)
    assert not lf["skip"].any() and np.all(lf["sb_type"] == t)
    short = kw.get("short", False)
    assert np.count_nonzero(q == 0) == (emap.astype(np.int64) > 0).sum() // 2 * short        # every coefficient, but the zeroed last positions
    host = TM.host_tokenize_picture(lf, q, emap, W, H)
    model = TM.tokenize_picture(lf, q, emap, W, H)
    for out in PICTURE_OUTPUTS:
        assert np.array_equal(model[out], host[out]), out
    assert np.all(host["guard"] == 0xA5A5A5A5)
    assert np.all(np.diff(host["sb_off"].astype(np.int64)) == 6144) and len(host["tokens"]) == 6144 * T.n_sb(W, H)
    tok = TM.unpack(host["tokens"])[0]
    assert np.count_nonzero(tok == TM.EOB_TOKEN) == (np.count_nonzero(emap) // 2 if short else 0)
    if t == 0:
        assert np.all(coded_blocks_per_sb(host["tok_off"], W, H) == 384)
    else:
        assert np.all(coded_blocks_per_sb(host["tok_off"], W, H) == 6)
    c = host["counts"]
    if kw.get("ones"):
        # ONE at the 4 x 1003 band-5 positions of the luma 32x32 blocks of 8 SBs: the most one bin can receive (a bin is one row and one
        # token, and these are all the positions of the row, so the dword's other half -- the row's ZERO -- is empty); the two chroma planes share a row: half of it
        assert int(c.max()) == 32096 == 8 * 4 * 1003 and np.count_nonzero(c == 32096) == 1 and np.count_nonzero(c == 16048) == 1
        assert int(c[int(c.argmax()) ^ 1]) == 0
    elif "values" in kw:
        # tokens 8 and 9 (one energy class, so one row) share a dword: both of its halves are large
        top = int(c.argmax())
        assert int(c[top]) + int(c[top ^ 1]) == 32096 and min(int(c[top]), int(c[top ^ 1])) > 15000
    else:
        assert np.count_nonzero(tok == 10) > 0             # values of at least 67 occur


STRIDE_CASES = ("edge_72x40_a", "sbs_136x136_a", "big_random")


def stride_case(name):
    """(W, H, lf_mi, qcoeff, eob_map) of a fixture picture of the mode-info stage, or of a big picture"""
    p = MM.fixture_picture(name) if name in MM.NAMES else next(p for p in MM.big_pictures() if p["name"] == name)
    return p["W"], p["H"], p["lf_mi"], p["qcoeff"], p["eob_map"]


@pytest.mark.parametrize("name", STRIDE_CASES)
def test_host_picture_form_on_a_wider_grid(name):
    """mi_stride = mi_cols + 9, random bytes in the records behind the picture: every output as on the tight grid"""
    W, H, lf, q, emap = stride_case(name)
    tight = MM.big_host(name)["tok"] if name.startswith("big") else TM.host_tokenize_picture(lf, q, emap, W, H)
    wide = TM.with_stride(lf, 9, 1)
    assert wide.shape == (H // 8, W // 8 + 9) and np.array_equal(wide[:, :W // 8], lf) and wide[:, W // 8:]["sb_type"].max() > 12
    got = TM.host_tokenize_picture(wide, q, emap, W, H)
    for out in PICTURE_OUTPUTS:
        assert np.array_equal(got[out], tight[out]), out
    assert np.all(got["guard"] == 0xA5A5A5A5)


def test_block_form_above_1024_blocks():
    """more than 2048 blocks: every lane of the block scan takes three entries"""
    case = T.make_rate_case(3, 512, 256)
    assert len(case["blocks"]) > 2048
    m_tok, m_off, m_cnt = TM.tokenize_blocks(case)
    h_tok, h_off, h_cnt, guard = TM.host_tokenize_blocks(case)
    assert np.array_equal(m_off, h_off) and np.array_equal(m_tok, h_tok) and np.array_equal(m_cnt, h_cnt) and np.all(guard == 0xA5A5A5A5)
    want, tables = T.oracle_rate_batch(case), T.rate_tables()[0]
    for i in range(len(case["blocks"])):
        assert TM.cost_of(h_tok[int(h_off[i]):int(h_off[i + 1])], tables) == int(want[i]), i

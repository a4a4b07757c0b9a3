"""CPU: the forward coefficient-probability update's host form (svt_hip_coef_update_picture, the text of csrc/coef_update_core.h) against
the reference's recorded results (tests/golden/coef_update_reference.npz: header bytes and tables after write_compressed_header under
TWO_LOOP), against the Python model on seeded streams and on a case whose sums leave 32 bits, the tables against the recorded ones, the
eob_branch scan as one run against a scan block by block, the header writer and reader around the stage, and the round trip through
the tile reader."""
import ctypes as C

import numpy as np
import pytest

import boolcode_model as BM
import coef_update_model as CM
import frame_model as FM
import modes_inter_model as IM
import modes_model as MM
import svt_testlib as T
import tokenize_model as TM
from test_tile_read_inter import IT, KT, Outputs, params_of, same_grids

B = T.B
G = CM.fixture()
NAMES = [str(n) for n in G["names"]]
DEFAULT = BM.tables()[0]["coef_probs"].reshape(-1)


def frame_params(fr, **kw):
    """the parameter set behind a fixture case's four frame values (inter, reference_mode, allow_comp_inter_inter, allow_hp)"""
    inter, mode, comp, hp = (int(v) for v in fr)
    return FM.inter(reference_mode=mode, allow_comp_inter_inter=comp, allow_hp=hp, **kw) if inter else FM.params(**kw)


_host = {}


def host_case(name):
    """the host form on a fixture case (computed once, left unchanged)"""
    if name not in _host:
        pre, suf = CM.header_parts(frame_params(G[f"frame|{name}"]))
        tok = G[f"tokens|{name}"]
        _host[name] = CM.host_picture(tok, CM.counts_of(tok), old_probs=G.get(f"old|{name}"), prefix=pre, suffix=suf)
    return _host[name]


@pytest.mark.parametrize("name", NAMES)
def test_host_form_equals_the_reference(name):
    h = host_case(name)
    assert np.all(h["guard"] == 0xA5A5) and h["segment"] == (0, h["n"], 1) and h["result"]["hdr_bools"] == h["n"]
    assert np.array_equal(h["probs"], G[f"probs|{name}"])
    coded = BM.host_code(bools=h["bools"], segments=[(0, h["n"], 1)])[0]
    assert coded == bytes(G[f"bytes|{name}"])
    rc, hdr, ub, cb, guard = CM.header_coef(frame_params(G[f"frame|{name}"]), h["bools"])
    assert rc == 0 and hdr[ub:] == coded and cb == len(coded) and np.all(guard == 0xA5)
    exits = G[f"exits|{name}"]            # 0 not searched, 1 no entry updates, 2 savings negative, 3 sent
    assert list(h["result"]["sent"]) == [int(e == 3) for e in exits]
    assert list(h["result"]["updated"]) == list(G[f"updates|{name}"]) and list(h["result"]["savings"]) == list(G[f"savings|{name}"])


def test_the_fixture_reaches_every_exit_and_every_arm():
    assert set(G["coverage"]) == {"not_searched", "no_entry", "negative", "sent", "subexp_16", "subexp_32", "subexp_64", "uniform_short", "uniform_long", "newp_above",
                                  "newp_below"}
    assert any(f"old|{n}" in G and (G[f"old|{n}"] == 1).any() and (G[f"old|{n}"] == 255).any() for n in NAMES)
    tot = {n: [int(CM.eob_branch(G[f"tokens|{n}"])[144 * t:144 * t + 144].reshape(4, 36)[:, :6].sum()) for t in range(4)] for n in ("tx_totals_20", "tx_totals_21")}
    assert tot["tx_totals_20"][0] == 20 and tot["tx_totals_21"][0] == 21
    assert G["exits|tx_totals_20"][0] == 0 and G["exits|tx_totals_21"][0] != 0


def test_tables_equal_the_recorded_ones():
    lib = B.load()
    assert np.array_equal(np.ctypeslib.as_array(lib.svt_hip_coef_update_cost_table(), (256,)), G["prob_cost"])
    remap, bits = np.zeros(255 * 255, np.uint8), np.zeros(255 * 255, np.uint8)
    lib.svt_hip_coef_update_remap_tables(remap.ctypes.data, bits.ctypes.data)
    assert np.array_equal(remap, G["remap"]) and np.array_equal(bits, G["update_bits"])
    m_remap, m_bits = CM.remap_tables()
    assert np.array_equal(m_remap, G["remap"]) and np.array_equal(m_bits, G["update_bits"])
    assert int(lib.svt_hip_coef_update_bools_capacity()) == B.CU_PREFIX_MAX + B.CU_SECTION_MAX + B.CU_SUFFIX_MAX


SEEDED = [(1, "default", None, 20000), (2, "zeros", "ends", 9000), (3, "large", "random", 9000), (4, "ones", None, 700), (5, "default", "random", 120)]


@pytest.mark.parametrize("seed,mix,old,n", SEEDED)
def test_host_form_equals_the_model_on_seeded_streams(seed, mix, old, n):
    tok = CM.seeded_stream(seed, n, mix=mix)
    oldp = None if old is None else CM.seeded_probs(seed, ends=old == "ends")
    pre, suf = (CM.rec(1, 128), CM.rec(1, 128), CM.rec(0, 128)), (CM.rec(0, 252),) * 7
    h = CM.host_picture(tok, CM.counts_of(tok), old_probs=oldp, prefix=pre, suffix=suf, device_count=bool(seed & 1))
    m = CM.decide(CM.counts_of(tok), CM.eob_branch(tok), DEFAULT if oldp is None else oldp, prefix=pre, suffix=suf)
    assert np.array_equal(h["eob"], CM.eob_branch(tok)) and np.array_equal(h["bools"], m["bools"]) and np.array_equal(h["probs"], m["probs"])
    assert list(h["result"]["updated"]) == m["updated"] and list(h["result"]["sent"]) == m["sent"] and list(h["result"]["savings"]) == m["savings"]
    assert h["result"]["tokens"] == len(tok) and np.all(h["guard"] == 0xA5A5)


def test_records_beyond_max_tokens_are_not_read():
    tok = CM.seeded_stream(7, 3000)
    h = CM.host_picture(tok, CM.counts_of(tok), device_count=True, max_tokens=1000)
    assert np.array_equal(h["eob"], CM.eob_branch(tok[:1000])) and h["result"]["tokens"] == 1000


def test_eob_branch_as_one_run_equals_the_scan_block_by_block():
    """the tokeniser's d_tok_off names every block's first record: restarting the predecessor test there changes nothing"""
    for name, kind, pic, fp in CM.real_pictures():
        s = CM.host_stream(kind, pic)
        off = s["tok"]["tok_off"]
        starts = np.sort(off[off != B.TOK_NONE])
        assert len(starts) > 20 and starts[0] == 0
        one = CM.eob_branch(s["tokens"])
        assert np.array_equal(one, CM.eob_branch_per_block(s["tokens"], starts)), name
        h = CM.host_picture(s["tokens"], s["counts"])
        assert np.array_equal(h["eob"], one), name
        # tx_totals = the blocks tokenised at a size
        tot = [int(one[144 * t:144 * t + 144].reshape(4, 36)[:, :6].sum()) for t in range(4)]
        assert sum(tot) == len(starts), name
    tok = CM.seeded_stream(9, 8000, mix="zeros")
    assert np.array_equal(CM.eob_branch(tok), CM.eob_branch_per_block(tok, CM.block_starts(tok)))
    # and it would not hold for a stream cut inside a block: the model tells the two apart
    assert not np.array_equal(CM.eob_branch(tok), CM.eob_branch_per_block(tok, np.arange(0, len(tok), 7)))


@pytest.mark.parametrize("name", [c[0] for c in FM.CASES])
def test_a_picture_without_counts_gives_the_plain_headers_bytes(name):
    fp = dict(FM.CASES)[name]
    pre, suf = CM.header_parts(fp)
    h = CM.host_picture(np.zeros(0, np.uint32), np.zeros(B.TOK_COUNTS, np.uint32), prefix=pre, suffix=suf)
    assert list(h["bools"]) == list(pre) + [CM.rec(0, 128)] * 4 + list(suf) and np.array_equal(h["probs"], DEFAULT)
    rc, hdr, ub, cb, guard = CM.header_coef(fp, h["bools"])
    assert rc == 0 and hdr == FM.host_header_bytes(fp) and np.all(guard == 0xA5)


def read_back(frame, kind, pic, old_probs=None):
    """the new header reader, then svt_hip_tile_read_host under the table it leaves: (info, tables, the tile reader's result)"""
    lib = B.load()
    buf = np.frombuffer(frame, np.uint8).copy()
    info, tabs = B.FrameReadInfo(), CM.tables_with(DEFAULT if old_probs is None else old_probs)
    vp = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    last = (C.c_int8 * 4)(*FM.DEFAULT_REF_DELTAS), (C.c_int8 * 2)(0, 0)
    assert lib.svt_hip_frame_read_header_host(vp(buf), len(buf), *last, C.byref(info)) == B.ERR_UNSUPPORTED       # the plain reader keeps refusing
    rc = lib.svt_hip_frame_read_header_coef_host(vp(buf), len(buf), *last, C.byref(info), vp(tabs))
    assert rc == 0, lib.svt_hip_last_error()
    W, H = pic["W"], pic["H"]
    fr = pic.get("frame", IM.frame())
    out = Outputs(W, H, W // 8)
    par = params_of(W, H, W // 8, fr, pic.get("restrict", 0), pic.get("lrf", (IM.LAST, IM.ALTREF)), int(pic["lf_mi"]["filter_level"][0, 0]), intra_only=int(kind == "key"))
    at = info.uncompressed_bytes + info.compressed_bytes
    tile = buf[at:].copy()
    rc = lib.svt_hip_tile_read_host(vp(tile), len(tile), C.byref(par), vp(tabs), vp(KT), vp(IT), *out.pointers())
    assert rc == 0, lib.svt_hip_last_error()
    return info, tabs, out.result()


def check_round_trip(kind, pic, fp, frame, stage_probs, what):
    info, tabs, got = read_back(frame, kind, pic)
    assert np.array_equal(tabs["coef_probs"][0], stage_probs), what
    assert got["guards"] and np.array_equal(got["qcoeff"], pic["qcoeff"]) and np.array_equal(got["eob_map"], np.asarray(pic["eob_map"]).view(np.uint16)), what
    if kind == "key":
        assert all(np.array_equal(got["lf_mi"][f], pic["lf_mi"][f]) for f in ("sb_type", "tx_size", "skip", "is_inter", "pad")), what
    else:
        same_grids(got, pic, what)
    assert got["res"]["past_end"] == 0


@pytest.mark.parametrize("k", range(4))
def test_round_trip_through_the_header_and_tile_readers(k):
    name, kind, pic, fp = CM.real_pictures()[k]
    a, b = CM.host_frame(kind, pic, fp, update=True), CM.host_frame(kind, pic, fp, update=False)
    assert a["frame"] == bytes(G[f"frame_with|{name}"]) and b["frame"] == bytes(G[f"frame_without|{name}"])
    assert sum(a["stage"]["result"]["sent"]) > 0 and not np.array_equal(a["probs"], DEFAULT)
    check_round_trip(kind, pic, fp, a["frame"], a["probs"], name)


_sparse = {}


def sparse_picture():
    """256 x 256, built directly (no encode): a random quad-tree whose coded blocks hold a few coefficients each -- short blocks, large
    values: statistics far from the default table's"""
    if not _sparse:
        lf, q, emap = MM.make_picture(256, 256, "random", 77)
        _sparse.update(W=256, H=256, lf_mi=lf, qcoeff=q, eob_map=emap)
    return _sparse


def test_a_stream_far_from_the_defaults_is_strictly_smaller_with_updates():
    pic = sparse_picture()
    fp = FM.params(width=256, height=256, refresh_frame_context=0, frame_parallel_decoding_mode=1)
    a, b = CM.host_frame("key", pic, fp, update=True), CM.host_frame("key", pic, fp, update=False)
    assert len(a["frame"]) < len(b["frame"]) and len(a["header"]) > len(b["header"]) and len(a["tile"]) < len(b["tile"])
    saved = sum(int(s) for s, t in zip(a["stage"]["result"]["savings"], a["stage"]["result"]["sent"]) if t) / 512 / 8
    print(f"256x256: {len(b['frame'])} -> {len(a['frame'])} bytes; the stage estimated {saved:.0f} bytes")
    check_round_trip("key", pic, fp, a["frame"], a["probs"], "sparse")


def test_sums_beyond_32_bits_equal_the_model():
    """a branch count of 2^20: count * cost passes 2^31 (the model's peak says so), where the reference's cost_branch256 wraps; the host
    form's 64-bit sums equal the model's.  Not a case of the reference fixture"""
    row = ((1 * 2 + 0) * 2 + 1) * 36 + 1 * 6 + 2           # 8x8, luma, inter, band 1, context 2
    one = np.uint32(row << 4 | 1)
    tok = np.concatenate([np.full(1 << 20, one, np.uint32), CM.seeded_stream(11, 4000, groups=(4, 5, 6, 7))])
    counts, eob = CM.counts_of(tok), CM.eob_branch(tok)
    assert counts[12 * row + 1] >= 1 << 20
    old = DEFAULT.copy()
    old[3 * row + 1] = 255              # "ZERO nearly always" against 2^20 ONEs: the old cost alone is 2^20 * cost_one(255) = 2^32
    m = CM.decide(counts, eob, old)
    assert m["peak"] >= 2 ** 32
    h = CM.host_picture(tok, counts, old_probs=old)
    assert np.array_equal(h["bools"], m["bools"]) and np.array_equal(h["probs"], m["probs"]) and list(h["result"]["savings"]) == m["savings"]
    assert m["sent"][1] == 1 and max(m["savings"]) >= 2 ** 31 and h["probs"][3 * row + 1] < 8


def test_refusals_write_nothing():
    lib = B.load()
    tok = CM.seeded_stream(3, 500)
    counts = CM.counts_of(tok)
    bools, n = np.full(int(lib.svt_hip_coef_update_bools_capacity()), 0xA5A5, np.uint16), np.full(1, 0x77777777, np.uint32)
    eob, probs, seg, res = np.zeros(576, np.uint32), np.zeros(1728, np.uint8), np.zeros(1, B.BOOL_SEGMENT_DTYPE), np.zeros(1, B.CU_RESULT_DTYPE)

    def pic(**over):
        p = B.CuPicture()
        p.d_tokens, p.n_tokens, p.max_tokens, p.d_counts = tok.ctypes.data, len(tok), len(tok), counts.ctypes.data
        p.d_eob_branch, p.d_probs, p.d_hdr_bools, p.d_n_hdr_bools, p.d_segment, p.d_result = (eob.ctypes.data, probs.ctypes.data, bools.ctypes.data, n.ctypes.data,
                                                                                              seg.ctypes.data, res.ctypes.data)
        for k, v in over.items():
            setattr(p, k, v)
        return p
    tabs = BM.tables()[1]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert lib.svt_hip_coef_update_picture(C.byref(pic()), vp(tabs)) == 0 and n[0] == res[0]["hdr_bools"] >= 4
    bools[:], n[0] = 0xA5A5, 0x77777777
    assert lib.svt_hip_coef_update_picture(None, vp(tabs)) != 0 and lib.svt_hip_coef_update_picture(C.byref(pic()), None) != 0
    for field in ("d_counts", "d_eob_branch", "d_probs", "d_hdr_bools", "d_n_hdr_bools", "d_segment", "d_result", "d_tokens"):
        assert lib.svt_hip_coef_update_picture(C.byref(pic(**{field: None})), vp(tabs)) != 0, field
    assert lib.svt_hip_coef_update_picture(C.byref(pic(n_prefix=B.CU_PREFIX_MAX + 1)), vp(tabs)) != 0
    assert lib.svt_hip_coef_update_picture(C.byref(pic(n_suffix=B.CU_SUFFIX_MAX + 1)), vp(tabs)) != 0
    assert np.all(bools == 0xA5A5) and n[0] == 0x77777777
    # the header writer: a buffer too short for the coded records, null arguments
    fp = FM.params()
    h = host_case("seeded_default")
    assert CM.header_coef(fp, h["bools"], capacity=40)[0] != 0
    s = FM.struct(fp)
    u = C.c_uint32()
    assert lib.svt_hip_frame_header_coef_host(C.byref(s), None, 0, vp(bools), 64, C.byref(u), C.byref(u)) != 0
    assert lib.svt_hip_frame_header_parts_host(C.byref(s), None, C.byref(u), vp(bools), C.byref(u)) != 0

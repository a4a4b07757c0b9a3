"""GPU: the key-frame mode-info stage (csrc/modeinfo.hip) through the C ABI, exactly against the host form (svt_hip_modes_kf_picture) and
the reference's tile bytes (tests/golden/modes_reference.npz): pictures singly and in batches, the chain tokeniser -> mode info -> bool
coder without a host round trip, the same chain behind the intra encode pass on a searched grid, capacity guard, malformed grids; and,
against the host forms alone (which test_modes.py pins to the serial models), pictures of 289 SBs, the unit with the most bools, wider grids."""
import ctypes as C

import numpy as np
import pytest
import torch

import boolcode_model as BM
import encdec_model as M
import modes_model as MM
import svt_testlib as T
import tokenize_model as TM
from test_gpu_encdec import dev, flags_of
from test_gpu_tokenize import KEY, TokBuffers, tokenize_device, upload
from test_modes import edge_crossing_grid, malformed_grids, worst_unit_grid

B = T.B
pytestmark = pytest.mark.gpu
GUARD16, GUARD32, GUARD8 = 0x5A5A, 0x5A5A5A5A, 0x5A


@pytest.fixture(scope="module")
def ctx():
    lib, c = B.load(), C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    B.check(lib.svt_hip_boolcode_set_tables(c, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_set_tables(c, MM.tables()[1].ctypes.data_as(C.c_void_p)))
    yield c
    lib.svt_hip_ctx_destroy(c)


class ModesBuffers:
    """device outputs of one picture, each with guard words behind it; capacity None = svt_hip_modes_bools_capacity"""

    def __init__(self, W, H, capacity=None):
        lib = B.load()
        self.cap = int(lib.svt_hip_modes_bools_capacity(W, H)) if capacity is None else capacity
        self.n_seg = int(lib.svt_hip_modes_segments(W, H))
        self.bools = torch.full((self.cap + 64,), GUARD16, dtype=torch.int16, device="cuda")
        self.segs = torch.full((3 * self.n_seg + 24,), GUARD32, dtype=torch.int32, device="cuda")
        self.n = torch.full((8,), GUARD32, dtype=torch.int32, device="cuda")

    def struct(self, lf_t, emap_t, tok_off_t):
        p = B.ModesPicture()
        p.d_lf_mi, p.d_eob_map, p.d_tok_off = lf_t.data_ptr(), emap_t.data_ptr(), tok_off_t.data_ptr()
        p.d_bools, p.d_segments, p.d_n_bools, p.capacity = self.bools.data_ptr(), self.segs.data_ptr(), self.n.data_ptr(), self.cap
        return p

    def result(self):
        bools, segs, n = self.bools.cpu().numpy().view(np.uint16), self.segs.cpu().numpy().view(np.uint32), self.n.cpu().numpy().view(np.uint32)
        total = int(n[0])
        got = bools[:min(total, self.cap)].copy() if total != B.MODES_BAD_GRID else np.zeros(0, np.uint16)
        return dict(bools=got, n_bools=total, segments=segs[:3 * self.n_seg].view(B.BOOL_SEGMENT_DTYPE).copy(), guard=bools[self.cap:], seg_guard=segs[3 * self.n_seg:],
                    n_guard=n[1:])


def modes_device(ctx, W, H, inputs, bufs=None, mi_stride=None):
    """inputs: [(lf_t, emap_t, tok_off_t)] device tensors.  Enqueues one svt_hip_modes_kf_batch_device; returns the buffers (not yet synchronised)"""
    bufs = bufs or [ModesBuffers(W, H) for _ in inputs]
    arr = (B.ModesPicture * len(inputs))(*[b.struct(*i) for b, i in zip(bufs, inputs)])
    B.check(B.load().svt_hip_modes_kf_batch_device(ctx, len(inputs), arr, W, H, mi_stride or W // 8))
    return bufs


def same(got, want):
    assert got["n_bools"] == want["n_bools"]
    assert np.array_equal(got["bools"], want["bools"]) and np.array_equal(got["segments"], want["segments"])
    assert np.all(got["guard"] == GUARD16) and np.all(got["seg_guard"] == GUARD32) and np.all(got["n_guard"] == GUARD32)


def upload_fixture(name):
    p, tok = MM.fixture_picture(name), MM.host_tokens(name)
    return dev(np.ascontiguousarray(p["lf_mi"]).view(np.uint8)), dev(np.ascontiguousarray(p["eob_map"]).view(np.int16)), dev(tok["tok_off"].view(np.int32))


def host_of(name):
    p, tok = MM.fixture_picture(name), MM.host_tokens(name)
    return MM.host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], p["W"], p["H"])


@pytest.mark.parametrize("name", MM.NAMES)
def test_single_picture_equals_the_host_form(ctx, name):
    p = MM.fixture_picture(name)
    inputs = [upload_fixture(name)]
    torch.cuda.synchronize()
    bufs = modes_device(ctx, p["W"], p["H"], inputs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(bufs[0].result(), host_of(name))


@pytest.mark.parametrize("size", ((64, 64), (72, 40), (136, 136)))
def test_batch_of_one_geometry_equals_the_host_form(ctx, size):
    names = [n for n, W, H, _, _ in MM.PICTURES if (W, H) == size]
    assert len(names) >= 2
    inputs = [upload_fixture(n) for n in names]
    torch.cuda.synchronize()
    bufs = modes_device(ctx, size[0], size[1], inputs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    for n, b in zip(names, bufs):
        same(b.result(), host_of(n))


class Tile:
    """the bool coder's stream over the tokeniser's and the mode-info stage's device buffers, sized from host-known bounds alone"""

    def __init__(self, W, H, tb, mb):
        lib = B.load()
        self.max_bools = int(lib.svt_hip_boolcode_bools_capacity(tb.cap)) + mb.cap
        self.cap = int(lib.svt_hip_boolcode_capacity(self.max_bools))
        self.bytes = torch.full((self.cap + 64,), GUARD8, dtype=torch.uint8, device="cuda")
        self.size = torch.full((1,), 0x77777777, dtype=torch.int32, device="cuda")
        s = B.BoolStream()
        s.d_tokens, s.d_bools, s.d_segments, s.n_segments = tb.tokens.data_ptr(), mb.bools.data_ptr(), mb.segs.data_ptr(), mb.n_seg
        s.d_n_tokens, s.n_tokens, s.max_bools, s.capacity, s.d_bytes, s.d_size = None, 0, self.max_bools, self.cap, self.bytes.data_ptr(), self.size.data_ptr()
        self.struct = s

    def result(self):
        raw, size = self.bytes.cpu().numpy(), int(self.size.cpu().numpy().view(np.uint32)[0])
        return bytes(raw[:min(size, self.cap)]), size, raw[self.cap:]


def chain(ctx, W, H, lf_t, q_t, emap_t):
    """tokeniser -> mode info -> bool coder, enqueued only; every output buffer exists before the first launch"""
    tb, mb = TokBuffers(W, H, counts=False), ModesBuffers(W, H)
    tile = Tile(W, H, tb, mb)
    torch.cuda.synchronize()
    tokenize_device(ctx, W, H, [(lf_t, q_t, emap_t)], [tb])
    modes_device(ctx, W, H, [(lf_t, emap_t, tb.tok_off)], [mb])
    arr = (B.BoolStream * 1)(tile.struct)
    B.check(B.load().svt_hip_boolcode_batch_device(ctx, 1, arr))
    return tb, mb, tile


@pytest.mark.parametrize("name", MM.NAMES)
def test_device_chain_equals_the_reference_tile(ctx, name):
    p = MM.fixture_picture(name)
    W, H = p["W"], p["H"]
    lf_t, q_t, emap_t = upload(p["lf_mi"], p["qcoeff"], p["eob_map"])
    tb, mb, tile = chain(ctx, W, H, lf_t, q_t, emap_t)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(mb.result(), host_of(name))
    got, size, guard = tile.result()
    assert got == p["tile"] and size == len(p["tile"]) and np.all(guard == GUARD8)


def test_chain_behind_the_intra_encode_pass_on_a_searched_grid(ctx):
    """the real producer: the grid of svt_hip_md_intra_search_device, `skip` written by svt_hip_encdec_intra_device"""
    lib = B.load()
    W, H, q_index = 136, 136, 160
    y, u, _ = T.gen_yuv(W, H, 23)
    y, u = y.copy(), u.copy()
    y[48:, 56:], u[24:, 28:] = 97, 140              # a flat corner: its leaves predict exactly and are skipped, beside coded ones
    src = (y, u, (255 - y[1::2, ::2] // 2).astype(np.uint8))
    srcb = dev(np.concatenate([p.ravel() for p in src]))
    nco, n_sb = T.n_sb(W, H) * B.SB_COEFFS, T.n_sb(W, H)
    q_t, dq_t = torch.zeros(nco, dtype=torch.int16, device="cuda"), torch.zeros(nco, dtype=torch.int16, device="cuda")
    rec = M.RefPic(W, H)
    rec_t = dev(rec.buf)
    lf_t = torch.zeros((H // 8) * (W // 8) * 8, dtype=torch.uint8, device="cuda")
    emap_t = torch.full((M.eob_map_offsets(W, H)[3],), 77, dtype=torch.int16, device="cuda")
    lfm_t, nz_t = torch.zeros(n_sb * 160, dtype=torch.uint8, device="cuda"), torch.full(((H // 8) * (W // 8),), 7, dtype=torch.uint8, device="cuda")
    ois_t = torch.zeros(n_sb * B.OIS_PER_SB * 12, dtype=torch.uint8, device="cuda")
    d = B.YuvPlanes()
    d.y, d.u, d.v = srcb.data_ptr(), srcb.data_ptr() + W * H, srcb.data_ptr() + W * H + (W // 2) * (H // 2)
    d.y_stride, d.uv_stride, d.width, d.height = W, W // 2, W, H
    p = B.EncdecPicture()
    p.d_lf_mi, p.src, p.recon = lf_t.data_ptr(), d, rec.desc(rec_t.data_ptr())
    p.d_qcoeff, p.d_dqcoeff, p.d_eob_map, p.d_lfm, p.d_nz = q_t.data_ptr(), dq_t.data_ptr(), emap_t.data_ptr(), lfm_t.data_ptr(), nz_t.data_ptr()
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    ac = lib.svt_hip_vp9_ac_step(q_index)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, 1, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_intra_search_device(ctx, C.byref(d), W, H, C.c_void_p(ois_t.data_ptr())))
        B.check(lib.svt_hip_md_intra_search_device(ctx, C.c_void_p(ois_t.data_ptr()), W, H, C.c_uint32(ac // 2), lib.svt_hip_lf_level_from_q(ac, 1),
                                                   C.c_void_p(lf_t.data_ptr()), W // 8))
        B.check(lib.svt_hip_encdec_intra_device(ctx, work, C.byref(p), W, H, W // 8, q_index, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
        tb, mb, tile = chain(ctx, W, H, lf_t, q_t, emap_t)
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    lf = lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
    q, emap = q_t.cpu().numpy(), emap_t.cpu().numpy().view(np.uint16)
    assert (lf["sb_type"] == 0).any() and (lf["sb_type"] > 0).any() and (lf["skip"] == 0).any() and (lf["skip"] == 1).any()
    tok = TM.host_tokenize_picture(lf, q, emap, W, H, counts=False)
    want = MM.host_modes(lf, emap, tok["tok_off"], W, H)
    assert want["rc"] == 0 and want["n_bools"] != B.MODES_BAD_GRID
    same(mb.result(), want)
    segs = [tuple(int(v) for v in s) for s in want["segments"]]
    want_tile = BM.host_code(tokens=tok["tokens"], bools=want["bools"], segments=segs)[0]
    got, size, guard = tile.result()
    assert got == want_tile and size == len(want_tile) and np.all(guard == GUARD8)
    # and the serial model agrees on the producer's grid
    recs, _ = MM.serial_walk(lf, W, H, MM.tables()[0])
    assert np.array_equal(want["bools"], recs)


def test_capacity_one_short_and_none(ctx):
    name = "sbs_136x136_a"
    p, full = MM.fixture_picture(name), host_of(name)
    W, H = p["W"], p["H"]
    inputs = [upload_fixture(name) for _ in range(3)]
    bufs = [ModesBuffers(W, H, capacity=full["n_bools"] - 1), ModesBuffers(W, H, capacity=0), ModesBuffers(W, H, capacity=full["n_bools"] // 2 + 1)]
    torch.cuda.synchronize()
    modes_device(ctx, W, H, inputs, bufs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    for b in bufs:
        got = b.result()
        assert got["n_bools"] == full["n_bools"] and np.array_equal(got["bools"], full["bools"][:b.cap]) and np.array_equal(got["segments"], full["segments"])
        assert np.all(got["guard"] == GUARD16) and len(got["guard"]) == 64 and np.all(got["seg_guard"] == GUARD32) and np.all(got["n_guard"] == GUARD32)


def test_malformed_grids_answer_the_named_value(ctx):
    """each malformed grid beside a well-formed one in the same batch: the named value, every segment empty, the neighbour untouched"""
    cases = [(what, lf, 64, 64) for what, lf in malformed_grids()] + [("a block crossing the picture edge", edge_crossing_grid(), 72, 40)]
    for W, H in ((64, 64), (72, 40)):
        good_name = "sb64_leaf6" if W == 64 else "edge_72x40_a"
        emap = np.zeros(MM.eob_offsets(W, H)[3], np.int16)
        tok_off = np.full(emap.size, -1, np.int32)
        bad = [(what, lf) for what, lf, w, h in cases if (w, h) == (W, H)]
        inputs = [(dev(np.ascontiguousarray(lf).view(np.uint8)), dev(emap), dev(tok_off)) for _, lf in bad] + [upload_fixture(good_name)]
        torch.cuda.synchronize()
        bufs = modes_device(ctx, W, H, inputs)
        B.check(B.load().svt_hip_ctx_synchronize(ctx))
        for (what, _), b in zip(bad, bufs):
            got = b.result()
            assert got["n_bools"] == B.MODES_BAD_GRID, what
            assert not got["segments"]["count"].any() and np.all(got["guard"] == GUARD16) and np.all(got["seg_guard"] == GUARD32), what
        same(bufs[-1].result(), host_of(good_name))


def test_entry_point_refusals(ctx):
    lib = B.load()
    inputs = [upload_fixture("sb64_leaf6")]
    b = ModesBuffers(64, 64)
    ok = b.struct(*inputs[0])

    def rc(p, n=1, W=64, H=64, stride=8):
        arr = (B.ModesPicture * max(n, 1))(*([p] * max(n, 1)))
        return lib.svt_hip_modes_kf_batch_device(ctx, n, arr, W, H, stride)
    assert rc(ok, 0) != 0 and rc(ok, 33) != 0 and rc(ok, W=60) != 0 and rc(ok, stride=7) != 0
    for field in ("d_lf_mi", "d_eob_map", "d_tok_off", "d_bools", "d_segments", "d_n_bools"):
        p = b.struct(*inputs[0])
        setattr(p, field, None)
        assert rc(p) != 0, field
    p = b.struct(*inputs[0])
    p.d_segments = b.segs.data_ptr() + 4
    assert rc(p) != 0
    fresh = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(fresh), 0))
    try:
        arr = (B.ModesPicture * 1)(ok)
        assert lib.svt_hip_modes_kf_batch_device(fresh, 1, arr, 64, 64, 8) != 0 and b"set_tables" in lib.svt_hip_last_error()
    finally:
        lib.svt_hip_ctx_destroy(fresh)
    torch.cuda.synchronize()
    assert np.all(b.result()["seg_guard"] == GUARD32) and b.result()["n_bools"] == GUARD32          # nothing ran


# ---- past the first pass of the scans, the unit at its ceiling, wider grids ------------------------------------------------------
def upload_grid(lf_mi, eob_map, tok_off):
    return dev(np.ascontiguousarray(lf_mi).view(np.uint8)), dev(np.ascontiguousarray(eob_map).view(np.int16)), dev(np.ascontiguousarray(tok_off).view(np.int32))


def test_big_pictures_in_one_batch_full_and_half_capacity(ctx):
    """289 SBs: two entries a lane in the SB scan, an odd SB count under the batch's % and /, 73 workgroups of the emit kernel a picture, the
    last with one live wave"""
    pics = MM.big_pictures()
    W, H = pics[0]["W"], pics[0]["H"]
    assert T.n_sb(W, H) == 289
    host = [MM.big_host(p["name"]) for p in pics]
    inputs = [upload_grid(p["lf_mi"], p["eob_map"], h["tok"]["tok_off"]) for p, h in zip(pics, host)]
    torch.cuda.synchronize()
    bufs = modes_device(ctx, W, H, inputs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    for b, h in zip(bufs, host):
        same(b.result(), h["modes"])
    half = host[1]["modes"]["n_bools"] // 2
    bufs = [ModesBuffers(W, H), ModesBuffers(W, H, capacity=half)]
    modes_device(ctx, W, H, inputs, bufs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(bufs[0].result(), host[0]["modes"])
    got, want = bufs[1].result(), host[1]["modes"]
    assert got["n_bools"] == want["n_bools"] and np.array_equal(got["bools"], want["bools"][:half]) and np.array_equal(got["segments"], want["segments"])
    assert np.all(got["guard"] == GUARD16) and len(got["guard"]) == 64 and np.all(got["seg_guard"] == GUARD32) and np.all(got["n_guard"] == GUARD32)


def test_worst_unit_on_the_device(ctx):
    """the unit that reaches SVT_MI_UNIT_BOOLS: the wave's part of LDS is sized by it"""
    lf = worst_unit_grid()
    lf["skip"] = 1
    W = H = 64
    emap = np.zeros(MM.eob_offsets(W, H)[3], np.uint16)
    tok_off = np.full(emap.size, 0xFFFFFFFF, np.uint32)
    want = MM.host_modes(lf, emap, tok_off, W, H)
    assert want["rc"] == 0 and want["segments"]["count"][want["segments"]["kind"] == 1].max() == B.MODES_UNIT_BOOLS
    inputs = [upload_grid(lf, emap, tok_off)]
    torch.cuda.synchronize()
    bufs = modes_device(ctx, W, H, inputs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(bufs[0].result(), want)


def test_device_chain_on_the_big_4x4_picture(ctx):
    """tokeniser -> mode info -> bool coder on 294 054 tokens + 527 731 bools: four passes of the bool coder's tile scan, 324 tiles of its carry scan"""
    p, h = MM.big_pictures()[1], MM.big_host("big_4x4")
    assert p["name"] == "big_4x4" and len(h["tok"]["tokens"]) + h["modes"]["n_bools"] > 3 * 256 * 1024 and len(h["tile"]) > 256 * 1024
    W, H = p["W"], p["H"]
    lf_t, q_t, emap_t = upload(p["lf_mi"], p["qcoeff"], p["eob_map"])
    tb, mb, tile = chain(ctx, W, H, lf_t, q_t, emap_t)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(mb.result(), h["modes"])
    got_tok = tb.result()
    assert np.array_equal(got_tok["tokens"], h["tok"]["tokens"]) and np.array_equal(got_tok["tok_off"], h["tok"]["tok_off"]) and np.all(got_tok["guard"] == GUARD32)
    got, size, guard = tile.result()
    assert size == len(h["tile"]) and got == h["tile"] and np.all(guard == GUARD8)


@pytest.mark.parametrize("name", ("edge_72x40_a", "sbs_136x136_a", "big_random"))
def test_wider_grid_equals_the_tight_host_form(ctx, name):
    """mi_stride = mi_cols + 9 with random bytes behind every row of the grid, through the tokeniser and the mode-info stage"""
    if name.startswith("big"):
        p, h = next(p for p in MM.big_pictures() if p["name"] == name), MM.big_host(name)
        tok, want = h["tok"], h["modes"]
    else:
        p, tok = MM.fixture_picture(name), MM.host_tokens(name)
        want = host_of(name)
    W, H = p["W"], p["H"]
    wide = TM.with_stride(p["lf_mi"], 9, 4)
    lf_t, q_t, emap_t = upload(wide, p["qcoeff"], p["eob_map"])
    tb, mb = TokBuffers(W, H, counts=False), ModesBuffers(W, H)
    torch.cuda.synchronize()
    tokenize_device(ctx, W, H, [(lf_t, q_t, emap_t)], [tb], mi_stride=W // 8 + 9)
    modes_device(ctx, W, H, [(lf_t, emap_t, tb.tok_off)], [mb], mi_stride=W // 8 + 9)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    got_tok = tb.result()
    for out in ("tokens", "tok_off", "sb_off"):
        assert np.array_equal(got_tok[out], tok[out]), out
    same(mb.result(), want)

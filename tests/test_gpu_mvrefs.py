"""GPU: the MV-reference stage (csrc/mvrefs.hip) through the C ABI, exactly against what the reference derived
(tests/golden/mvrefs_reference.npz) and the host form (svt_hip_mvrefs_picture): every fixture picture singly, a batch whose pictures
differ in restrict flag, sign biases and ref_mask, wider grids, the 8192x64 and int16-ceiling pictures, a picture of 289 SBs, the chain
tokeniser -> MV references -> inter mode info -> bool coder without a host round trip against the reference's tile bytes, the same chain
behind the mode-decision stand-in and the inter encode pass, malformed grids, optional outputs left out, entry-point refusals, outputs at
the records' own alignment alone and beside aligned ones in one call."""
import ctypes as C

import numpy as np
import pytest
import torch

import boolcode_model as BM
import encdec_model as EM
import modes_inter_model as IM
import mvrefs_model as M
import svt_testlib as T
import tokenize_model as TM
from test_gpu_encdec import DevPicture, dev, flags_of, make_inputs
from test_gpu_modes import GUARD8, Tile
from test_gpu_modes_inter import InterBuffers, modes_device, seeded_ext, upload_grids
from test_gpu_modes_inter import same as same_modes
from test_gpu_tokenize import KEY, TokBuffers, tokenize_device, upload
from test_mvrefs import MALFORMED, stripped

B = T.B
pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    lib, c = B.load(), C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    B.check(lib.svt_hip_boolcode_set_tables(c, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(c, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    yield c
    lib.svt_hip_ctx_destroy(c)


class MvBuffers:
    """device outputs of one picture on a grid of `stride` records a row, each with guard bytes behind it"""

    def __init__(self, W, H, stride=None, want_ext=True, want_cand=True):
        self.rows, self.cols, self.stride = H // 8, W // 8, stride or W // 8
        units = self.rows * self.stride
        self.ext = torch.full((units * 12 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.cand = torch.full((units * 32 + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.status = torch.full((2 + 6,), 0x77777777, dtype=torch.int32, device="cuda")
        self.want_ext, self.want_cand = want_ext, want_cand

    def struct(self, grids, pic, ref_mask=M.ALL_REFS, restrict=None, bias=None):
        """grids: (lf_t, mc_t, ext_t) device tensors"""
        p = B.MvrefsPicture()
        p.d_lf_mi, p.d_mc_mi, p.d_ext, p.d_status = grids[0].data_ptr(), grids[1].data_ptr(), grids[2].data_ptr(), self.status.data_ptr()
        p.d_ext_out, p.d_cand = self.ext.data_ptr() if self.want_ext else None, self.cand.data_ptr() if self.want_cand else None
        M.fill_picture(p, pic, ref_mask, restrict, bias)
        return p

    def result(self):
        eo, ca, st = self.ext.cpu().numpy(), self.cand.cpu().numpy(), self.status.cpu().numpy().view(np.uint32)
        return dict(ext_out=eo[:-GUARD].view(B.MI_INTER_EXT_DTYPE).reshape(self.rows, self.stride)[:, :self.cols], raw_ext=eo, raw_cand=ca,
                    cand=ca[:-GUARD].view(B.MVREF_CAND_DTYPE).reshape(self.rows, self.stride)[:, :self.cols], status=(int(st[0]), int(st[1])),
                    guards=bool((eo[-GUARD:] == 0xA5).all() and (ca[-GUARD:] == 0x5A).all() and (st[2:] == 0x77777777).all()))


def mvrefs_device(ctx, W, H, structs, mi_stride=None):
    """enqueues one svt_hip_mvrefs_batch_device (not synchronised)"""
    arr = (B.MvrefsPicture * len(structs))(*structs)
    B.check(B.load().svt_hip_mvrefs_batch_device(ctx, len(structs), arr, W, H, mi_stride or W // 8))


def same(got, want, ref_mask=M.ALL_REFS):
    """want: a fixture picture (the reference's records) or a host-form result"""
    assert got["guards"] and got["status"] == want["status"]
    assert np.array_equal(got["ext_out"], want["ext_out"])
    assert np.array_equal(got["cand"], M.mask_cand(want["cand"], ref_mask))


def run_single(ctx, p, **kw):
    grids = upload_grids(p)
    b = MvBuffers(p["W"], p["H"], stride=p["lf_mi"].shape[1])
    torch.cuda.synchronize()
    mvrefs_device(ctx, p["W"], p["H"], [b.struct(grids, p, **kw)], mi_stride=p["lf_mi"].shape[1])
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    return b.result()


@pytest.mark.parametrize("name", M.names())
def test_single_picture_equals_the_reference_and_the_host_form(ctx, name):
    """(the 8192x64 pictures, whose clamp bounds exceed int16, and the int16-ceiling pictures are among them)"""
    p = M.fixture_picture(name)
    got = run_single(ctx, p)
    same(got, p)
    same(got, M.host_mvrefs(p))


def test_batch_whose_pictures_differ_in_flag_biases_and_mask(ctx):
    base = M.fixture_picture("mix_136x136_b")
    cases = [(M.fixture_picture("mix_136x136_a"), {}), (base, {}), (M.fixture_picture("mix_136x136_c"), dict(ref_mask=2)),
             (M.fixture_picture("mix_136x136_d"), dict(ref_mask=12)), (base, dict(restrict=1, ref_mask=0)), (base, dict(bias=M.ZERO_BIAS, ref_mask=10)),
             (M.fixture_picture("pert_136x136"), dict(ref_mask=8)), (M.fixture_picture("ceil_136x136"), {})]
    grids = [upload_grids(p) for p, _ in cases]
    bufs = [MvBuffers(136, 136) for _ in cases]
    torch.cuda.synchronize()
    mvrefs_device(ctx, 136, 136, [b.struct(g, p, **kw) for b, g, (p, kw) in zip(bufs, grids, cases)])
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    for b, (p, kw) in zip(bufs, cases):
        want = M.host_mvrefs(p, **kw)
        assert want["rc"] == 0
        same(b.result(), want, kw.get("ref_mask", M.ALL_REFS))
        if set(kw) <= {"ref_mask"}:
            same(b.result(), p, kw.get("ref_mask", M.ALL_REFS))


@pytest.mark.parametrize("name", ("edge_72x40_b", "mix_136x136_d", "wide_8192x64_b", "ceil_8192x64"))
def test_wider_grid_equals_the_tight_result(ctx, name):
    """mi_stride = mi_cols + 9 with random bytes behind every row of the three grids; the outputs' records behind a row stay untouched"""
    p = M.fixture_picture(name)
    got = run_single(ctx, M.with_stride(p, 9, 6))
    same(got, p)
    cols = p["W"] // 8
    for raw, size, fill in ((got["raw_ext"], 12, 0xA5), (got["raw_cand"], 32, 0x5A)):
        assert (raw[:-GUARD].reshape(p["H"] // 8, (cols + 9) * size)[:, cols * size:] == fill).all()


def test_picture_of_289_sbs_equals_the_host_form(ctx):
    """more than one entry per thread of the status kernel and threads with none; an odd SB count under the batch's % and /"""
    p = M.big_picture()
    assert T.n_sb(p["W"], p["H"]) == 289 and p["host"]["rc"] == 0 and p["host"]["status"][0] > 0
    grids = upload_grids(p)
    bufs = [MvBuffers(1080, 1080), MvBuffers(1080, 1080)]
    torch.cuda.synchronize()
    mvrefs_device(ctx, 1080, 1080, [bufs[0].struct(grids, p), bufs[1].struct(grids, p, ref_mask=4, restrict=1)])
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(bufs[0].result(), p["host"])
    same(bufs[1].result(), M.host_mvrefs(p, ref_mask=4, restrict=1), 4)


def chain(ctx, W, H, grids, pic, q_t, emap_t):
    """tokeniser -> MV references -> inter mode info -> bool coder, enqueued only: the inter stage's d_ext is the new stage's d_ext_out;
    every output buffer exists before the first launch"""
    tb, vb, mb = TokBuffers(W, H, counts=False), MvBuffers(W, H, want_cand=False), InterBuffers(W, H)
    tile = Tile(W, H, tb, mb)
    torch.cuda.synchronize()
    tokenize_device(ctx, W, H, [(grids[0], q_t, emap_t)], [tb])
    mvrefs_device(ctx, W, H, [vb.struct(grids, pic, ref_mask=0)])
    modes_device(ctx, W, H, [((grids[0], grids[1], vb.ext), emap_t, tb.tok_off, pic["frame"])], [mb])
    B.check(B.load().svt_hip_boolcode_batch_device(ctx, 1, (B.BoolStream * 1)(tile.struct)))
    return tb, vb, mb, tile


@pytest.mark.parametrize("name", M.names(1))
def test_device_chain_equals_the_reference_tile(ctx, name):
    """the extension records the chain starts from hold ref_frame and the modes only: no host code computed ref_mv_* or mode_context"""
    p = M.fixture_picture(name)
    W, H = p["W"], p["H"]
    _, q_t, emap_t = upload(p["lf_mi"], p["qcoeff"], p["eob_map"])
    tb, vb, mb, tile = chain(ctx, W, H, upload_grids(stripped(p)), p, q_t, emap_t)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    refs = vb.result()
    assert refs["guards"] and refs["status"] == p["status"] and np.array_equal(refs["ext_out"], p["ext_out"])
    got, size, guard = tile.result()
    assert got == p["tile"] and size == len(p["tile"]) and np.all(guard == GUARD8)


def test_chain_behind_the_mode_decision_stand_in_and_the_encode_pass(ctx):
    """the real producers: the grids of svt_hip_md_default_batch_device, `skip`, coefficients and eob map of svt_hip_encdec_batch_device;
    two pictures of one call that differ in restrict flag; against the host chain"""
    lib = B.load()
    W, H, q_index, n = 136, 136, 120, 2
    srcs, refs, me = make_inputs(W, H, n, seed=63)
    frames = [IM.frame(**IM.B_PICTURE), IM.frame(**IM.B_PICTURE)]
    restricts = (0, 1)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    pic, nco = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
    slab_src, slab_pred = torch.zeros(n * pic, dtype=torch.uint8, device="cuda"), torch.zeros(n * pic, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(n * nco, dtype=torch.int16, device="cuda"), torch.zeros(n * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    blank = (np.zeros((H // 8, W // 8), B.MC_MODE_INFO_DTYPE), np.zeros((H // 8, W // 8), B.LF_MODE_INFO_DTYPE))
    dp = [DevPicture(W, H, srcs[i], refs_dev, blank[0], blank[1], slab_src, slab_pred, slab_q, slab_dq, i, EM.RefPic(W, H)) for i in range(n)]
    res_t = [dev(m.view(np.uint8)) for m in me]
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
    torch.cuda.synchronize()
    B.check(lib.svt_hip_md_default_batch_device(ctx, n, ptrs(res_t), W, H, 300, level, ptrs([d.mc_t for d in dp]), ptrs([d.lf_t for d in dp]), W // 8))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    mcs = [d.mc_t.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8) for d in dp]
    exts = [stripped(dict(ext=seeded_ext(mc, fr, 80 + i)))["ext"] for i, (mc, fr) in enumerate(zip(mcs, frames))]
    ext_t = [dev(e.view(np.uint8)) for e in exts]
    arr = (B.EncdecPicture * n)(*[d.struct(refs) for d in dp])
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    tbs, vbs, mbs = [TokBuffers(W, H, counts=False) for _ in dp], [MvBuffers(W, H) for _ in dp], [InterBuffers(W, H) for _ in dp]
    tiles = [Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]
    pics = [dict(W=W, H=H, frame=fr, restrict=rs) for fr, rs in zip(frames, restricts)]
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_encdec_batch_device(ctx, work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), EM.PAD, EM.PAD))
        tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t) for d in dp], tbs)
        mvrefs_device(ctx, W, H, [vb.struct((d.lf_t, d.mc_t, e), p) for vb, d, e, p in zip(vbs, dp, ext_t, pics)])
        modes_device(ctx, W, H, [((d.lf_t, d.mc_t, vb.ext), d.emap_t, tb.tok_off, fr) for d, vb, tb, fr in zip(dp, vbs, tbs, frames)], mbs)
        B.check(lib.svt_hip_boolcode_batch_device(ctx, n, (B.BoolStream * n)(*[t.struct for t in tiles])))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    for d, mc, ext, p, vb, mb, tile in zip(dp, mcs, exts, pics, vbs, mbs, tiles):
        lf = d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
        q, emap = d.q_t.cpu().numpy(), d.emap_t.cpu().numpy().view(np.uint16)
        full = dict(p, lf_mi=lf, mc_mi=mc, ext=ext, qcoeff=q, eob_map=emap)
        want_refs = M.host_mvrefs(full)
        assert want_refs["rc"] == 0 and want_refs["status"][1] > 0 and want_refs["status"][0] != B.MODES_BAD_GRID
        same(vb.result(), want_refs)
        model = M.derive_picture(full)                    # and the serial model agrees on the producers' grids
        assert np.array_equal(want_refs["cand"], model["cand"]) and want_refs["status"] == model["status"]
        tok = TM.host_tokenize_picture(lf, q, emap, W, H, counts=False)
        want = IM.host_modes(dict(full, ext=want_refs["ext_out"]), tok["tok_off"])
        assert want["rc"] == 0 and want["n_bools"] != B.MODES_BAD_GRID
        same_modes(mb.result(), want)
        segs = [tuple(int(v) for v in s) for s in want["segments"]]
        want_tile = BM.host_code(tokens=tok["tokens"], bools=want["bools"], segments=segs)[0]
        got, size, guard = tile.result()
        assert got == want_tile and size == len(want_tile) and np.all(guard == GUARD8)
        assert (lf["skip"] == 0).any() and emap.any()


def test_malformed_grids_answer_the_named_value(ctx):
    """every malformed grid (and the well-formed controls) in batches beside a fixture picture: the named value twice, nothing written
    outside the buffers, the neighbour untouched"""
    for W, H, good_name in ((136, 136, "mix_136x136_a"), (72, 40, "edge_72x40_a")):
        cases = [(what, p, good) for what, p, good in MALFORMED if (p["W"], p["H"]) == (W, H)]
        for k in range(0, len(cases), 24):
            part = cases[k:k + 24]
            pics = [p for _, p, _ in part] + [M.fixture_picture(good_name)]
            grids = [upload_grids(p) for p in pics]
            bufs = [MvBuffers(W, H) for _ in pics]
            torch.cuda.synchronize()
            mvrefs_device(ctx, W, H, [b.struct(g, p) for b, g, p in zip(bufs, grids, pics)])
            B.check(B.load().svt_hip_ctx_synchronize(ctx))
            for (what, p, good), b in zip(part, bufs):
                got = b.result()
                assert got["guards"], what
                if good:
                    same(got, M.host_mvrefs(p))
                    assert got["status"][0] != B.MODES_BAD_GRID, what
                else:
                    assert got["status"] == (B.MODES_BAD_GRID, B.MODES_BAD_GRID), what
            same(bufs[-1].result(), M.fixture_picture(good_name))


def test_optional_outputs_may_be_left_out(ctx):
    p = M.fixture_picture("mix_136x136_b")
    grids = upload_grids(p)
    wants = ((False, True), (True, False), (False, False))
    bufs = [MvBuffers(136, 136, want_ext=e, want_cand=c) for e, c in wants]
    torch.cuda.synchronize()
    mvrefs_device(ctx, 136, 136, [b.struct(grids, p) for b in bufs])
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    for b, (want_ext, want_cand) in zip(bufs, wants):
        got = b.result()
        assert got["guards"] and got["status"] == p["status"]
        assert np.array_equal(got["ext_out"], p["ext_out"]) if want_ext else (got["raw_ext"] == 0xA5).all()
        assert np.array_equal(got["cand"], p["cand"]) if want_cand else (got["raw_cand"] == 0x5A).all()


def test_entry_point_refusals(ctx):
    lib = B.load()
    p = M.fixture_picture("sb64_leaf6_b")
    grids = upload_grids(p)
    b = MvBuffers(64, 64)
    ok = b.struct(grids, p)

    def rc(d, n=1, W=64, H=64, stride=8):
        arr = (B.MvrefsPicture * max(n, 1))(*([d] * max(n, 1)))
        return lib.svt_hip_mvrefs_batch_device(ctx, n, arr, W, H, stride)
    assert rc(ok, 0) != 0 and rc(ok, 33) != 0 and rc(ok, W=60) != 0 and rc(ok, H=8200) != 0 and rc(ok, stride=7) != 0
    assert lib.svt_hip_mvrefs_batch_device(ctx, 1, None, 64, 64, 8) != 0 and lib.svt_hip_mvrefs_batch_device(None, 1, (B.MvrefsPicture * 1)(ok), 64, 64, 8) != 0
    for field in ("d_lf_mi", "d_mc_mi", "d_ext", "d_status"):
        d = b.struct(grids, p)
        setattr(d, field, None)
        assert rc(d) != 0, field
    for mask in (1, 0x10, 0x80, 0xF):
        assert rc(b.struct(grids, p, ref_mask=mask)) != 0, mask
    d = b.struct(grids, p)
    d.d_ext_out = grids[2].data_ptr()
    assert rc(d) != 0
    torch.cuda.synchronize()
    got = b.result()
    assert (got["raw_ext"] == 0xA5).all() and (got["raw_cand"] == 0x5A).all() and got["status"] == (0x77777777, 0x77777777)          # nothing ran


class OffsetOutputs:
    """d_ext_out and d_cand of one tight picture `offset` bytes behind a 16-byte boundary, guard bytes before and behind them"""

    def __init__(self, p, offset):
        self.units, self.offset = (p["H"] // 8) * (p["W"] // 8), offset
        self.ext = torch.full((offset + self.units * 12 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.cand = torch.full((offset + self.units * 32 + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.status = MvBuffers(p["W"], p["H"])

    def struct(self, grids, p, want_ext=True):
        s = self.status.struct(grids, p)
        s.d_ext_out, s.d_cand = self.ext.data_ptr() + self.offset if want_ext else None, self.cand.data_ptr() + self.offset
        assert self.ext.data_ptr() % 16 == 0 and s.d_cand % 16 == self.offset
        return s

    def check(self, want, want_ext=True):
        """want: the host form's result"""
        eo, ca, o = self.ext.cpu().numpy(), self.cand.cpu().numpy(), self.offset
        assert bytes(eo[o:-GUARD]) == want["ext_out"].tobytes() if want_ext else (eo == 0xA5).all()
        assert bytes(ca[o:-GUARD]) == want["cand"].tobytes()
        assert (eo[:o] == 0xA5).all() and (eo[-GUARD:] == 0xA5).all() and (ca[:o] == 0x5A).all() and (ca[-GUARD:] == 0x5A).all()
        assert self.status.result()["status"] == want["status"]


def test_outputs_at_their_own_alignment_only(ctx):
    """d_ext_out at an address that is 2 modulo 4 and d_cand at one that is 2 modulo 16 (the records' own alignment): the 16-bit stores"""
    p = M.fixture_picture("mix_136x136_d")
    grids = upload_grids(p)
    out = OffsetOutputs(p, 2)
    s = out.struct(grids, p)
    assert s.d_ext_out % 4 == 2 and s.d_cand % 16 == 2
    torch.cuda.synchronize()
    mvrefs_device(ctx, 136, 136, [s])
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    want = M.host_mvrefs(p)
    assert want["rc"] == 0 and want["status"][1] > 0
    out.check(want)


def test_store_forms_mixed_in_one_batch(ctx):
    """three pictures of one call: aligned outputs; both outputs at the records' own alignment; d_ext_out left out and d_cand at its own
    alignment -- the store form is chosen per picture inside one launch"""
    p = M.fixture_picture("edge_72x40_b")
    grids = upload_grids(p)
    cases = ((0, True), (2, True), (2, False))
    outs = [OffsetOutputs(p, offset) for offset, _ in cases]
    torch.cuda.synchronize()
    mvrefs_device(ctx, 72, 40, [o.struct(grids, p, want_ext) for o, (_, want_ext) in zip(outs, cases)])
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    want = M.host_mvrefs(p)
    assert want["rc"] == 0 and want["status"][1] > 0
    for o, (_, want_ext) in zip(outs, cases):
        o.check(want, want_ext)

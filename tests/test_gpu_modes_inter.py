"""GPU: the inter mode-info stage (csrc/modeinfo_inter.hip) through the C ABI, exactly against the host form
(svt_hip_modes_inter_picture) and the reference's tile bytes (tests/golden/modes_inter_reference.npz): pictures singly and in batches
whose pictures differ in frame parameters, the chain tokeniser -> inter mode info -> bool coder without a host round trip, the same chain
behind the mode-decision stand-in and the inter encode pass, capacity guard, malformed grids, entry-point refusals; and, against the host
form alone (which test_modes_inter.py pins to the serial model), the unit with the most bools, wider grids and pictures of 289 SBs."""
import ctypes as C

import numpy as np
import pytest
import torch

import boolcode_model as BM
import encdec_model as M
import modes_inter_model as IM
import svt_testlib as T
import tokenize_model as TM
from test_gpu_encdec import DevPicture, dev, flags_of, make_inputs
from test_gpu_modes import GUARD8, GUARD16, GUARD32, Tile
from test_gpu_tokenize import KEY, TokBuffers, tokenize_device, upload
from test_modes_inter import MALFORMED, worst_unit_picture

B = T.B
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib, c = B.load(), C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    B.check(lib.svt_hip_boolcode_set_tables(c, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(c, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    yield c
    lib.svt_hip_ctx_destroy(c)


class InterBuffers:
    """device outputs of one picture, each with guard words behind it; capacity None = svt_hip_modes_inter_bools_capacity"""

    def __init__(self, W, H, capacity=None):
        lib = B.load()
        self.cap = int(lib.svt_hip_modes_inter_bools_capacity(W, H)) if capacity is None else capacity
        self.n_seg = int(lib.svt_hip_modes_segments(W, H))
        self.bools = torch.full((self.cap + 64,), GUARD16, dtype=torch.int16, device="cuda")
        self.segs = torch.full((3 * self.n_seg + 24,), GUARD32, dtype=torch.int32, device="cuda")
        self.n = torch.full((8,), GUARD32, dtype=torch.int32, device="cuda")

    def struct(self, grids, emap_t, tok_off_t, fr):
        """grids: (lf_t, mc_t, ext_t) device tensors"""
        p = B.ModesInterPicture()
        p.d_lf_mi, p.d_mc_mi, p.d_ext, p.d_eob_map, p.d_tok_off = grids[0].data_ptr(), grids[1].data_ptr(), grids[2].data_ptr(), emap_t.data_ptr(), tok_off_t.data_ptr()
        p.d_bools, p.d_segments, p.d_n_bools, p.capacity = self.bools.data_ptr(), self.segs.data_ptr(), self.n.data_ptr(), self.cap
        IM.fill_frame(p, fr)
        return p

    def result(self):
        bools, segs, n = self.bools.cpu().numpy().view(np.uint16), self.segs.cpu().numpy().view(np.uint32), self.n.cpu().numpy().view(np.uint32)
        total = int(n[0])
        got = bools[:min(total, self.cap)].copy() if total != B.MODES_BAD_GRID else np.zeros(0, np.uint16)
        return dict(bools=got, n_bools=total, segments=segs[:3 * self.n_seg].view(B.BOOL_SEGMENT_DTYPE).copy(), guard=bools[self.cap:], seg_guard=segs[3 * self.n_seg:],
                    n_guard=n[1:])


def modes_device(ctx, W, H, inputs, bufs=None, mi_stride=None):
    """inputs: [((lf_t, mc_t, ext_t), emap_t, tok_off_t, frame)].  Enqueues one svt_hip_modes_inter_batch_device; returns the buffers (not yet synchronised)"""
    bufs = bufs or [InterBuffers(W, H) for _ in inputs]
    arr = (B.ModesInterPicture * len(inputs))(*[b.struct(*i) for b, i in zip(bufs, inputs)])
    B.check(B.load().svt_hip_modes_inter_batch_device(ctx, len(inputs), arr, W, H, mi_stride or W // 8))
    return bufs


def same(got, want):
    assert got["n_bools"] == want["n_bools"]
    assert np.array_equal(got["bools"], want["bools"]) and np.array_equal(got["segments"], want["segments"])
    assert np.all(got["guard"] == GUARD16) and np.all(got["seg_guard"] == GUARD32) and np.all(got["n_guard"] == GUARD32)


def upload_grids(p):
    return tuple(dev(np.ascontiguousarray(p[k]).view(np.uint8)) for k in ("lf_mi", "mc_mi", "ext"))


def upload_picture(p, tok_off, fr=None):
    return (upload_grids(p), dev(np.ascontiguousarray(p["eob_map"]).view(np.int16)), dev(np.ascontiguousarray(tok_off).view(np.int32)), fr or p["frame"])


def upload_fixture(name):
    return upload_picture(IM.fixture_picture(name), IM.host_tokens(name)["tok_off"])


@pytest.mark.parametrize("name", IM.NAMES)
def test_single_picture_equals_the_host_form(ctx, name):
    p = IM.fixture_picture(name)
    inputs = [upload_fixture(name)]
    torch.cuda.synchronize()
    bufs = modes_device(ctx, p["W"], p["H"], inputs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(bufs[0].result(), IM.host_of(name))


@pytest.mark.parametrize("size", ((64, 64), (72, 40), (136, 136)))
def test_batch_of_one_geometry_and_differing_frame_parameters(ctx, size):
    """single-reference and REFERENCE_MODE_SELECT pictures (136x136: also one with high-precision MVs) in one call"""
    names = [n for n, W, H, *_ in IM.PICTURES if (W, H) == size]
    assert len({IM.fixture_picture(n)["frame"]["reference_mode"] for n in names}) == 2
    inputs = [upload_fixture(n) for n in names]
    torch.cuda.synchronize()
    bufs = modes_device(ctx, size[0], size[1], inputs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    for n, b in zip(names, bufs):
        same(b.result(), IM.host_of(n))


def chain(ctx, W, H, grids, q_t, emap_t, fr):
    """tokeniser -> inter mode info -> bool coder, enqueued only; every output buffer exists before the first launch"""
    tb, mb = TokBuffers(W, H, counts=False), InterBuffers(W, H)
    tile = Tile(W, H, tb, mb)
    torch.cuda.synchronize()
    tokenize_device(ctx, W, H, [(grids[0], q_t, emap_t)], [tb])
    modes_device(ctx, W, H, [(grids, emap_t, tb.tok_off, fr)], [mb])
    arr = (B.BoolStream * 1)(tile.struct)
    B.check(B.load().svt_hip_boolcode_batch_device(ctx, 1, arr))
    return tb, mb, tile


@pytest.mark.parametrize("name", IM.NAMES)
def test_device_chain_equals_the_reference_tile(ctx, name):
    p = IM.fixture_picture(name)
    W, H = p["W"], p["H"]
    _, q_t, emap_t = upload(p["lf_mi"], p["qcoeff"], p["eob_map"])
    tb, mb, tile = chain(ctx, W, H, upload_grids(p), q_t, emap_t, p["frame"])
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(mb.result(), IM.host_of(name))
    got, size, guard = tile.result()
    assert got == p["tile"] and size == len(p["tile"]) and np.all(guard == GUARD8)


def seeded_ext(mc, fr, seed):
    """extension records for a grid of the mode-decision stand-in: references that agree with its ref_list, a random mode and mode
    context per leaf, reference MVs a random class away from the leaf's MVs"""
    rng = np.random.default_rng(seed)
    ext = np.zeros(mc.shape, B.MI_INTER_EXT_DTYPE)
    for r in range(mc.shape[0]):
        for c in range(mc.shape[1]):
            m = mc[r, c]
            n = int(m["bw8"])
            if r % n or c % n:
                ext[r, c]["ref_frame"] = ext[r - r % n, c - c % n]["ref_frame"]
                continue
            comp = m["ref_list"][1] >= 0
            e = ext[r, c]
            e["ref_frame"] = (IM.LAST if rng.random() < 0.5 else IM.GOLDEN, IM.ALTREF) if comp else ((IM.LAST, IM.GOLDEN)[int(rng.integers(0, 2))] if m["ref_list"][0] == 0 else IM.ALTREF, 0)
            e["mode"], e["mode_context"] = int(rng.choice((10, 11, 12, 13, 13))), int(rng.integers(0, 7))
            for k in range(2):
                d = [IM.mv_component(rng, int(rng.integers(0, 9)), not fr["allow_hp"]) if rng.random() < 0.7 else 0 for _ in range(2)]
                e["ref_mv_row"][k], e["ref_mv_col"][k] = int(m["mv_row"][k]) - d[0], int(m["mv_col"][k]) - d[1]
    return ext


def test_chain_behind_the_mode_decision_stand_in_and_the_encode_pass(ctx):
    """the real producers: the grids of svt_hip_md_default_batch_device, `skip`, coefficients and eob map of svt_hip_encdec_batch_device;
    two pictures of one call, one with high-precision MVs"""
    lib = B.load()
    W, H, q_index, n = 136, 136, 120, 2
    srcs, refs, me = make_inputs(W, H, n, seed=61)
    frames = [IM.frame(**IM.B_PICTURE), IM.frame(allow_hp=1, **IM.B_PICTURE)]
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    pic, nco, mi_n = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS, (H // 8) * (W // 8)
    slab_src, slab_pred = torch.zeros(n * pic, dtype=torch.uint8, device="cuda"), torch.zeros(n * pic, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(n * nco, dtype=torch.int16, device="cuda"), torch.zeros(n * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    blank = (np.zeros((H // 8, W // 8), B.MC_MODE_INFO_DTYPE), np.zeros((H // 8, W // 8), B.LF_MODE_INFO_DTYPE))
    dp = [DevPicture(W, H, srcs[i], refs_dev, blank[0], blank[1], slab_src, slab_pred, slab_q, slab_dq, i, M.RefPic(W, H)) for i in range(n)]
    res_t = [dev(m.view(np.uint8)) for m in me]
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
    torch.cuda.synchronize()
    B.check(lib.svt_hip_md_default_batch_device(ctx, n, ptrs(res_t), W, H, 300, level, ptrs([d.mc_t for d in dp]), ptrs([d.lf_t for d in dp]), W // 8))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    mcs = [d.mc_t.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8) for d in dp]
    exts = [seeded_ext(mc, fr, 70 + i) for i, (mc, fr) in enumerate(zip(mcs, frames))]
    ext_t = [dev(e.view(np.uint8)) for e in exts]
    arr = (B.EncdecPicture * n)(*[d.struct(refs) for d in dp])
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    tbs, mbs = [TokBuffers(W, H, counts=False) for _ in dp], [InterBuffers(W, H) for _ in dp]
    tiles = [Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_encdec_batch_device(ctx, work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
        tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t) for d in dp], tbs)
        modes_device(ctx, W, H, [((d.lf_t, d.mc_t, e), d.emap_t, tb.tok_off, fr) for d, e, tb, fr in zip(dp, ext_t, tbs, frames)], mbs)
        B.check(lib.svt_hip_boolcode_batch_device(ctx, n, (B.BoolStream * n)(*[t.struct for t in tiles])))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    kinds = set()
    for d, mc, ext, fr, mb, tile in zip(dp, mcs, exts, frames, mbs, tiles):
        lf = d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
        q, emap = d.q_t.cpu().numpy(), d.emap_t.cpu().numpy().view(np.uint16)
        p = dict(W=W, H=H, frame=fr, lf_mi=lf, mc_mi=mc, ext=ext, qcoeff=q, eob_map=emap)
        tok = TM.host_tokenize_picture(lf, q, emap, W, H, counts=False)
        want = IM.host_modes(p, tok["tok_off"])
        assert want["rc"] == 0 and want["n_bools"] != B.MODES_BAD_GRID
        same(mb.result(), want)
        segs = [tuple(int(v) for v in s) for s in want["segments"]]
        want_tile = BM.host_code(tokens=tok["tokens"], bools=want["bools"], segments=segs)[0]
        got, size, guard = tile.result()
        assert got == want_tile and size == len(want_tile) and np.all(guard == GUARD8)
        recs, _ = IM.serial_walk(p, IM.tables()[0])          # and the serial model agrees on the producers' grids
        assert np.array_equal(want["bools"], recs)
        kinds |= {int(t) for t in np.unique(lf["sb_type"])}
        assert (lf["skip"] == 0).any() and emap.any()
    assert len(kinds) >= 2


def test_capacity_one_short_and_none(ctx):
    name = "mix_136x136_select"
    p, full = IM.fixture_picture(name), IM.host_of(name)
    W, H = p["W"], p["H"]
    inputs = [upload_fixture(name) for _ in range(3)]
    bufs = [InterBuffers(W, H, capacity=full["n_bools"] - 1), InterBuffers(W, H, capacity=0), InterBuffers(W, H, capacity=full["n_bools"] // 2 + 1)]
    torch.cuda.synchronize()
    modes_device(ctx, W, H, inputs, bufs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    for b in bufs:
        got = b.result()
        assert got["n_bools"] == full["n_bools"] and np.array_equal(got["bools"], full["bools"][:b.cap]) and np.array_equal(got["segments"], full["segments"])
        assert np.all(got["guard"] == GUARD16) and len(got["guard"]) == 64 and np.all(got["seg_guard"] == GUARD32) and np.all(got["n_guard"] == GUARD32)


def test_malformed_grids_answer_the_named_value(ctx):
    """every malformed grid (and the well-formed controls) in batches beside a fixture picture: the named value, every segment empty, the
    neighbour untouched"""
    for W, H, good_name in ((64, 64, "sb64_leaf6"), (72, 40, "edge_72x40_a")):
        cases = []
        for what, p, fr, good in MALFORMED:
            if (p["W"], p["H"]) == (W, H):
                p = dict(p, lf_mi=p["lf_mi"].copy(), eob_map=np.zeros_like(p["eob_map"]))
                p["lf_mi"]["skip"] = 1
                cases.append((what, p, fr or p["frame"], good))
        for k in range(0, len(cases), 24):
            part = cases[k:k + 24]
            inputs = [upload_picture(p, np.full(p["eob_map"].size, 0xFFFFFFFF, np.uint32), fr) for _, p, fr, _ in part] + [upload_fixture(good_name)]
            torch.cuda.synchronize()
            bufs = modes_device(ctx, W, H, inputs)
            B.check(B.load().svt_hip_ctx_synchronize(ctx))
            for (what, p, fr, good), b in zip(part, bufs):
                got = b.result()
                if good:
                    same(got, IM.host_modes(p, np.full(p["eob_map"].size, 0xFFFFFFFF, np.uint32), frame_override=fr))
                    assert got["n_bools"] != B.MODES_BAD_GRID, what
                else:
                    assert got["n_bools"] == B.MODES_BAD_GRID, what
                    assert not got["segments"]["count"].any() and np.all(got["guard"] == GUARD16) and np.all(got["seg_guard"] == GUARD32), what
            same(bufs[-1].result(), IM.host_of(good_name))


def test_entry_point_refusals(ctx):
    lib = B.load()
    inputs = [upload_fixture("sb64_leaf6")]
    b = InterBuffers(64, 64)
    ok = b.struct(*inputs[0])

    def rc(p, n=1, W=64, H=64, stride=8):
        arr = (B.ModesInterPicture * max(n, 1))(*([p] * max(n, 1)))
        return lib.svt_hip_modes_inter_batch_device(ctx, n, arr, W, H, stride)
    assert rc(ok, 0) != 0 and rc(ok, 33) != 0 and rc(ok, W=60) != 0 and rc(ok, stride=7) != 0
    assert lib.svt_hip_modes_inter_batch_device(ctx, 1, None, 64, 64, 8) != 0 and lib.svt_hip_modes_inter_batch_device(None, 1, (B.ModesInterPicture * 1)(ok), 64, 64, 8) != 0
    for field in ("d_lf_mi", "d_mc_mi", "d_ext", "d_eob_map", "d_tok_off", "d_bools", "d_segments", "d_n_bools"):
        p = b.struct(*inputs[0])
        setattr(p, field, None)
        assert rc(p) != 0, field
    p = b.struct(*inputs[0])
    p.d_segments = b.segs.data_ptr() + 4
    assert rc(p) != 0
    p = b.struct(*inputs[0])
    p.d_bools = b.bools.data_ptr() + 2
    assert rc(p) != 0
    p = b.struct(*inputs[0])
    p.reference_mode = 3
    assert rc(p) != 0
    p = b.struct(*inputs[0])
    p.comp_fixed_ref = 0
    assert rc(p) != 0
    fresh = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(fresh), 0))
    try:
        arr = (B.ModesInterPicture * 1)(ok)
        assert lib.svt_hip_modes_inter_batch_device(fresh, 1, arr, 64, 64, 8) != 0 and b"set_tables" in lib.svt_hip_last_error()
    finally:
        lib.svt_hip_ctx_destroy(fresh)
    torch.cuda.synchronize()
    assert np.all(b.result()["seg_guard"] == GUARD32) and b.result()["n_bools"] == GUARD32          # nothing ran


def test_worst_unit_on_the_device(ctx):
    """the unit that reaches SVT_MII_UNIT_BOOLS: the wave's part of LDS is sized by it"""
    p = worst_unit_picture()
    tok_off = np.full(p["eob_map"].size, 0xFFFFFFFF, np.uint32)
    want = IM.host_modes(p, tok_off)
    assert want["rc"] == 0 and want["segments"]["count"][want["segments"]["kind"] == 1].max() == B.MODES_INTER_UNIT_BOOLS
    inputs = [upload_picture(p, tok_off)]
    torch.cuda.synchronize()
    bufs = modes_device(ctx, 64, 64, inputs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(bufs[0].result(), want)


def test_big_pictures_in_one_batch_full_and_half_capacity(ctx):
    """289 SBs: two entries a lane in the SB scan, an odd SB count under the batch's % and /, 145 workgroups of the emit kernel a picture, the
    last with one live wave"""
    pics = IM.big_pictures()
    W, H = pics[0]["W"], pics[0]["H"]
    assert T.n_sb(W, H) == 289
    host = [IM.big_host(p["name"]) for p in pics]
    inputs = [upload_picture(p, h["tok"]["tok_off"]) for p, h in zip(pics, host)]
    torch.cuda.synchronize()
    bufs = modes_device(ctx, W, H, inputs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    for b, h in zip(bufs, host):
        same(b.result(), h["modes"])
    half = host[1]["modes"]["n_bools"] // 2
    bufs = [InterBuffers(W, H), InterBuffers(W, H, capacity=half)]
    modes_device(ctx, W, H, inputs, bufs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    same(bufs[0].result(), host[0]["modes"])
    got, want = bufs[1].result(), host[1]["modes"]
    assert got["n_bools"] == want["n_bools"] and np.array_equal(got["bools"], want["bools"][:half]) and np.array_equal(got["segments"], want["segments"])
    assert np.all(got["guard"] == GUARD16) and len(got["guard"]) == 64 and np.all(got["seg_guard"] == GUARD32) and np.all(got["n_guard"] == GUARD32)


@pytest.mark.parametrize("name", ("edge_72x40_b", "mix_136x136_select", "big_select_hp"))
def test_wider_grid_equals_the_tight_host_form(ctx, name):
    """mi_stride = mi_cols + 9 with random bytes behind every row of the three grids, through the tokeniser and the mode-info stage"""
    if name.startswith("big"):
        p, h = next(p for p in IM.big_pictures() if p["name"] == name), IM.big_host(name)
        tok, want = h["tok"], h["modes"]
    else:
        p, tok, want = IM.fixture_picture(name), IM.host_tokens(name), IM.host_of(name)
    W, H = p["W"], p["H"]
    wide = IM.with_stride(p, 9, 4)
    _, q_t, emap_t = upload(p["lf_mi"], p["qcoeff"], p["eob_map"])
    grids = upload_grids(wide)
    tb, mb = TokBuffers(W, H, counts=False), InterBuffers(W, H)
    torch.cuda.synchronize()
    tokenize_device(ctx, W, H, [(grids[0], q_t, emap_t)], [tb], mi_stride=W // 8 + 9)
    modes_device(ctx, W, H, [(grids, emap_t, tb.tok_off, p["frame"])], [mb], mi_stride=W // 8 + 9)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    got_tok = tb.result()
    for out in ("tokens", "tok_off", "sb_off"):
        assert np.array_equal(got_tok[out], tok[out]), out
    same(mb.result(), want)

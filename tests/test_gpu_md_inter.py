"""GPU: inter mode labelling (csrc/md_inter.hip) through the C ABI, exactly against the host form (svt_hip_md_inter_modes_picture) and
the Python statement of the rule (tests/md_inter_model.py): one SB of each leaf size, partial SBs, 136x72 on grids of 24 records a row
with guard patterns, mixed quad-trees with intra leaves, compound leaves, both restrict flags, sign biases that force the negation, MVs
at the difference bound and odd components with and without the high-precision bit, the constructed cases of the rule's order, a batch
of 32 pictures that differ in every parameter, d_cand left out, a picture of 289 SBs, every refusal, the chain mode-decision
stand-in -> encode pass -> tokeniser -> labelling -> inter mode info -> bool coder -> frame on one stream against the host forms, and
the chain from the tokeniser on against the reference's tiles (tests/golden/md_inter_reference.npz)."""
import ctypes as C

import numpy as np
import pytest
import torch

import boolcode_model as BM
import encdec_model as EM
import frame_model as FM
import md_inter_model as D
import modes_inter_model as IM
import mvrefs_model as M
import svt_testlib as T
import tokenize_model as TM
from test_gpu_encdec import DevPicture, dev, flags_of, make_inputs
from test_gpu_frame import FILL, TABLE_FILL, frame_batch
from test_gpu_modes import GUARD8, Tile
from test_gpu_modes_inter import InterBuffers, modes_device
from test_gpu_modes_inter import same as same_modes
from test_gpu_tokenize import KEY, TokBuffers, tokenize_device, upload
from test_md_inter import MALFORMED, SEEDED, constructed, put, seeded, uniform

B = T.B
pytestmark = pytest.mark.gpu
GUARD = 64
UNTOUCHED = (0x77777777,) * 4


@pytest.fixture(scope="module")
def ctx():
    lib, c = B.load(), C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    B.check(lib.svt_hip_boolcode_set_tables(c, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(c, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    yield c
    lib.svt_hip_ctx_destroy(c)


class MdBuffers:
    """device outputs of one picture on a grid of `stride` records a row, each with guard bytes behind it"""

    def __init__(self, W, H, stride=None, want_cand=True):
        self.rows, self.cols, self.stride = H // 8, W // 8, stride or W // 8
        units = self.rows * self.stride
        self.ext = torch.full((units * 12 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.cand = torch.full((units * 32 + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.status = torch.full((4 + 4,), 0x77777777, dtype=torch.int32, device="cuda")
        self.want_cand = want_cand

    def struct(self, grids, pic, ref_mask=M.ALL_REFS, **over):
        """grids: (lf_t, mc_t) device tensors"""
        p = B.MdInterPicture()
        p.d_lf_mi, p.d_mc_mi, p.d_ext_out, p.d_status = grids[0].data_ptr(), grids[1].data_ptr(), self.ext.data_ptr(), self.status.data_ptr()
        p.d_cand = self.cand.data_ptr() if self.want_cand else None
        D.fill_picture(p, pic, ref_mask, **over)
        return p

    def result(self):
        eo, ca, st = self.ext.cpu().numpy(), self.cand.cpu().numpy(), self.status.cpu().numpy().view(np.uint32)
        return dict(ext_out=eo[:-GUARD].view(B.MI_INTER_EXT_DTYPE).reshape(self.rows, self.stride)[:, :self.cols], raw_ext=eo, raw_cand=ca,
                    cand=ca[:-GUARD].view(B.MVREF_CAND_DTYPE).reshape(self.rows, self.stride)[:, :self.cols], status=tuple(int(v) for v in st[:4]),
                    guards=bool((eo[-GUARD:] == 0xA5).all() and (ca[-GUARD:] == 0x5A).all() and (st[4:] == 0x77777777).all()))


def upload_grids(p):
    return tuple(dev(np.ascontiguousarray(p[k]).view(np.uint8)) for k in ("lf_mi", "mc_mi"))


def md_device(ctx, W, H, structs, mi_stride=None):
    """enqueues one svt_hip_md_inter_modes_batch_device (not synchronised)"""
    arr = (B.MdInterPicture * len(structs))(*structs)
    B.check(B.load().svt_hip_md_inter_modes_batch_device(ctx, len(structs), arr, W, H, mi_stride or W // 8))


def same(got, want, ref_mask=M.ALL_REFS):
    """want: a host-form result or the model's"""
    assert got["guards"] and got["status"] == want["status"]
    assert np.array_equal(got["ext_out"], want["ext_out"])
    assert np.array_equal(got["cand"], M.mask_cand(want["cand"], ref_mask))


def run_batch(ctx, W, H, cases, stride=None):
    """cases: [(picture, keyword arguments of struct)] -> the results"""
    grids = [upload_grids(p) for p, _ in cases]
    bufs = [MdBuffers(W, H, stride=stride, want_cand=kw.get("want_cand", True)) for _, kw in cases]
    torch.cuda.synchronize()
    md_device(ctx, W, H, [b.struct(g, p, **{k: v for k, v in kw.items() if k != "want_cand"}) for b, g, (p, kw) in zip(bufs, grids, cases)], mi_stride=stride)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    return [b.result() for b in bufs]


@pytest.mark.parametrize("name", [n for n, _ in SEEDED])
def test_single_picture_equals_the_host_form_and_the_model(ctx, name):
    """a batch of one: 64x64 of one leaf size each (every mv_ref_blocks row), 72x40 (partial SBs on both edges), 136x72 (candidates across
    SB borders), intra leaves among inter ones, compound leaves, both restrict flags, three sign-bias settings, odd and far MVs"""
    p = seeded(name)
    got = run_batch(ctx, p["W"], p["H"], [(p, {})])[0]
    same(got, D.host_md_inter(p))
    same(got, D.label_picture(p))


def test_136x72_on_a_grid_of_24_records_a_row(ctx):
    """random bytes behind every row of the inputs; the guard pattern behind every row of the outputs survives.  The pictures have leaf
    origins on the first row and column of the SBs below and right of the first, and at the corner unit (8, 8), whose candidates lie in the
    SBs above, left and above-left: the three extra units of the window"""
    for name in ("mix_136x72", "mix_136x72_hp"):
        p = seeded(name)
        want = D.label_picture(p)
        got = run_batch(ctx, 136, 72, [(D.with_stride(p, 7, 11), {})], stride=24)[0]
        same(got, want)
        for raw, size, fill in ((got["raw_ext"], 12, 0xA5), (got["raw_cand"], 32, 0x5A)):
            assert (raw[:-GUARD].reshape(9, 24 * size)[:, 17 * size:] == fill).all()
        origins = want["cand"]["count"][..., 0] != 0xFF
        assert origins[8, 1:].any() and origins[1:8, 8].any() and origins[8, 8] and (want["cand"]["count"][8, 8] > 0).any()


def test_constructed_cases_of_the_order(ctx):
    cases = constructed()
    got = run_batch(ctx, 64, 64, [(p, {}) for _, p, _, _ in cases])
    for (what, p, at, mode), g in zip(cases, got):
        same(g, D.host_md_inter(p))
        assert int(g["ext_out"][at]["mode"]) == mode, what


def test_the_difference_bound_and_the_high_precision_bit(ctx):
    """MVs 16382 .. 16384 from the reference MV on a picture wide enough that the clamp leaves the candidate alone; an odd difference with
    allow_hp 0 and 1 beside a small and beside a large reference MV"""
    cases = []
    for delta in (16383, 16384, 16382, -16382, -16384):
        p = uniform(8192, 64, IM.frame())
        put(p, (0, 0), (0, 100)), put(p, (0, 1), (0, 100 + delta))
        cases.append((p, {}, int(abs(delta) > 16383 or delta & 1)))
    got = run_batch(ctx, 8192, 64, [(p, kw) for p, kw, _ in cases])
    for (p, kw, count), g in zip(cases, got):
        same(g, D.host_md_inter(p, **kw))
        assert g["status"][1] >= 1 and g["status"][2] == count
    cases = []
    for ref, hp, count in (((8, 8), 0, 1), ((8, 8), 1, 0), ((64, 8), 1, 1), ((8, -64), 1, 1), ((63, -63), 1, 0)):
        p = uniform(64, 64, IM.frame())
        put(p, (0, 1), ref), put(p, (1, 1), (ref[0] + 1, ref[1]))
        cases.append((p, dict(allow_hp=hp), count))
    got = run_batch(ctx, 64, 64, [(p, kw) for p, kw, _ in cases])
    for (p, kw, count), g in zip(cases, got):
        same(g, D.host_md_inter(p, **kw))
        assert int(g["ext_out"][1, 1]["mode"]) == 13 and g["status"][2] == count, (kw, count)


def test_batch_of_32_pictures_that_differ_in_every_parameter(ctx):
    pics = [seeded(n) for n in ("mix_136x72", "mix_136x72_hp", "mix_136x72_zero_bias", "mix_136x72_last_golden")]
    cases = []
    for i in range(32):
        p = pics[i % 4]
        kw = dict(ref_mask=(14, 0, 2, 12, 8, 6)[i % 6], restrict_ref_mvs=(i >> 2) & 1, allow_hp=(i >> 3) & 1, want_cand=i % 5 != 0)
        if i % 4 == 0 and i >= 16:
            kw["ref_frame_sign_bias"] = (0, 1, 0, 1)
        cases.append((p, kw))
    got = run_batch(ctx, 136, 72, cases)
    statuses = set()
    for (p, kw), g in zip(cases, got):
        want = D.host_md_inter(p, **kw)
        assert want["rc"] == 0 and g["guards"] and g["status"] == want["status"] and np.array_equal(g["ext_out"], want["ext_out"])
        assert np.array_equal(g["cand"], want["cand"]) if kw["want_cand"] else (g["raw_cand"] == 0x5A).all()
        statuses.add(g["status"])
    assert len(statuses) > 8 and all(s[0] != B.MODES_BAD_GRID for s in statuses)


def test_erased_fixture_grids_in_batches_equal_the_model(ctx):
    by_size = {}
    for name, p in D.fixture_inputs():
        by_size.setdefault((p["W"], p["H"]), []).append(p)
    for (W, H), pics in by_size.items():
        for k in range(0, len(pics), 32):
            for p, g in zip(pics[k:k + 32], run_batch(ctx, W, H, [(p, {}) for p in pics[k:k + 32]])):
                same(g, D.host_md_inter(p))


def test_picture_of_289_sbs_equals_the_host_form(ctx):
    p = D.big_picture()
    assert T.n_sb(p["W"], p["H"]) == 289
    cases = [(p, {}), (p, dict(ref_mask=4, restrict_ref_mvs=1, allow_hp=1))]
    for (_, kw), g in zip(cases, run_batch(ctx, 1080, 1080, cases)):
        want = D.host_md_inter(p, **kw)
        same(g, want, kw.get("ref_mask", M.ALL_REFS))
        assert want["status"][1] > 0 and want["status"][2] > 0


def test_malformed_grids_answer_the_named_value(ctx):
    """every malformed grid in batches beside a well-formed picture: the named value four times, nothing written outside the buffers,
    the neighbour untouched"""
    for W, H, good_name in ((136, 72, "mix_136x72"), (72, 40, "edge_72x40")):
        cases = [(what, p, over) for what, p, over in MALFORMED if (p["W"], p["H"]) == (W, H)]
        good = seeded(good_name)
        for k in range(0, len(cases), 24):
            part = cases[k:k + 24]
            got = run_batch(ctx, W, H, [(p, over) for _, p, over in part] + [(good, {})])
            for (what, _, _), g in zip(part, got):
                assert g["guards"] and g["status"] == D.BAD, what
            same(got[-1], D.host_md_inter(good))


def test_entry_point_refusals(ctx):
    lib = B.load()
    p = seeded("sb64_leaf6")
    grids = upload_grids(p)
    b = MdBuffers(64, 64)
    ok = b.struct(grids, p)

    def rc(d, n=1, W=64, H=64, stride=8):
        arr = (B.MdInterPicture * max(n, 1))(*([d] * max(n, 1)))
        return lib.svt_hip_md_inter_modes_batch_device(ctx, n, arr, W, H, stride)
    assert rc(ok, 0) != 0 and rc(ok, 33) != 0 and rc(ok, W=60) != 0 and rc(ok, H=8200) != 0 and rc(ok, stride=7) != 0
    assert lib.svt_hip_md_inter_modes_batch_device(ctx, 1, None, 64, 64, 8) != 0
    assert lib.svt_hip_md_inter_modes_batch_device(None, 1, (B.MdInterPicture * 1)(ok), 64, 64, 8) != 0
    for field in ("d_lf_mi", "d_mc_mi", "d_ext_out", "d_status"):
        d = b.struct(grids, p)
        setattr(d, field, None)
        assert rc(d) != 0, field
    for mask in (1, 0x10, 0x80, 0xF):
        assert rc(b.struct(grids, p, ref_mask=mask)) != 0, mask
    assert rc(b.struct(grids, p, reference_mode=3)) != 0 and rc(b.struct(grids, p, comp_fixed_ref=0)) != 0 and rc(b.struct(grids, p, comp_var_ref=(1, 4))) != 0
    torch.cuda.synchronize()
    got = b.result()
    assert (got["raw_ext"] == 0xA5).all() and (got["raw_cand"] == 0x5A).all() and got["status"] == UNTOUCHED          # nothing ran


def test_chain_from_the_stand_in_to_the_packets_on_one_stream(ctx):
    """svt_hip_md_default_batch_device -> svt_hip_encdec_batch_device -> tokeniser -> labelling -> inter mode info -> bool coder -> frame,
    two 136x72 pictures that differ in the restrict flag, nothing between the calls; against the same chain on host forms over the
    downloaded grids and coefficients"""
    lib = B.load()
    W, H, q_index, n = 136, 72, 120, 2
    srcs, refs, me = make_inputs(W, H, n, seed=67)
    fr = IM.frame(**IM.B_PICTURE)
    lrf = (IM.LAST, IM.ALTREF)
    fp = FM.inter(width=W, height=H, reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1), base_qindex=q_index)
    head = FM.host_header_bytes(fp)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    pic, nco = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
    slab_src, slab_pred = torch.zeros(n * pic, dtype=torch.uint8, device="cuda"), torch.zeros(n * pic, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(n * nco, dtype=torch.int16, device="cuda"), torch.zeros(n * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    blank = (np.zeros((H // 8, W // 8), B.MC_MODE_INFO_DTYPE), np.zeros((H // 8, W // 8), B.LF_MODE_INFO_DTYPE))
    dp = [DevPicture(W, H, srcs[i], refs_dev, blank[0], blank[1], slab_src, slab_pred, slab_q, slab_dq, i, EM.RefPic(W, H)) for i in range(n)]
    res_t = [dev(m.view(np.uint8)) for m in me]
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
    arr = (B.EncdecPicture * n)(*[d.struct(refs) for d in dp])
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    tbs, vbs, mbs = [TokBuffers(W, H, counts=False) for _ in dp], [MdBuffers(W, H, want_cand=False) for _ in dp], [InterBuffers(W, H) for _ in dp]
    tiles = [Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]
    arena, packets = frame_batch(ctx, tiles, [head] * n)
    pics = [dict(W=W, H=H, frame=fr, restrict=rs, lrf=lrf) for rs in (0, 1)]
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_md_default_batch_device(ctx, n, ptrs(res_t), W, H, 300, level, ptrs([d.mc_t for d in dp]), ptrs([d.lf_t for d in dp]), W // 8))
        B.check(lib.svt_hip_encdec_batch_device(ctx, work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), EM.PAD, EM.PAD))
        tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t) for d in dp], tbs)
        md_device(ctx, W, H, [vb.struct((d.lf_t, d.mc_t), p, ref_mask=0) for vb, d, p in zip(vbs, dp, pics)])
        modes_device(ctx, W, H, [((d.lf_t, d.mc_t, vb.ext), d.emap_t, tb.tok_off, fr) for d, vb, tb in zip(dp, vbs, tbs)], mbs)
        B.check(lib.svt_hip_boolcode_batch_device(ctx, n, (B.BoolStream * n)(*[t.struct for t in tiles])))
        B.check(lib.svt_hip_frame_batch_device(ctx, n, packets, arena.address, arena.cap, arena.table.data_ptr()))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    data, table, front, back, tguard = arena.result()
    at = 0
    for i, (d, p, vb, mb, tile) in enumerate(zip(dp, pics, vbs, mbs, tiles)):
        lf = d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
        mc = d.mc_t.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
        q, emap = d.q_t.cpu().numpy(), d.emap_t.cpu().numpy().view(np.uint16)
        full = dict(p, lf_mi=lf, mc_mi=mc)
        want = D.host_md_inter(full, ref_mask=0, want_cand=False)
        assert want["rc"] == 0 and want["status"][0] > 0 and want["status"][0] != B.MODES_BAD_GRID
        got = vb.result()
        assert got["guards"] and got["status"] == want["status"] and np.array_equal(got["ext_out"], want["ext_out"]) and (got["raw_cand"] == 0x5A).all()
        model = D.label_picture(full, ref_mask=0)           # and the rule as Python states it agrees on the producers' grids
        assert model["status"] == want["status"] and np.array_equal(model["ext_out"], want["ext_out"])
        tok = TM.host_tokenize_picture(lf, q, emap, W, H, counts=False)
        modes = IM.host_modes(dict(full, ext=want["ext_out"], eob_map=emap), tok["tok_off"])
        assert modes["rc"] == 0 and modes["n_bools"] != B.MODES_BAD_GRID
        same_modes(mb.result(), modes)
        want_tile = BM.host_code(tokens=tok["tokens"], bools=modes["bools"], segments=[tuple(int(v) for v in s) for s in modes["segments"]])[0]
        tile_got, size, guard = tile.result()
        assert tile_got == want_tile and size == len(want_tile) and np.all(guard == GUARD8)
        packet = head + want_tile
        assert table[i].tolist() == [at, len(packet)] and bytes(data[at:at + len(packet)]) == packet
        at += len(packet)
        assert (lf["skip"] == 0).any() and emap.any()
    assert table[n].tolist() == [at, 0] and np.all(front == FILL) and np.all(back == FILL) and np.all(tguard == TABLE_FILL) and np.all(data[at:] == FILL)


def chain(ctx, W, H, grids, pic, q_t, emap_t):
    """tokeniser -> labelling -> inter mode info -> bool coder, enqueued only: the inter stage's d_ext is the new stage's d_ext_out; every
    output buffer exists before the first launch.  grids: (lf_t, mc_t).  Returns (the labelling buffers, the tile)"""
    tb, vb, mb = TokBuffers(W, H, counts=False), MdBuffers(W, H, want_cand=False), InterBuffers(W, H)
    tile = Tile(W, H, tb, mb)
    torch.cuda.synchronize()
    tokenize_device(ctx, W, H, [(grids[0], q_t, emap_t)], [tb])
    md_device(ctx, W, H, [vb.struct(grids, pic, ref_mask=0)])
    modes_device(ctx, W, H, [((grids[0], grids[1], vb.ext), emap_t, tb.tok_off, pic["frame"])], [mb])
    B.check(B.load().svt_hip_boolcode_batch_device(ctx, 1, (B.BoolStream * 1)(tile.struct)))
    return vb, tile


@pytest.mark.parametrize("name", [g[0] for g in D.GOLDEN])
def test_device_chain_equals_the_reference_tile(ctx, name):
    """on a picture of tests/golden/md_inter_reference.npz: the records the reference's eb_vp9_find_mv_refs and the four-way comparison
    gave, and the tile the reference wrote for them"""
    p = D.golden_picture(name)
    lf_t, q_t, emap_t = upload(p["lf_mi"], p["qcoeff"], p["eob_map"])
    vb, tile = chain(ctx, p["W"], p["H"], (lf_t, upload_grids(p)[1]), p, q_t, emap_t)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    got = vb.result()
    assert got["guards"] and np.array_equal(got["ext_out"], p["ext"]) and got["status"][2:] == (0, 0)
    tile_got, size, guard = tile.result()
    assert tile_got == p["tile"] and size == len(p["tile"]) and np.all(guard == GUARD8)


def test_outputs_at_their_own_alignment_only(ctx):
    """d_ext_out at an address that is 2 modulo 4 and d_cand at one that is 2 modulo 16 (the records' own alignment): the 16-bit stores"""
    p = seeded("mix_136x72")
    grids = upload_grids(p)
    units = 9 * 17
    ext = torch.full((2 + units * 12 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    cand = torch.full((2 + units * 32 + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    b = MdBuffers(136, 72)
    s = b.struct(grids, p)
    s.d_ext_out, s.d_cand = ext.data_ptr() + 2, cand.data_ptr() + 2
    assert s.d_ext_out % 4 == 2 and s.d_cand % 16 == 2
    torch.cuda.synchronize()
    md_device(ctx, 136, 72, [s])
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    want = D.host_md_inter(p)
    eo, ca = ext.cpu().numpy(), cand.cpu().numpy()
    assert bytes(eo[2:-GUARD]) == want["ext_out"].tobytes() and bytes(ca[2:-GUARD]) == want["cand"].tobytes()
    assert (eo[:2] == 0xA5).all() and (eo[-GUARD:] == 0xA5).all() and (ca[:2] == 0x5A).all() and (ca[-GUARD:] == 0x5A).all()
    assert b.result()["status"] == want["status"]

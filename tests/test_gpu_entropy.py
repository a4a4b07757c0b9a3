"""GPU: the entropy pass (csrc/entropy.hip) through the C ABI -- svt_hip_entropy_batch_device against the reference's bytes (the key frames
of tests/golden/frame_reference.npz, the inter pictures of tests/golden/md_inter_reference.npz as host header || the reference's tile)
and, picture by picture, against the host form svt_hip_entropy_picture (which tests/test_entropy_host.py pins to the same bytes): mixed
batches in both orders, 32 pictures, a grid of 24 records a row, pictures of 289 SBs, the chain behind the encode pass with the packets
read back, a workspace used twice, pictures withheld by every budget and by the grid, refusals.  Every output lies between guard bands."""
import ctypes as C

import numpy as np
import pytest
import torch

import encdec_model as EM
import entropy_model as E
import frame_model as FM
import md_inter_model as D
import modes_inter_model as IM
import mvrefs_model as M
import svt_testlib as T
import tokenize_model as TM
from test_gpu_encdec import DevPicture, dev, flags_of, make_inputs
from test_gpu_frame import FILL, TABLE_FILL, Arena
from test_gpu_tokenize import KEY
from test_md_inter import put, uniform
from test_tile_read_inter import read_frame

B = T.B
pytestmark = pytest.mark.gpu
RES_FILL, CNT_FILL = 0x3C3C3C3C, 0x19191919
KEYS = [w for w in FM.WHOLE if w[1] == "modes"]
SHOW_EXT = b"".join(FM.show_existing(s) for s in (0, 3, 7, 3))


@pytest.fixture(scope="module")
def ctx():
    lib, c = B.load(), C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    tb, tm, ti = E.tables()
    B.check(lib.svt_hip_boolcode_set_tables(c, tb.ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_set_tables(c, tm.ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(c, ti.ctypes.data_as(C.c_void_p)))
    yield c
    lib.svt_hip_ctx_destroy(c)


class Work:
    def __init__(self, ctx, W, H, lim, stride=None):
        self.ctx, self.W, self.H, self.lim, self.stride, self.ptr = ctx, W, H, lim, stride or W // 8, C.c_void_p()
        B.check(B.load().svt_hip_entropy_work_create(ctx, W, H, self.stride, C.byref(lim), C.byref(self.ptr)))

    def buffers(self, pic):
        b = B.EntropyBuffers()
        B.check(B.load().svt_hip_entropy_work_buffers(self.ptr, pic, C.byref(b)))
        return b

    def tile(self, pic, n):
        """the first n bytes of picture pic's tile slot and its size word"""
        b = self.buffers(pic)
        raw, size = np.zeros(n, np.uint8), np.zeros(1, np.uint32)
        lib = B.load()
        B.check(lib.svt_hip_mem_download(self.ctx, raw.ctypes.data_as(C.c_void_p), C.c_void_p(b.d_tile), n))
        B.check(lib.svt_hip_mem_download(self.ctx, size.ctypes.data_as(C.c_void_p), C.c_void_p(b.d_tile_size), 4))
        return bytes(raw), int(size[0])

    def free(self):
        B.load().svt_hip_entropy_work_destroy(self.ctx, self.ptr)


class DevPic:
    """a picture's inputs on the device; d_counts between guards when asked for"""

    def __init__(self, pic, counts=False):
        self.lf = dev(np.ascontiguousarray(pic["lf_mi"]).view(np.uint8))
        self.mc = dev(np.ascontiguousarray(pic["mc_mi"]).view(np.uint8)) if pic.get("mc_mi") is not None else None
        self.q, self.em = dev(np.ascontiguousarray(pic["qcoeff"], np.int16)), dev(np.ascontiguousarray(pic["eob_map"], np.uint16).view(np.int16))
        self.counts = torch.full((8 + B.TOK_COUNTS + 8,), CNT_FILL, dtype=torch.int32, device="cuda") if counts else None

    def ptrs(self):
        return self.lf.data_ptr(), self.mc.data_ptr() if self.mc is not None else None, self.q.data_ptr(), self.em.data_ptr()

    def counts_result(self):
        c = self.counts.cpu().numpy().view(np.uint32)
        return c[8:-8], bool((c[:8] == CNT_FILL).all() and (c[-8:] == CNT_FILL).all())


def struct_of(d, pic, fp, trailer=b""):
    return E.fill_struct(B.EntropyPicture(), d.ptrs(), fp, pic.get("lrf", (1, 3)), pic.get("restrict", 0), trailer, d.counts.data_ptr() + 32 if d.counts is not None else None)


class Call:
    """the outputs of one svt_hip_entropy_batch_device: arena and table (test_gpu_frame.Arena), results between guard words"""

    def __init__(self, ctx, n, capacity):
        self.n, self.arena = n, Arena(ctx, n, capacity)
        self.results = torch.full((8 + 8 * n + 8,), RES_FILL, dtype=torch.int32, device="cuda")

    def enqueue(self, ctx, work, arr, n=None):
        return B.load().svt_hip_entropy_batch_device(ctx, work.ptr, self.n if n is None else n, arr, self.arena.address, self.arena.cap, self.arena.table.data_ptr(),
                                                     self.results.data_ptr() + 32)

    def result(self):
        """(arena bytes, table, result records, every guard intact)"""
        data, table, front, back, tguard = self.arena.result()
        r = self.results.cpu().numpy().view(np.uint32)
        ok = bool(np.all(front == FILL) and np.all(back == FILL) and np.all(tguard == TABLE_FILL) and (r[:8] == RES_FILL).all() and (r[-8:] == RES_FILL).all())
        return data, table, r[8:-8].view(B.ENTROPY_RESULT_DTYPE), ok

    def untouched(self):
        data, table, front, back, tguard = self.arena.result()
        return bool(np.all(data == FILL) and np.all(table == TABLE_FILL) and (self.results.cpu().numpy().view(np.uint32) == RES_FILL).all())


def expected(cases, lim):
    """cases: [(picture, frame parameters, trailer)] -> the host form's answers"""
    return [E.host_entropy(p, fp, lim, trailer=tr) for p, fp, tr in cases]


def check_call(call, want):
    """the arena holds the packets of `want` densely in the caller's order; the table and the results say the same"""
    data, table, res, ok = call.result()
    assert ok
    at, none = 0, 0
    for i, w in enumerate(want):
        assert w["rc"] == 0
        assert {k: int(res[i][k]) for k in res.dtype.names} == w["result"], i
        if w["packet"] is None:
            assert table[i].tolist() == [at, B.FRAME_SIZE_NONE], i
            none += 1
            continue
        assert table[i].tolist() == [at, len(w["packet"])], i
        assert bytes(data[at:at + len(w["packet"])]) == w["packet"], i
        at += len(w["packet"])
    assert table[len(want)].tolist() == [at, none] and np.all(data[at:] == FILL)
    return res


def run(ctx, cases, lim=None, stride=None, counts=False, work=None, slack=64):
    """one call over [(picture, frame parameters, trailer)] under `lim` (default: the worst case), checked against the host form"""
    W, H = cases[0][0]["W"], cases[0][0]["H"]
    lim = lim or E.limits(W, H, len(cases))
    want = expected(cases, lim)
    devs = [DevPic(p, counts) for p, _, _ in cases]
    arr = (B.EntropyPicture * len(cases))(*[struct_of(d, p, fp, tr) for d, (p, fp, tr) in zip(devs, cases)])
    call = Call(ctx, len(cases), sum(len(w["packet"] or b"") for w in want) + slack)
    own = work is None
    work = work or Work(ctx, W, H, lim, stride)
    torch.cuda.synchronize()
    try:
        B.check(call.enqueue(ctx, work, arr))
        B.check(B.load().svt_hip_ctx_synchronize(ctx))
        res = check_call(call, want)
        if counts:
            for d, w in zip(devs, want):
                got, ok = d.counts_result()
                assert ok and int(got.sum()) == w["result"]["tokens"]
    finally:
        if own:
            work.free()
    return want, res, devs


def key_case(w, trailer=b""):
    return E.key_picture(w[2]), w[3], trailer


def inter_case(name, trailer=b"", **fp_over):
    p, fp, _ = E.golden_inter(name)
    return p, dict(fp, **fp_over), trailer


def test_key_pictures_equal_the_reference_frames(ctx):
    """the two 72x40 key pictures in one call: the fixture's whole frames, dense offsets, d_table[2] = {total, 0}"""
    want, res, _ = run(ctx, [key_case(w) for w in KEYS], counts=True)
    frames = [bytes(FM.fixture()[f"frame|{w[0]}"]) for w in KEYS]
    assert [w["packet"] for w in want] == frames and len(frames) == 2
    assert all(int(r["flags"]) == 0 and int(r["inter_leaves"]) == 0 for r in res)


def test_inter_pictures_equal_host_header_and_the_reference_tile(ctx):
    """edge_72x40_select alone; the two 136x72 pictures, which differ in allow_hp, sign biases, restrict and list_ref_frame, in one call"""
    for names in (("edge_72x40_select",), ("mix_136x72_select_hp", "mix_136x72_single_restrict")):
        cases = [inter_case(n) for n in names]
        want, res, _ = run(ctx, cases, counts=True)
        for n, w, r in zip(names, want, res):
            assert w["packet"] == E.golden_inter(n)[2], n
            status = D.host_md_inter(D.golden_picture(n), ref_mask=0, want_cand=False)["status"]
            assert (int(r["inter_leaves"]), int(r["newmv_leaves"]), int(r["unfaithful_leaves"])) == status[:3] and status[2] == 0
    a, b = (D.golden_picture(n) for n in ("mix_136x72_select_hp", "mix_136x72_single_restrict"))
    assert a["frame"]["allow_hp"] != b["frame"]["allow_hp"] and a["frame"]["sign_bias"] != b["frame"]["sign_bias"] and a["restrict"] != b["restrict"] and a["lrf"] != b["lrf"]


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_mixed_batch_of_a_key_and_an_inter_picture(ctx, order):
    """one 72x40 call over a key picture and edge_72x40_select; the inter packet ends in the four show-existing bytes"""
    both = [key_case(KEYS[0]), inter_case("edge_72x40_select", SHOW_EXT)]
    cases = [both[i] for i in order]
    want, _, _ = run(ctx, cases)
    packets = [bytes(FM.fixture()[f"frame|{KEYS[0][0]}"]), E.golden_inter("edge_72x40_select")[2] + SHOW_EXT]
    assert [w["packet"] for w in want] == [packets[i] for i in order]


def full_batch(stride_extra=0):
    """32 pictures of 136x72, key and inter pictures alternating, the inter ones differing in their parameters"""
    inter = [inter_case("mix_136x72_select_hp"), inter_case("mix_136x72_single_restrict", SHOW_EXT[:2])]
    other = D.encoder_like(136, 72, 411, IM.frame(reference_mode=IM.SELECT, sign_bias=M.ALT_BIAS), 1, (IM.LAST, IM.ALTREF), 0.3)
    inter.append((other, E.inter_params(other, base_qindex=33), b""))
    keys = []
    for seed in (5, 6):
        g = IM.make_picture(136, 72, "random", 500 + seed, IM.frame(), 1.0)           # every leaf intra: a key picture's grid
        keys.append((dict(W=136, H=72, lf_mi=g["lf_mi"], mc_mi=None, qcoeff=g["qcoeff"], eob_map=g["eob_map"]), E.key_params(136, 72, base_qindex=40 + seed), SHOW_EXT[:seed - 4]))
    cases = [keys[(i // 2) % 2] if i % 2 == 0 else inter[(i // 2) % 3] for i in range(32)]
    if stride_extra:
        cases = [(dict(p, lf_mi=TM.with_stride(p["lf_mi"], stride_extra, i), mc_mi=TM.with_stride(p["mc_mi"], stride_extra, 40 + i) if p["mc_mi"] is not None else None), fp, tr)
                 for i, (p, fp, tr) in enumerate(cases)]
    return cases


def budget_of(want, n_pics):
    """limits that hold exactly the largest picture of the host form's answers"""
    return dict(max_pics=n_pics, max_tokens=max(w["result"]["tokens"] for w in want), max_bools=max(w["stream_bools"] for w in want),
                max_tile_bytes=max(w["result"]["tile_bytes"] for w in want))


@pytest.mark.parametrize("stride", [17, 24])
def test_full_batch_of_32_pictures_equals_the_host_form(ctx, stride):
    """alternating kinds; on a grid of 24 records a row (mi_stride > width / 8) random bytes lie behind every row of the inputs.  The
    workspace is sized by budgets taken from the host form's counts, as a caller with 32 pictures would size it"""
    cases = full_batch(stride - 17)
    lim = E.limits(136, 72, 32, **budget_of(expected(cases, E.limits(136, 72, 32)), 32))
    want, res, _ = run(ctx, cases, lim, stride=stride)
    assert all(w["packet"] is not None for w in want) and len({w["packet"] for w in want}) >= 5
    assert sum(int(r["inter_leaves"]) > 0 for r in res) == 16


def test_pictures_of_289_sbs_equal_the_host_form(ctx):
    """1080x1080.  The generator of test_gpu_md_inter's large picture has unfaithful and far MVs: it is withheld, and the gate zeroes a list
    of 55 488 vectors in 27 passes of its stride loop.  An encoder-like picture of the same size with coefficients ships: about half a
    million bools, many passes of the bool coder's loops"""
    big = E.zero_coefficients(D.big_picture())
    assert T.n_sb(1080, 1080) == 289
    want, res, _ = run(ctx, [(big, E.inter_params(big), b"")], E.limits(1080, 1080, 1, max_tokens=1024, max_bools=1 << 20, max_tile_bytes=1 << 18))
    assert want[0]["packet"] is None and int(res[0]["flags"]) & (B.ENT_BAD_GRID | B.ENT_UNFAITHFUL_MV) and int(res[0]["unfaithful_leaves"]) > 0
    like = D.encoder_like(1080, 1080, 77, IM.frame(reference_mode=IM.SELECT, sign_bias=M.ALT_BIAS), 0, (IM.LAST, IM.ALTREF), 0.15)
    case = [(like, E.inter_params(like), b"")]
    lim = E.limits(1080, 1080, 1, **budget_of(expected(case, E.limits(1080, 1080, 1)), 1))
    want, res, _ = run(ctx, case, lim)
    assert want[0]["packet"] is not None and want[0]["stream_bools"] > 300000 and int(res[0]["tokens"]) > 30000


def test_behind_the_encode_pass_on_one_stream(ctx):
    """svt_hip_md_default_batch_device -> svt_hip_encdec_batch_device -> svt_hip_entropy_batch_device, two 136x72 B pictures that differ in
    the restrict flag, nothing between the calls: the packets equal the host form over the downloaded grids, and svt_hip_frame_read_host
    returns from them the grids, coefficients and eob map the encode pass held"""
    lib = B.load()
    W, H, q_index, n = 136, 72, 120, 2
    srcs, refs, me = make_inputs(W, H, n, seed=67)
    fr, lrf = IM.frame(**IM.B_PICTURE), (IM.LAST, IM.ALTREF)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    fp = FM.inter(width=W, height=H, reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1), base_qindex=q_index, filter_level=level,
                  frame_parallel_decoding_mode=1)
    assert lib.svt_hip_entropy_deliverable(C.byref(FM.struct(fp))) == 0
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
    metas = [dict(W=W, H=H, frame=fr, restrict=rs, lrf=lrf) for rs in (0, 1)]
    ent = (B.EntropyPicture * n)(*[E.fill_struct(B.EntropyPicture(), (d.lf_t.data_ptr(), d.mc_t.data_ptr(), d.q_t.data_ptr(), d.emap_t.data_ptr()), fp, lrf, m["restrict"])
                                   for d, m in zip(dp, metas)])
    lim = E.limits(W, H, n)
    call = Call(ctx, n, n * (B.FRAME_HEADER_MAX + 40000))
    encdec_work, work = C.c_void_p(), Work(ctx, W, H, lim)
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(encdec_work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_md_default_batch_device(ctx, n, ptrs(res_t), W, H, 300, level, ptrs([d.mc_t for d in dp]), ptrs([d.lf_t for d in dp]), W // 8))
        B.check(lib.svt_hip_encdec_batch_device(ctx, encdec_work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), EM.PAD, EM.PAD))
        B.check(call.enqueue(ctx, work, ent))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, encdec_work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, encdec_work)
        work.free()
    held = [dict(m, lf_mi=d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8), mc_mi=d.mc_t.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8),
                 qcoeff=d.q_t.cpu().numpy(), eob_map=d.emap_t.cpu().numpy().view(np.uint16)) for d, m in zip(dp, metas)]
    want = expected([(p, fp, b"") for p in held], lim)
    check_call(call, want)
    for p, w in zip(held, want):
        assert w["packet"] is not None and w["result"]["inter_leaves"] > 0 and w["result"]["tokens"] > 0
        rc, info, out = read_frame(w["packet"], W, H, restrict=p["restrict"], lrf=lrf)
        assert rc == 0 and out["guards"] and info.needs_backward_adaptation == 0, lib.svt_hip_last_error()
        assert out["lf_mi"].tobytes() == p["lf_mi"].tobytes() and out["mc_mi"].tobytes() == p["mc_mi"].tobytes()
        assert np.array_equal(out["qcoeff"], p["qcoeff"]) and np.array_equal(out["eob_map"], p["eob_map"])
        assert out["ext"].tobytes() == np.ascontiguousarray(D.host_md_inter(p, ref_mask=0, want_cand=False)["ext_out"]).tobytes()


def test_one_workspace_used_twice_with_one_synchronisation(ctx):
    """two calls on one workspace into two arenas, the second enqueued behind the first: both right"""
    first = [inter_case("mix_136x72_select_hp"), inter_case("mix_136x72_single_restrict")]
    second = [first[1], key_case_136(), first[0]]
    lim = E.limits(136, 72, 3)
    work = Work(ctx, 136, 72, lim)
    try:
        calls = []
        for cases in (first, second):
            devs = [DevPic(p) for p, _, _ in cases]
            arr = (B.EntropyPicture * len(cases))(*[struct_of(d, p, fp, tr) for d, (p, fp, tr) in zip(devs, cases)])
            want = expected(cases, lim)
            calls.append((Call(ctx, len(cases), sum(len(w["packet"]) for w in want) + 32), arr, devs, want))
        torch.cuda.synchronize()
        for call, arr, _, _ in calls:
            B.check(call.enqueue(ctx, work, arr))
        B.check(B.load().svt_hip_ctx_synchronize(ctx))
        for call, _, _, want in calls:
            check_call(call, want)
    finally:
        work.free()


def key_case_136():
    g = IM.make_picture(136, 72, "random", 507, IM.frame(), 1.0)
    return dict(W=136, H=72, lf_mi=g["lf_mi"], mc_mi=None, qcoeff=g["qcoeff"], eob_map=g["eob_map"]), E.key_params(136, 72), b""


def three_pictures():
    """three 136x72 inter pictures with coefficients whose token, bool and byte counts all differ"""
    fr = IM.frame(reference_mode=IM.SELECT, sign_bias=M.ALT_BIAS)
    pics = [D.encoder_like(136, 72, 420 + k, fr, k & 1, (IM.LAST, IM.ALTREF), 0.1 + 0.1 * k) for k in range(3)]
    return [(p, E.inter_params(p), b"") for p in pics]


WITHHELD = ("max_tokens", "max_bools", "max_tile_bytes", "sb_type", "odd_newmv")


@pytest.mark.parametrize("what", WITHHELD)
def test_a_withheld_first_picture_leaves_the_other_two_exact(ctx, what):
    """a 3-picture 136x72 batch whose first picture is the bad one (a stray read would stay inside the slab): exactly that flag, no packet,
    d_table[3].size == 1, the other two packets byte-exact and dense; for the reasons phase A finds, the picture's tile slot holds the
    empty stream's bytes -- the segments were emptied in front of the bool coder.  Budgets come from the host form's counts"""
    cases = three_pictures()
    full = expected(cases, E.limits(136, 72, 3))
    assert all(w["packet"] is not None for w in full)
    field = dict(max_tokens=lambda w: w["result"]["tokens"], max_bools=lambda w: w["stream_bools"], max_tile_bytes=lambda w: w["result"]["tile_bytes"])
    flag = dict(max_tokens=B.ENT_TOKENS_OVER, max_bools=B.ENT_STREAM_OVER, max_tile_bytes=B.ENT_TILE_OVER, sb_type=B.ENT_BAD_GRID, odd_newmv=B.ENT_UNFAITHFUL_MV)[what]
    budget = budget_of(full, 3)
    if what in field:
        counts = [field[what](w) for w in full]
        first = int(np.argmax(counts))
        assert sorted(counts)[-1] > sorted(counts)[-2], "one picture holds the most"
        order = [first] + [i for i in range(3) if i != first]
        cases = [cases[i] for i in order]
        budget[what] -= 1
    elif what == "sb_type":
        p = cases[0][0]
        bad = dict(p, lf_mi=p["lf_mi"].copy())
        bad["lf_mi"]["sb_type"][0, 0] = 1                                       # a rectangular block
        cases[0] = (bad, cases[0][1], b"")
    else:
        odd = E.zero_coefficients(uniform(136, 72, IM.frame()))                  # the construction of test_gpu_md_inter's high-precision cases
        put(odd, (0, 1), (8, 8)), put(odd, (1, 1), (9, 8))
        cases[0] = (odd, E.inter_params(odd), b"")
    lim = E.limits(136, 72, 3, **budget)
    work = Work(ctx, 136, 72, lim)
    try:
        want, res, _ = run(ctx, cases, lim, work=work)
        assert [int(r["flags"]) for r in res] == [flag, 0, 0] and want[0]["packet"] is None and want[1]["packet"] and want[2]["packet"]
        assert int(res[0]["tile_bytes"]) == 0
        empty = E.empty_stream_bytes()
        raw, size = work.tile(0, len(empty))
        assert size == B.BOOL_SIZE_OVERFLOW                                     # phase B's mark for the frame stage
        if flag in (B.ENT_TOKENS_OVER, B.ENT_BAD_GRID, B.ENT_UNFAITHFUL_MV):
            assert raw == empty and want[0]["coded_size"] == len(empty)
    finally:
        work.free()


def test_budgets_at_exactly_the_counts_withhold_nothing(ctx):
    cases = three_pictures()
    full = expected(cases, E.limits(136, 72, 3))
    want, res, _ = run(ctx, cases, E.limits(136, 72, 3, **budget_of(full, 3)))
    assert [int(r["flags"]) for r in res] == [0, 0, 0] and [w["packet"] for w in want] == [w["packet"] for w in full]


def test_refusals_launch_nothing(ctx):
    lib = B.load()
    inter, key = inter_case("edge_72x40_select"), key_case(KEYS[0])
    cases = [key, inter]
    devs = [DevPic(p, counts=True) for p, _, _ in cases]
    lim = E.limits(72, 40, 2)
    work, other = Work(ctx, 72, 40, lim), Work(ctx, 136, 72, E.limits(136, 72, 2))
    call = Call(ctx, 2, 4096)
    torch.cuda.synchronize()

    def rc(n=2, c=ctx, w=None, arr=0, arena=0, table=0, results=0, pic=1, fp=None, **change):
        if arr == 0:
            structs = [struct_of(d, p, f, tr) for d, (p, f, tr) in zip(devs, cases)]
            if fp is not None:
                structs[pic].frame = FM.struct(dict(cases[pic][1], **fp))
            for k, v in change.items():
                if k == "lrf":
                    structs[pic].list_ref_frame[0], structs[pic].list_ref_frame[1] = v
                else:
                    setattr(structs[pic], k, v)
            arr = (B.EntropyPicture * 33)(*structs)
        return lib.svt_hip_entropy_batch_device(c, (w or work).ptr if w is not False else None, n, arr, call.arena.address if arena == 0 else arena, call.arena.cap,
                                                call.arena.table.data_ptr() if table == 0 else table, call.results.data_ptr() + 32 if results == 0 else results)
    try:
        assert rc(c=None) == -1 and rc(w=False) == -1 and rc(arr=None) == -1 and rc(arena=None) == -1 and rc(table=None) == -1 and rc(results=None) == -1
        assert rc(n=0) == -1 and rc(n=33) == -1 and rc(n=3) == -1                                   # 3: above the workspace's max_pics
        for f in ("d_lf_mi", "d_qcoeff", "d_eob_map"):
            assert rc(**{f: None}) == -1, f
        assert rc(d_qcoeff=devs[1].q.data_ptr() + 2) == -1
        assert rc(d_mc_mi=None) == -1                                                               # null on an inter picture
        assert rc(pic=0, d_mc_mi=devs[1].mc.data_ptr()) == -1                                       # set on a key picture
        assert rc(trailer_len=5) == -1
        assert rc(fp=dict(color_space=7)) == -1 and rc(fp=dict(uv_dc_delta_q=16)) == -1 and rc(pic=0, fp=dict(filter_level=64)) == -1
        assert rc(lrf=(0, 3)) == -1 and rc(lrf=(1, 4)) == -1
        assert rc(fp=dict(width=64, render_width=64)) == -1 and rc(pic=0, fp=dict(height=48, render_height=48)) == -1
        assert rc(w=other) == -1                                                                    # a workspace of another geometry
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert call.untouched()
        for d in devs:
            assert (d.counts.cpu().numpy().view(np.uint32) == CNT_FILL).all()
        assert rc() == 0
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        check_call(call, expected(cases, lim))
    finally:
        work.free()
        other.free()
    # a context whose tables were never set refuses too, before any launch
    c2 = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c2), 0))
    try:
        w2 = Work(c2, 72, 40, lim)
        call2 = Call(c2, 2, 4096)
        torch.cuda.synchronize()
        arr = (B.EntropyPicture * 2)(*[struct_of(d, p, f, tr) for d, (p, f, tr) in zip(devs, cases)])
        assert call2.enqueue(c2, w2, arr) == -1 and call2.enqueue(ctx, w2, arr) == -1               # and a workspace of another context
        B.check(lib.svt_hip_ctx_synchronize(c2))
        assert call2.untouched()
        w2.free()
    finally:
        lib.svt_hip_ctx_destroy(c2)


def test_arena_table_and_results_in_pinned_host_memory(ctx):
    """d_arena, d_table and d_results in svt_hip_host_alloc memory: after one synchronisation the host reads packets, table and records"""
    lib = B.load()
    cases = [inter_case("mix_136x72_select_hp", SHOW_EXT), key_case_136(), inter_case("mix_136x72_single_restrict")]
    lim = E.limits(136, 72, 3)
    want = expected(cases, lim)
    total = sum(len(w["packet"]) for w in want)
    sizes = (64 + total + 64, 64 + 8 * 4 + 64, 64 + 32 * 3 + 64)                  # arena, table, results: each between 64 guard bytes
    ptrs = [C.c_void_p() for _ in sizes]
    for ptr, n in zip(ptrs, sizes):
        B.check(lib.svt_hip_host_alloc(ctx, n, C.byref(ptr)))
    host = [np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (n,)) for ptr, n in zip(ptrs, sizes)]
    for h in host:
        h[:] = FILL
    devs = [DevPic(p) for p, _, _ in cases]
    arr = (B.EntropyPicture * 3)(*[struct_of(d, p, fp, tr) for d, (p, fp, tr) in zip(devs, cases)])
    work = Work(ctx, 136, 72, lim)
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_entropy_batch_device(ctx, work.ptr, 3, arr, ptrs[0].value + 64, total, ptrs[1].value + 64, ptrs[2].value + 64))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        arena, table, results = (h.copy() for h in host)
    finally:
        work.free()
        for ptr in ptrs:
            lib.svt_hip_host_free(ctx, ptr)
    for a in (arena, table, results):
        assert (a[:64] == FILL).all() and (a[-64:] == FILL).all()
    assert bytes(arena[64:-64]) == b"".join(w["packet"] for w in want)
    tab = table[64:-64].view(np.uint32).reshape(4, 2)
    assert tab[:, 1].tolist() == [len(w["packet"]) for w in want] + [0] and int(tab[3, 0]) == total
    res = results[64:-64].view(B.ENTROPY_RESULT_DTYPE)
    assert [{k: int(r[k]) for k in res.dtype.names} for r in res] == [w["result"] for w in want]


def test_stage_hook_sees_every_stage_in_order(ctx):
    seen = []
    hook = B.ENTROPY_STAGE_HOOK(lambda user, stage: seen.append(stage))
    cases = [key_case(KEYS[0]), inter_case("edge_72x40_select")]
    work = Work(ctx, 72, 40, E.limits(72, 40, 2))
    try:
        B.load().svt_hip_entropy_work_set_stage_hook(work.ptr, hook, None)
        run(ctx, cases, work=work)
    finally:
        work.free()
    assert seen == list(range(len(B.ENT_STAGES)))

"""GPU: the coefficient tokeniser (csrc/tokenize.hip) through the C ABI -- block form against the numpy model and the reference's rate by
the cost identity, picture form against the reference's eb_vp9_tokenize_sb (tests/golden/tokens_reference.npz), batches, capacity
guard, the chain behind the encode pass without a host round trip, scratch reuse across picture sizes; and, against the host form alone
(which test_tokenize.py pins to the model), pictures of 289 SBs, SBs whose every block slot and token is used, wider grids."""
import ctypes as C

import numpy as np
import pytest
import torch

import encdec_model as M
import modes_model as MM
import svt_testlib as T
import tokenize_model as TM
from test_gpu_encdec import DevPicture, _chroma, dev, flags_of, make_inputs, md_host

B = T.B
pytestmark = pytest.mark.gpu
KEY = dict(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=0, loop_filter=1)
GUARD = 0x5A5A5A5A
RATE_KEYS = [k for k in np.load(T.RATE_GOLD).files if k.startswith("bits|")]


def new_ctx():
    c = C.c_void_p()
    B.check(B.load().svt_hip_ctx_create(C.byref(c), 0))
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    B.load().svt_hip_ctx_destroy(c)


class TokBuffers:
    """device outputs of one picture; capacity None = the worst case"""

    def __init__(self, W, H, capacity=None, counts=True):
        self.cap = int(B.load().svt_hip_tokenize_capacity(W, H)) if capacity is None else capacity
        self.tokens = torch.full((self.cap + 64,), GUARD, dtype=torch.int32, device="cuda")
        self.tok_off = torch.full((M.eob_map_offsets(W, H)[3],), 123, dtype=torch.int32, device="cuda")
        self.sb_off = torch.full((T.n_sb(W, H) + 1,), 77, dtype=torch.int32, device="cuda")
        self.counts = torch.full((B.TOK_COUNTS,), 9, dtype=torch.int32, device="cuda") if counts else None

    def struct(self, lf_t, q_t, emap_t):
        p = B.TokPicture()
        p.d_lf_mi, p.d_qcoeff, p.d_eob_map = lf_t.data_ptr(), q_t.data_ptr(), emap_t.data_ptr()
        p.d_tokens, p.capacity, p.d_tok_off, p.d_sb_off = self.tokens.data_ptr(), self.cap, self.tok_off.data_ptr(), self.sb_off.data_ptr()
        p.d_counts = self.counts.data_ptr() if self.counts is not None else None
        return p

    def result(self):
        tokens, sb_off = self.tokens.cpu().numpy().view(np.uint32), self.sb_off.cpu().numpy().view(np.uint32)
        return dict(tokens=tokens[:min(int(sb_off[-1]), self.cap)].copy(), tok_off=self.tok_off.cpu().numpy().view(np.uint32), sb_off=sb_off,
                    counts=self.counts.cpu().numpy().view(np.uint32) if self.counts is not None else None, guard=tokens[self.cap:])


def tokenize_device(ctx, W, H, inputs, bufs=None, mi_stride=None):
    """inputs: [(lf_t, q_t, emap_t)] device tensors.  Enqueues one svt_hip_tokenize_batch_device; returns the buffers (not yet synchronised)"""
    bufs = bufs or [TokBuffers(W, H) for _ in inputs]
    arr = (B.TokPicture * len(inputs))(*[b.struct(*i) for b, i in zip(bufs, inputs)])
    B.check(B.load().svt_hip_tokenize_batch_device(ctx, len(inputs), arr, W, H, mi_stride or W // 8))
    return bufs


def upload(lf_mi, qcoeff, eob_map):
    return dev(np.ascontiguousarray(lf_mi).view(np.uint8)), dev(np.ascontiguousarray(qcoeff, np.int16)), dev(np.ascontiguousarray(eob_map).view(np.int16))


def same(got, want, names=("tokens", "tok_off", "sb_off", "counts")):
    for name in names:
        assert np.array_equal(got[name], want[name]), name
    assert np.all(got["guard"] == GUARD)


# ---- 5. block form ------------------------------------------------------------------------------------------------
def device_blocks(ctx, case, **kw):
    return TM.blocks_call(B.load().svt_hip_tokenize_blocks, case, ctx=ctx, **kw)


@pytest.mark.parametrize("key", RATE_KEYS)
def test_block_form_equals_model_and_reference_rate(ctx, key):
    _, seed, w, h, ext = key.split("|")
    case = T.make_rate_case(int(seed), int(w), int(h), extreme=bool(int(ext)))
    want_bits, tables = np.load(T.RATE_GOLD)[key], T.rate_tables()[0]
    m_tok, m_off, m_cnt = TM.tokenize_blocks(case)
    tok, off, cnt, guard = device_blocks(ctx, case)
    assert np.array_equal(off, m_off) and np.array_equal(tok, m_tok) and np.array_equal(cnt, m_cnt) and np.all(guard == 0xA5A5A5A5)
    assert len(want_bits) == len(case["blocks"])
    for i in range(len(case["blocks"])):
        assert TM.cost_of(tok[int(off[i]):int(off[i + 1])], tables) == int(want_bits[i]), i
    # a second call through the same context: counts are overwritten, not accumulated; a short buffer is not overrun
    tok2, off2, cnt2, guard2 = device_blocks(ctx, case, capacity=len(m_tok) - 3)
    assert np.array_equal(off2, m_off) and np.array_equal(cnt2, m_cnt) and np.array_equal(tok2, m_tok[:-3]) and np.all(guard2 == 0xA5A5A5A5)


def test_block_form_class_boundaries(ctx):
    case, expect = TM.boundary_case()
    tok, off, cnt, _ = device_blocks(ctx, case)
    TM.check_boundary(case, expect, tok, off)
    m_tok, m_off, m_cnt = TM.tokenize_blocks(case)
    assert np.array_equal(tok, m_tok) and np.array_equal(off, m_off) and np.array_equal(cnt, m_cnt)


# ---- 6. picture form against the reference ------------------------------------------------------------------------
def test_picture_form_equals_the_reference(ctx):
    W, H, pics = TM.fixture_pictures()
    inputs = [upload(p["lf_mi"], p["qcoeff"], p["eob_map"]) for p in pics]
    torch.cuda.synchronize()
    bufs = tokenize_device(ctx, W, H, inputs)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    for p, b in zip(pics, bufs):
        got = b.result()
        TM.check_against_fixture(p, got, W, H)
        same(got, TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], W, H))


# ---- 7. batch form ------------------------------------------------------------------------------------------------
def quadtree_grid(seed, W, H, level):
    """inter blocks 64x64 .. 8x8 with zero motion from list 0 (W, H multiples of 64)"""
    rng = np.random.default_rng(seed)
    mc = np.zeros((H // 8, W // 8), dtype=B.MC_MODE_INFO_DTYPE)
    lf = np.zeros((H // 8, W // 8), dtype=B.LF_MODE_INFO_DTYPE)
    mc["ref_list"][..., 1] = -1
    lf["is_inter"], lf["filter_level"] = 1, level

    def split(r, c, n8):
        if n8 > 1 and rng.random() < 0.6:
            for dr in (0, n8 // 2):
                for dc in (0, n8 // 2):
                    split(r + dr, c + dc, n8 // 2)
            return
        lf["sb_type"][r:r + n8, c:c + n8], lf["tx_size"][r:r + n8, c:c + n8] = {1: 3, 2: 6, 4: 9, 8: 12}[n8], {1: 1, 2: 2, 4: 3, 8: 3}[n8]
        mc["bw8"][r:r + n8, c:c + n8] = mc["bh8"][r:r + n8, c:c + n8] = n8
    for r in range(0, H // 8, 8):
        for c in range(0, W // 8, 8):
            split(r, c, 8)
    return mc, lf


def encode_batch(ctx, W, H, srcs, refs, grids, q_index, has_intra=0):
    """svt_hip_encdec_batch_device, enqueued only: (device pictures, workspace)"""
    lib = B.load()
    n, pic, nco = len(srcs), W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
    slab_src, slab_pred = torch.zeros(n * pic, dtype=torch.uint8, device="cuda"), torch.zeros(n * pic, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(n * nco, dtype=torch.int16, device="cuda"), torch.zeros(n * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    dp = [DevPicture(W, H, srcs[i], refs_dev, grids[i][0], grids[i][1], slab_src, slab_pred, slab_q, slab_dq, i, M.RefPic(W, H)) for i in range(n)]
    arr = (B.EncdecPicture * n)(*[d.struct(refs, has_intra=has_intra) for d in dp])
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    torch.cuda.synchronize()
    B.check(lib.svt_hip_encdec_batch_device(ctx, work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
    return dp, work, (slab_src, slab_pred, slab_q, slab_dq, refs_dev)


def downloaded(d, W, H):
    return (d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8), d.q_t.cpu().numpy(), d.emap_t.cpu().numpy().view(np.uint16))


def test_batch_form_all_skip_picture_and_capacity(ctx):
    lib = B.load()
    W, H, q_index = 256, 192, 140
    frames = T.gen_clip_subpel(W, H, 4, 9)
    refs = [M.RefPic(W, H).set_padded(frames[k], *_chroma(frames[k], k)) for k in (0, 3)]
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    grids = [quadtree_grid(40 + i, W, H, level) for i in range(3)]
    # the third picture's source is reference 0 itself: zero motion from list 0 predicts it exactly, so nothing is coded
    srcs = [(frames[1],) + _chroma(frames[1], 1), (frames[0],) + _chroma(frames[0], 0), (frames[2],) + _chroma(frames[2], 2)]
    dp, work, keep = encode_batch(ctx, W, H, srcs, refs, grids, q_index)
    try:
        inputs = [(d.lf_t, d.q_t, d.emap_t) for d in dp]
        bufs = tokenize_device(ctx, W, H, inputs)
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        got = [b.result() for b in bufs]
        host = [TM.host_tokenize_picture(*downloaded(d, W, H), W, H) for d in dp]
        for g, h in zip(got, host):
            same(g, h)
        assert int(got[1]["sb_off"][-1]) == 0 and np.all(got[1]["tok_off"] == TM.NO_OFFSET) and not got[1]["counts"].any() and not got[1]["sb_off"].any()
        totals = [int(g["sb_off"][-1]) for g in got]
        assert totals[0] > 0 and totals[2] > 0
        assert len({int(t) for t in np.unique(downloaded(dp[0], W, H)[0]["sb_type"])}) >= 3
        # again, picture 0 one record short: the total is still reported, nothing lands behind the buffer, the others do not notice
        bufs2 = [TokBuffers(W, H, capacity=totals[0] - 1), TokBuffers(W, H, counts=False), TokBuffers(W, H)]
        tokenize_device(ctx, W, H, inputs, bufs2)
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        got2 = [b.result() for b in bufs2]
        assert int(got2[0]["sb_off"][-1]) == totals[0] and np.all(got2[0]["guard"] == GUARD) and len(got2[0]["guard"]) == 64
        assert np.array_equal(got2[0]["tok_off"], host[0]["tok_off"]) and np.array_equal(got2[0]["sb_off"], host[0]["sb_off"])
        same(got2[1], host[1], names=("tokens", "tok_off", "sb_off"))
        same(got2[2], host[2])
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)


# ---- 8. behind the encode pass, nothing downloaded in between --------------------------------------------------------
def test_chain_behind_the_inter_encode_pass(ctx):
    lib = B.load()
    W, H, q_index = 136, 72, 120
    srcs, refs, me = make_inputs(W, H, 2, seed=77)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    grids = [md_host(m, W, H, 300, level) for m in me]
    dp, work, keep = encode_batch(ctx, W, H, srcs, refs, grids, q_index)
    try:
        bufs = tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t) for d in dp])
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
        for d, b in zip(dp, bufs):
            got = b.result()
            lf, q, emap = downloaded(d, W, H)
            assert emap.any()
            same(got, TM.tokenize_picture(lf, q, emap, W, H))
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)


def test_chain_behind_the_intra_encode_pass_on_a_searched_grid(ctx):
    lib = B.load()
    W, H, q_index = 136, 72, 60
    y, u, _ = T.gen_yuv(W, H, 21)
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
        B.check(lib.svt_hip_md_intra_search_device(ctx, C.c_void_p(ois_t.data_ptr()), W, H, C.c_uint32(ac // 8), lib.svt_hip_lf_level_from_q(ac, 1),
                                                   C.c_void_p(lf_t.data_ptr()), W // 8))
        B.check(lib.svt_hip_encdec_intra_device(ctx, work, C.byref(p), W, H, W // 8, q_index, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
        bufs = tokenize_device(ctx, W, H, [(lf_t, q_t, emap_t)])
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    lf = lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
    assert (lf["sb_type"] == 0).any() and (lf["sb_type"] > 0).any()                  # units of 4x4 blocks occur, and larger blocks
    same(bufs[0].result(), TM.tokenize_picture(lf, q_t.cpu().numpy(), emap_t.cpu().numpy().view(np.uint16), W, H))


# ---- 9. scratch reuse ------------------------------------------------------------------------------------------------
def test_context_reuse_across_picture_sizes(ctx):
    lib = B.load()
    W1, H1, pics = TM.fixture_pictures()
    small = pics[2]
    rng = np.random.default_rng(3)
    W2, H2 = 256, 192
    _, lf2 = quadtree_grid(5, W2, H2, 20)
    # a synthetic larger picture: sparse coefficients, the eob map of their scan order, skip flags as the encode pass would set them
    model_in = synthetic_picture(rng, lf2, W2, H2)

    def run(c, W, H, lf, q, emap):
        inputs = [upload(lf, q, emap)]
        torch.cuda.synchronize()
        bufs = tokenize_device(c, W, H, inputs)
        B.check(lib.svt_hip_ctx_synchronize(c))
        return bufs[0].result()
    seq = [(W1, H1, small["lf_mi"], small["qcoeff"], small["eob_map"]), (W2, H2) + model_in, (W1, H1, small["lf_mi"], small["qcoeff"], small["eob_map"])]
    shared = [run(ctx, *s) for s in seq]
    for s, got in zip(seq, shared):
        fresh_ctx = new_ctx()
        try:
            fresh = run(fresh_ctx, *s)
        finally:
            lib.svt_hip_ctx_destroy(fresh_ctx)
        same(got, fresh)
        same(got, TM.host_tokenize_picture(s[2], s[3], s[4], s[0], s[1]))
    assert int(shared[1]["sb_off"][-1]) > 0


def synthetic_picture(rng, lf, W, H):
    """(lf_mi, qcoeff, eob_map) consistent with each other for an inter grid: random sparse blocks, eob = last non-zero scan position + 1"""
    lf = lf.copy()
    offs, tab = TM.scan_tables()
    q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
    emap = np.zeros(M.eob_map_offsets(W, H)[3], np.uint16)
    lf["skip"] = 0
    coded = np.zeros(lf.shape, bool)
    for b in TM.picture_blocks(lf, emap, W, H):
        n = 16 << (2 * b["ts"])
        if rng.random() < 0.3:
            continue
        k = int(rng.integers(1, min(n, 40) + 1))
        scan = tab[offs[(b["ts"], b["tt"])]:offs[(b["ts"], b["tt"])] + n]
        vals = rng.integers(-70, 71, k)
        vals[-1] = vals[-1] or 1
        q[b["coeff_off"] + scan[:k].astype(np.int64)] = vals
        emap[b["map_index"]] = k
        ur, uc = (b["y4"], b["x4"]) if b["plane"] else (b["y4"] >> 1, b["x4"] >> 1)
        coded[ur, uc] = True
    w8 = np.array([1, 1, 1, 1, 1, 2, 2, 2, 4, 4, 4, 8, 8])[lf["sb_type"]]
    for r in range(lf.shape[0]):
        for c in range(lf.shape[1]):
            n8 = int(w8[r, c])
            r0, c0 = r - r % n8, c - c % n8
            lf["skip"][r, c] = 0 if coded[r0:r0 + n8, c0:c0 + n8].any() else 1
    return lf, q, emap


# ---- 10. past the first pass of the scans, full staging arrays, wider grids ------------------------------------------------------
def run_pictures(ctx, W, H, pics, bufs=None, mi_stride=None):
    """pics: [(lf_mi, qcoeff, eob_map)] host arrays through one batch call -> the results"""
    inputs = [upload(*p) for p in pics]
    torch.cuda.synchronize()
    bufs = tokenize_device(ctx, W, H, inputs, bufs, mi_stride)
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    return [b.result() for b in bufs]


def test_big_pictures_in_one_batch(ctx):
    """289 SBs: two entries a lane in the SB scan (and lanes with none), 37 workgroups of the emit kernel a picture, the last with one SB"""
    pics = MM.big_pictures()
    assert len({(p["W"], p["H"]) for p in pics}) == 1 and T.n_sb(pics[0]["W"], pics[0]["H"]) == 289
    got = run_pictures(ctx, pics[0]["W"], pics[0]["H"], [(p["lf_mi"], p["qcoeff"], p["eob_map"]) for p in pics])
    for p, g in zip(pics, got):
        same(g, MM.big_host(p["name"])["tok"])


@pytest.mark.parametrize("size", sorted({d[:2] for d in MM.DENSE}))
def test_dense_pictures_equal_the_host_form(ctx, size):
    """every SB at 6144 tokens (49 152 in a workgroup's run), 384 block slots for units of 4x4 blocks, one bin of the counts at 32 096"""
    W, H = size
    cases = [d for d in MM.DENSE if d[:2] == size]
    pics = [MM.dense_picture(w, h, t, seed, **kw) for w, h, t, seed, kw in cases]
    host = [TM.host_tokenize_picture(*p, W, H) for p in pics]
    for g, h in zip(run_pictures(ctx, W, H, pics), host):
        assert np.all(np.diff(h["sb_off"].astype(np.int64)) == 6144)
        same(g, h)
    if size == (512, 64):
        assert max(int(h["counts"].max()) for h in host) == 32096


def test_dense_picture_one_record_short(ctx):
    W, H, t, seed, kw = MM.DENSE[0]
    assert t == 0
    pic = MM.dense_picture(W, H, t, seed, **kw)
    full = TM.host_tokenize_picture(*pic, W, H)
    total = int(full["sb_off"][-1])
    assert total == 6144 * 9
    got = run_pictures(ctx, W, H, [pic], [TokBuffers(W, H, capacity=total - 1)])[0]
    assert int(got["sb_off"][-1]) == total and np.all(got["guard"] == GUARD) and len(got["guard"]) == 64
    assert np.array_equal(got["tokens"], full["tokens"][:-1])
    for name in ("tok_off", "sb_off", "counts"):
        assert np.array_equal(got[name], full[name]), name


def test_block_form_above_1024_blocks(ctx):
    """more than 2048 blocks: three entries a lane in the block scan"""
    case = T.make_rate_case(3, 512, 256)
    assert len(case["blocks"]) > 2048
    m_tok, m_off, m_cnt = TM.tokenize_blocks(case)
    tok, off, cnt, guard = device_blocks(ctx, case)
    assert np.array_equal(off, m_off) and np.array_equal(tok, m_tok) and np.array_equal(cnt, m_cnt) and np.all(guard == 0xA5A5A5A5)


@pytest.mark.parametrize("name", ("edge_72x40_a", "sbs_136x136_a", "big_random"))
def test_picture_form_on_a_wider_grid(ctx, name):
    """mi_stride = mi_cols + 9 with random bytes behind every row of the grid: the tight grid's host results"""
    p = MM.fixture_picture(name) if name in MM.NAMES else next(p for p in MM.big_pictures() if p["name"] == name)
    W, H = p["W"], p["H"]
    tight = MM.big_host(name)["tok"] if name.startswith("big") else TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], W, H)
    wide = TM.with_stride(p["lf_mi"], 9, 3)
    assert wide.shape == (H // 8, W // 8 + 9)
    same(run_pictures(ctx, W, H, [(wide, p["qcoeff"], p["eob_map"])], mi_stride=W // 8 + 9)[0], tight)

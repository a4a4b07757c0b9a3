"""GPU: the mixed stand-in decision (svt_hip_md_mixed_batch_device) against its host form, the batched open-loop intra search
(svt_hip_intra_search_batch_device) against the single-picture entry, their refusals, and the whole chain on pictures a decision made:
batched search -> mixed decision -> encode pass -> tokeniser -> labelling -> inter mode info -> bool coder -> frame -> reader -> decode pass.
The host form is pinned to an independent model by tests/test_md_mixed_host.py; the yardsticks of the chain are the oracle chain
(encdec_model) and the encode pass's own buffers.  All comparisons exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import boolcode_model as BM
import encdec_model as M
import frame_model as FM
import intra_search_model as S
import md_mixed_model as X
import me_configs as MC
import modes_inter_model as IM
import svt_testlib as T
from test_gpu_decode_intra import MixedBuffers, mixed_decode, mixed_equal, thresholds
from test_gpu_encdec import DevPicture, _chroma, dev, flags_of, make_inputs
from test_gpu_frame import frame_batch
from test_gpu_intra_search import device_search, picture
from test_gpu_md_inter import MdBuffers, md_device
from test_gpu_modes import Tile
from test_gpu_modes_inter import InterBuffers
from test_gpu_modes_inter import modes_device as inter_modes_device
from test_gpu_tokenize import TokBuffers, tokenize_device
from test_tile_read_inter import read_frame

B = T.B
pytestmark = pytest.mark.gpu
GUARD = 64            # bytes in front of and behind every output
JUNK = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


class MixedRun:
    """device buffers of one call of svt_hip_md_mixed_batch_device: inputs uploaded, every output between guard bytes and filled with 0x33"""

    def __init__(self, inputs, W, H, mi_stride):
        self.W, self.H, self.stride, self.n = W, H, mi_stride, len(inputs)
        self.res_t = [dev(np.ascontiguousarray(me).view(np.uint8).ravel()) for me, _ in inputs]
        self.ois_t = [dev(np.ascontiguousarray(ois).view(np.uint8).ravel()) for _, ois in inputs]
        units = (H // 8) * mi_stride
        self.mc_t = [torch.full((2 * GUARD + units * 12,), 0x33, dtype=torch.uint8, device="cuda") for _ in inputs]
        self.lf_t = [torch.full((2 * GUARD + units * 8,), 0x33, dtype=torch.uint8, device="cuda") for _ in inputs]
        self.cnt_t = torch.full((self.n + 2,), JUNK, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def structs(self):
        arr = (B.MdMixedPicture * self.n)()
        for i in range(self.n):
            arr[i].d_results, arr[i].d_ois = self.res_t[i].data_ptr(), self.ois_t[i].data_ptr()
            arr[i].d_mc_mi, arr[i].d_lf_mi = self.mc_t[i].data_ptr() + GUARD, self.lf_t[i].data_ptr() + GUARD
        return arr

    def call(self, ctx, lam, penalty, level, arr=None, n=None, W=None, H=None, stride=None, counts=True):
        return B.load().svt_hip_md_mixed_batch_device(ctx, self.n if n is None else n, self.structs() if arr is None else arr, self.W if W is None else W,
                                                      self.H if H is None else H, lam, penalty, level, self.stride if stride is None else stride,
                                                      C.c_void_p(self.cnt_t.data_ptr() + 4) if counts else None)

    def result(self, i):
        """(mc grid, lf grid) of picture i, mi_stride wide, after checking its guard bytes"""
        mc, lf = self.mc_t[i].cpu().numpy(), self.lf_t[i].cpu().numpy()
        for a in (mc, lf):
            assert (a[:GUARD] == 0x33).all() and (a[-GUARD:] == 0x33).all(), "guard bytes"
        return (mc[GUARD:-GUARD].view(B.MC_MODE_INFO_DTYPE).reshape(self.H // 8, self.stride), lf[GUARD:-GUARD].view(B.LF_MODE_INFO_DTYPE).reshape(self.H // 8, self.stride))

    def counts(self):
        c = self.cnt_t.cpu().numpy()
        assert c[0] == JUNK and c[-1] == JUNK, "guards of the counters"
        return c[1:-1].tolist()

    def untouched(self):
        return (self.cnt_t.cpu().numpy() == JUNK).all() and all((t.cpu().numpy() == 0x33).all() for t in self.mc_t + self.lf_t)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. device == host form
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(64, 64), (136, 72), (200, 136)])
def test_device_equals_the_host_form(ctx, W, H):
    lam, penalty, level, stride = 150, 300, 21, W // 8 + 3
    inputs = [(X.random_me(10 + i, W, H), S.random_ois(20 + i, W, H)) for i in range(3)]
    inputs[1] = (inputs[1][0], np.ascontiguousarray(inputs[1][1]))
    inputs[1][1]["sad"][:, :84] = S.NONE                                       # picture 1: no intra record anywhere -> no intra leaf, count 0
    run = MixedRun(inputs, W, H, stride)
    B.check(run.call(ctx, lam, penalty, level))
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    counts = run.counts()
    for i, (me, ois) in enumerate(inputs):
        mc_h, lf_h, n_h = X.host(me, ois, W, H, lam, penalty, level, mi_stride=stride, fill=0x33)
        mc_d, lf_d = run.result(i)
        assert lf_d.tobytes() == lf_h.tobytes() and mc_d.tobytes() == mc_h.tobytes(), i      # (the columns beyond the picture stay 0x33 in both)
        assert counts[i] == n_h == int((lf_h["is_inter"][:, :W // 8] == 0).sum()), (i, counts, n_h)
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. more pictures than one launch takes; the counters are zeroed by every call
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_thirty_three_pictures_cross_the_chunk_boundary(ctx):
    W = H = 64
    lam, penalty, level = 100, 200, 9
    inputs = [(X.random_me(100 + i, W, H), S.random_ois(200 + i, W, H)) for i in range(33)]
    want = [X.host(me, ois, W, H, lam, penalty, level) for me, ois in inputs]
    assert len({w[2] for w in want[30:]}) == 3 and want[31][2] > 0 and want[32][2] > 0     # the three pictures at the boundary differ in their counts
    run = MixedRun(inputs, W, H, W // 8)
    for _ in range(2):                                                                       # twice in a row: the counts do not accumulate
        B.check(run.call(ctx, lam, penalty, level))
        B.check(B.load().svt_hip_ctx_synchronize(ctx))
        assert run.counts() == [w[2] for w in want]
    for i in (30, 31, 32):
        mc_d, lf_d = run.result(i)
        assert mc_d.tobytes() == want[i][0].tobytes() and lf_d.tobytes() == want[i][1].tobytes(), i


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. batched search
# ---------------------------------------------------------------------------------------------------------------------------------------
class SearchRun:
    def __init__(self, srcs, stride_pad):
        H, W = srcs[0][0].shape
        self.W, self.H, self.n = W, H, len(srcs)
        ys, cs = W + stride_pad, W // 2 + stride_pad // 2
        self.bufs, self.desc = [], (B.YuvPlanes * self.n)()
        for i, src in enumerate(srcs):
            y = np.full((H, ys), 0xEE, np.uint8); y[:, :W] = src[0]
            u = np.full((H // 2, cs), 0xEE, np.uint8); u[:, :W // 2] = src[1]
            v = np.full((H // 2, cs), 0xEE, np.uint8); v[:, :W // 2] = src[2]
            t = dev(np.concatenate([y.ravel(), u.ravel(), v.ravel()]))
            self.bufs.append(t)
            d = self.desc[i]
            d.y, d.u, d.v, d.y_stride, d.uv_stride, d.width, d.height = t.data_ptr(), t.data_ptr() + y.size, t.data_ptr() + y.size + u.size, ys, cs, W, H
        self.rec_bytes = T.n_sb(W, H) * B.OIS_PER_SB * 12
        self.out_t = [torch.full((2 * GUARD + self.rec_bytes,), 0x5A, dtype=torch.uint8, device="cuda") for _ in srcs]
        torch.cuda.synchronize()

    def outs(self):
        return (C.c_void_p * self.n)(*[t.data_ptr() + GUARD for t in self.out_t])

    def records(self, i):
        a = self.out_t[i].cpu().numpy()
        assert (a[:GUARD] == 0x5A).all() and (a[-GUARD:] == 0x5A).all(), "guard bytes"
        return a[GUARD:-GUARD].view(B.OIS_BLOCK_DTYPE).reshape(T.n_sb(self.W, self.H), B.OIS_PER_SB)

    def untouched(self):
        return all((t.cpu().numpy() == 0x5A).all() for t in self.out_t)


@pytest.mark.parametrize("W,H", [(136, 72), (200, 136)])
def test_batched_search_equals_the_single_picture_entry(ctx, W, H):
    lib = B.load()
    srcs = [picture(W, H, 30 + i) for i in range(3)]
    single = [device_search(ctx, s, 64)[1] for s in srcs]
    assert any((r["sad"][:, 84:] != S.NONE).any() for r in single)
    for with_4x4 in (1, 0):
        run = SearchRun(srcs, 64)
        B.check(lib.svt_hip_intra_search_batch_device(ctx, 3, run.desc, W, H, with_4x4, run.outs()))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        for i in range(3):
            got = run.records(i)
            assert got[:, :84].tobytes() == single[i][:, :84].tobytes(), (with_4x4, i)
            if with_4x4:
                assert got.tobytes() == single[i].tobytes(), i
            else:
                none = np.zeros((), dtype=B.OIS_BLOCK_DTYPE)
                none["sad"], none["uv_sad"], none["mode"], none["uv_mode"] = S.NONE, S.NONE, 0xFF, 0xFF
                assert got[:, 84:].tobytes() == np.full(got[:, 84:].shape, none).tobytes(), i


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. refusals: non-zero, nothing launched, nothing written
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_decision_entry(ctx):
    lib = B.load()
    W, H = 136, 72
    inputs = [(X.random_me(1 + i, W, H), S.random_ois(5 + i, W, H)) for i in range(2)]
    run = MixedRun(inputs, W, H, W // 8)
    bad = B.ERR_BAD_PARAMETER
    assert run.call(None, 10, 20, 5) == bad and run.call(ctx, 10, 20, 5, n=0) == bad and run.call(ctx, 10, 20, 5, counts=False) == bad
    assert lib.svt_hip_md_mixed_batch_device(ctx, 2, None, W, H, 10, 20, 5, W // 8, C.c_void_p(run.cnt_t.data_ptr() + 4)) == bad
    assert run.call(ctx, 10, 20, 5, W=W + 4) == bad and run.call(ctx, 10, 20, 5, H=0) == bad and run.call(ctx, 10, 20, 5, stride=W // 8 - 1) == bad
    assert run.call(ctx, 10, 20, 64) == bad and run.call(ctx, 10, 20, -1) == bad
    for field in ("d_results", "d_ois", "d_mc_mi", "d_lf_mi"):
        arr = run.structs()
        setattr(arr[1], field, None)                                             # the LAST picture: nothing of the first may have run
        assert run.call(ctx, 10, 20, 5, arr=arr) == bad, field
    arr = run.structs()
    arr[1].d_ois += 2
    assert run.call(ctx, 10, 20, 5, arr=arr) == bad                              # records are read as dwords
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert run.untouched()
    B.check(run.call(ctx, 10, 20, 5))                                            # and the same buffers are fine
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert run.counts() == [X.host(me, ois, W, H, 10, 20, 5)[2] for me, ois in inputs]


def test_refusals_of_the_batched_search(ctx):
    lib = B.load()
    W, H = 136, 72
    run = SearchRun([picture(W, H, 3), picture(W, H, 4)], 0)
    bad = B.ERR_BAD_PARAMETER

    def rc(c=ctx, n=2, desc=run.desc, w=W, h=H, w4=0, outs=None):
        return lib.svt_hip_intra_search_batch_device(c, n, desc, w, h, w4, run.outs() if outs is None else outs)
    assert rc(c=None) == bad and rc(n=0) == bad and rc(desc=None) == bad and rc(w=W + 4) == bad and rc(h=4) == bad and rc(w4=2) == bad and rc(w4=-1) == bad
    assert lib.svt_hip_intra_search_batch_device(ctx, 2, run.desc, W, H, 1, None) == bad
    for plane in "yuv":
        saved = getattr(run.desc[1], plane)
        setattr(run.desc[1], plane, None)
        assert rc() == bad, plane
        setattr(run.desc[1], plane, saved)
    run.desc[1].y_stride = W - 1
    assert rc() == bad
    run.desc[1].y_stride = W
    run.desc[1].uv_stride = W // 2 - 1
    assert rc() == bad
    run.desc[1].uv_stride = W // 2
    outs = run.outs()
    outs[1] = None
    assert rc(outs=outs) == bad
    outs = run.outs()
    outs[1] += 2
    assert rc(outs=outs) == bad
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert run.untouched()
    assert rc() == 0
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert not run.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the chain on pictures a decision made
# ---------------------------------------------------------------------------------------------------------------------------------------
CHAIN = dict(W=136, H=72, q_index=120, lam=300, seed=67, region=(slice(0, 72), slice(48, 136)))


@functools.lru_cache(maxsize=None)
def chain_inputs():
    """two B pictures of 136x72 from make_inputs; picture 0's luma holds a region of random row-constant stripes (no reference predicts it, H
    predicts it exactly from the stripe to its left), picture 1 is left alone.  -> sources, references, ME records of the sources as they
    are now, the search model's records, the host form's grids and counts.  CPU only."""
    lib = B.load()
    W, H, lam = CHAIN["W"], CHAIN["H"], CHAIN["lam"]
    srcs, refs, me = make_inputs(W, H, 2, seed=CHAIN["seed"])
    frames = T.gen_clip_subpel(W, H, 4, CHAIN["seed"])                           # (make_inputs' clip: its pictures 0 and 3 are the references)
    y = srcs[0][0].copy()
    rows, cols = CHAIN["region"]
    y[rows, cols] = np.random.default_rng(5).integers(0, 256, (rows.stop - rows.start, 1), dtype=np.uint8)
    srcs = [(y,) + _chroma(y, 1), srcs[1]]
    pics = [T.PaPic(f) for f in (frames[0], frames[3])]
    me = [T.oracle_me_picture_mt(T.PaPic(y), pics[0], pics[1], MC.preset("c2_1080p_m8", 2, 1))[0], me[1]]
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(CHAIN["q_index"]), 0)
    ois = [S.oracle_ois(s) for s in srcs]
    model = [X.model(m, o, W, H, lam, 2 * lam, level) for m, o in zip(me, ois)]
    host = [X.host(m, o, W, H, lam, 2 * lam, level) for m, o in zip(me, ois)]
    return dict(srcs=srcs, refs=refs, me=me, ois=ois, model=model, host=host, level=level)


def intra_leaves(lf):
    """(row, col, size in units) of every intra leaf of a grid"""
    out = []
    for ur, uc in np.argwhere(lf["is_inter"] == 0):
        w8 = {3: 1, 6: 2, 9: 4}[int(lf["sb_type"][ur, uc])]
        if ur % w8 == 0 and uc % w8 == 0:
            out.append((int(ur), int(uc), w8))
    return out


def test_chain_inputs_hold_what_the_chain_test_needs():
    """conditions on the inputs, from the model alone (no device): the striped picture has at least 10 intra leaves of two sizes or more, all
    with mode H where their left neighbour is a stripe; the other picture has none; the host form agrees"""
    c = chain_inputs()
    leaves = intra_leaves(c["model"][0][1])
    assert len(leaves) >= 10 and len({w for _, _, w in leaves}) >= 2, leaves
    assert c["model"][0][2] > 0 and c["model"][1][2] == 0 and (c["model"][1][1]["is_inter"] == 1).all()
    x0 = CHAIN["region"][1].start // 8
    inner = [(r, col, w) for r, col, w in leaves if col > x0]
    assert len(inner) >= 8 and all(int(c["model"][0][1]["pad"][r, col, 1]) == 2 for r, col, w in inner)
    for i in range(2):
        assert c["host"][i][0].tobytes() == c["model"][i][0].tobytes() and c["host"][i][1].tobytes() == c["model"][i][1].tobytes() and c["host"][i][2] == c["model"][i][2]


def test_chain_on_decided_pictures(ctx):
    lib = B.load()
    B.check(lib.svt_hip_boolcode_set_tables(ctx, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(ctx, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    c = chain_inputs()
    W, H, q_index, lam, n = CHAIN["W"], CHAIN["H"], CHAIN["q_index"], CHAIN["lam"], 2
    srcs, refs, level = c["srcs"], c["refs"], c["level"]
    assert len(intra_leaves(c["model"][0][1])) >= 10 and c["model"][1][2] == 0                      # (established on the CPU, see above)
    fr, lrf = IM.frame(**IM.B_PICTURE), (IM.LAST, IM.ALTREF)
    fp = FM.inter(width=W, height=H, reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1), base_qindex=q_index, filter_level=level,
                  frame_parallel_decoding_mode=1)
    head = FM.host_header_bytes(fp)
    pic, nco = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
    slab_src, slab_pred = torch.zeros(n * pic, dtype=torch.uint8, device="cuda"), torch.zeros(n * pic, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(n * nco, dtype=torch.int16, device="cuda"), torch.zeros(n * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    junk_mc, junk_lf = np.full((H // 8, W // 8 * 12), 0x33, np.uint8).view(B.MC_MODE_INFO_DTYPE), np.full((H // 8, W // 8 * 8), 0x33, np.uint8).view(B.LF_MODE_INFO_DTYPE)
    dp = [DevPicture(W, H, srcs[i], refs_dev, junk_mc, junk_lf, slab_src, slab_pred, slab_q, slab_dq, i, M.RefPic(W, H)) for i in range(n)]
    res_t = [dev(np.ascontiguousarray(m).view(np.uint8).ravel()) for m in c["me"]]
    ois_t = [torch.full((T.n_sb(W, H) * B.OIS_PER_SB * 12,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(n)]
    cnt_t = torch.full((n,), JUNK, dtype=torch.int32, device="cuda")
    src_desc = (B.YuvPlanes * n)(*[d.tight(d.src_t.data_ptr(), W) for d in dp])
    md = (B.MdMixedPicture * n)()
    for i, d in enumerate(dp):
        md[i].d_results, md[i].d_ois, md[i].d_mc_mi, md[i].d_lf_mi = res_t[i].data_ptr(), ois_t[i].data_ptr(), d.mc_t.data_ptr(), d.lf_t.data_ptr()
    flags, thr = flags_of(**dict(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=1, loop_filter=1)), thresholds()
    tbs, vbs, mbs = [TokBuffers(W, H, counts=False) for _ in dp], [MdBuffers(W, H, want_cand=False) for _ in dp], [InterBuffers(W, H) for _ in dp]
    tiles = [Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]
    arena, packets = frame_batch(ctx, tiles, [head] * n)
    metas = [dict(W=W, H=H, frame=fr, restrict=rs, lrf=lrf) for rs in (0, 1)]
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        # the decision, on the stream
        B.check(lib.svt_hip_intra_search_batch_device(ctx, n, src_desc, W, H, 0, (C.c_void_p * n)(*[t.data_ptr() for t in ois_t])))
        B.check(lib.svt_hip_md_mixed_batch_device(ctx, n, md, W, H, lam, 2 * lam, level, W // 8, C.c_void_p(cnt_t.data_ptr())))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        counts = cnt_t.cpu().numpy().tolist()                                    # (the caller's wait for the counts)
        assert counts == [c["host"][0][2], 0]
        for i, d in enumerate(dp):                                               # the device's records and grids are the model's / the host form's
            got = ois_t[i].cpu().numpy().view(B.OIS_BLOCK_DTYPE).reshape(-1, B.OIS_PER_SB)
            assert got[:, :84].tobytes() == c["ois"][i][:, :84].tobytes(), i
            assert d.mc_t.cpu().numpy().tobytes() == c["host"][i][0].tobytes() and d.lf_t.cpu().numpy().tobytes() == c["host"][i][1].tobytes(), i
        arr = (B.EncdecPicture * n)(*[d.struct(refs, has_intra=int(counts[i] > 0)) for i, d in enumerate(dp)])
        # everything behind it
        B.check(lib.svt_hip_encdec_batch_device(ctx, work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
        tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t) for d in dp], tbs)
        md_device(ctx, W, H, [vb.struct((d.lf_t, d.mc_t), m, ref_mask=0) for vb, d, m in zip(vbs, dp, metas)])
        inter_modes_device(ctx, W, H, [((d.lf_t, d.mc_t, vb.ext), d.emap_t, tb.tok_off, fr) for d, vb, tb in zip(dp, vbs, tbs)], mbs)
        B.check(lib.svt_hip_boolcode_batch_device(ctx, n, (B.BoolStream * n)(*[t.struct for t in tiles])))
        B.check(lib.svt_hip_frame_batch_device(ctx, n, packets, arena.address, arena.cap, arena.table.data_ptr()))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        cnt = (C.c_int32 * 8)()
        assert lib.svt_hip_encdec_work_status(ctx, work, cnt) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    data, table, _, _, _ = arena.result()
    pics = []
    for i, (d, vb, m) in enumerate(zip(dp, vbs, metas)):
        got = vb.result()
        assert got["guards"] and got["status"][2] == 0, got["status"]           # no leaf the labelling could not code faithfully
        g = dict(lf=d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8), mc=d.mc_t.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8),
                 q=d.q_t.cpu().numpy(), emap=d.emap_t.cpu().numpy().view(np.uint16), pred=d.pred_t.cpu().numpy(), rec=d.rec_t.cpu().numpy(),
                 lfm=d.lfm_t.cpu().numpy().view(B.LF_MASK_DTYPE))
        # encode side: the oracle chain on the host form's grids
        o = M.oracle_encdec_picture(srcs[i], refs, c["host"][i][0], c["host"][i][1], q_index, flags, thr, recon_init=M.RefPic(W, H))
        assert np.array_equal(g["pred"], np.concatenate([p.ravel() for p in o["pred"]])), "prediction"
        assert np.array_equal(g["q"], o["qcoeff"]) and np.array_equal(g["emap"], o["eob_map"]), "coefficients"
        assert g["lf"].tobytes() == o["lf_mi"].tobytes(), "grid with its skip flags"
        assert np.array_equal(g["rec"], o["rec"].buf), ("reconstruction", int(np.sum(g["rec"] != o["rec"].buf)))
        # read-back side: the packet's grids, modes and coefficients
        off, size = (int(v) for v in table[i])
        packet = bytes(data[off:off + size])
        assert packet[:len(head)] == head and size > len(head)
        rc, info, r = read_frame(packet, W, H, restrict=m["restrict"], lrf=lrf)
        assert rc == 0, lib.svt_hip_last_error()
        assert r["guards"] and r["res"]["past_end"] == 0
        assert (r["res"]["inter_leaves"] < r["res"]["leaves"]) == (i == 0)
        assert r["lf_mi"].tobytes() == g["lf"].tobytes(), [f for f in g["lf"].dtype.names if not np.array_equal(r["lf_mi"][f], g["lf"][f])]
        inter = g["lf"]["is_inter"] == 1
        for f in g["mc"].dtype.names:
            assert np.array_equal(r["mc_mi"][f][inter], g["mc"][f][inter]), f
        assert np.array_equal(r["qcoeff"], g["q"]) and np.array_equal(r["eob_map"], g["emap"])
        pics.append(dict(g, lf=np.ascontiguousarray(r["lf_mi"]), mc=np.ascontiguousarray(r["mc_mi"]), q=np.ascontiguousarray(r["qcoeff"]),
                         emap=np.ascontiguousarray(r["eob_map"]), has_intra=int(i == 0)))
    enc = dict(W=W, H=H, q_index=q_index, flags=flags, thr=thr, refs=refs, refs_dev=refs_dev, pics=pics, counts=list(cnt))
    bufs = MixedBuffers(enc)
    rc, got_cnt = mixed_decode(ctx, enc, bufs, bufs.structs(enc))
    assert rc == 0 and got_cnt == enc["counts"]
    mixed_equal(enc, bufs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. through the public API
# ---------------------------------------------------------------------------------------------------------------------------------------
import test_enc_shim_encdec as E  # noqa: E402  (its helpers: run_clip, structure, chroma, stand_in)

API = dict(W=256, H=192, N=18, enc_mode=8, tune=1, qp=40, intra_period=-1, striped=(3, 7, 11, 13))


@functools.lru_cache(maxsize=None)
def api_frames():
    """the clip of the shim tests; four pictures of the deepest layer (no picture predicts from them) carry a region of random row-constant
    stripes of their own"""
    W, H = API["W"], API["H"]
    frames = [f.copy() for f in T.gen_clip_subpel(W, H, API["N"], 41)]
    for k in API["striped"]:
        x0 = 64 + 8 * (k % 5)
        frames[k][24:152, x0:x0 + 120] = np.random.default_rng(700 + k).integers(0, 256, (128, 1), dtype=np.uint8)
    return tuple(frames)


def mixed_stand_in(me, ois, W, H, lam, level):
    """the library's mixed stand-in from the host form: svt_hip_md_mixed_picture on the search model's records with intra_penalty = 2 lambda"""
    return X.host(me, ois, W, H, lam, 2 * lam, level)


@functools.lru_cache(maxsize=None)
def oracle_clip_mixed():
    """E.oracle_clip with the mixed stand-in in place of md_default on the inter pictures.  CPU only."""
    lib = B.load()
    W, H, N, enc_mode, tune, qp, intra_period = (API[k] for k in ("W", "H", "N", "enc_mode", "tune", "qp", "intra_period"))
    frames = api_frames()
    q_index = lib.svt_hip_vp9_qindex_from_qp(qp)
    level_key = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 1)
    thr = thresholds()
    pics = [T.PaPic(f) for f in frames]
    recs, outs = {}, {}
    for (k, layer, lv, nl, r0, r1, used) in E.structure(N, 16, intra_period):
        src = (frames[k],) + E.chroma(frames[k], k)
        c, fl = B.EncdecFlagsConfig(enc_mode=enc_mode, tune=tune, temporal_layer_index=layer, is_used_as_reference=used, recon_file=1, loop_filter=1), B.EncdecFlags()
        assert lib.svt_hip_encdec_flags_derive(C.byref(c), C.byref(fl)) == 0
        if nl == 0:
            o = M.oracle_intra_chain(src, E.intra_stand_in(W, H, level_key), q_index, fl, thr)
            recs[k], outs[k] = o["rec"], dict(intra=True, o=o)
            continue
        p = B.me_params_derive(pic_width=W, pic_height=H, enc_mode=enc_mode, tune=tune, frame_rate=60, num_ref_lists=nl, temporal_layer_index=layer,
                               hierarchical_levels=lv, is_used_as_reference=used, same_ref_poc=int(nl == 2 and r0 == r1))
        me, _ = T.oracle_me_picture_mt(pics[k], pics[r0], pics[r1] if nl == 2 else None, p)
        q_pic = lib.svt_hip_vp9_layer_qindex(qp, tune, lv, layer, 0)
        ac_pic = lib.svt_hip_vp9_ac_step(q_pic)
        ois = S.oracle_ois(src)
        mc, lf, n_intra = mixed_stand_in(me, ois, W, H, 4 * ac_pic, lib.svt_hip_lf_level_from_q(ac_pic, 0))
        assert n_intra == X.model(me, ois, W, H, 4 * ac_pic, 8 * ac_pic, lib.svt_hip_lf_level_from_q(ac_pic, 0))[2]
        o = M.oracle_encdec_picture(src, [recs[r0], recs[r1 if nl == 2 else r0]], mc, lf, q_pic, fl, thr, use_subpel=int(p.fractional_search_model != 2))
        recs[k], outs[k] = o["rec"], dict(intra=False, o=o, mc=mc, n_intra=n_intra)
    return recs, outs


def test_api_clip_holds_pictures_with_and_without_intra_leaves():
    """conditions on the input, from the model alone: at least three inter pictures come out with intra leaves and at least one with none"""
    _, outs = oracle_clip_mixed()
    counts = {k: o["n_intra"] for k, o in outs.items() if not o["intra"]}
    assert sum(n > 0 for n in counts.values()) >= 3 and sum(n == 0 for n in counts.values()) >= 1, counts
    assert all(counts[k] > 0 for k in API["striped"]), counts


def test_public_api_mixed_opt_in_equals_the_oracle_chain():
    W, H, N, enc_mode, tune, qp, intra_period = (API[k] for k in ("W", "H", "N", "enc_mode", "tune", "qp", "intra_period"))
    frames = list(api_frames())
    recs, outs = oracle_clip_mixed()
    _, recon, order, flags_seen, packets, infos, _, _ = E.run_clip(W, H, N, enc_mode, tune, qp, 1, intra_period, False, env={"SVT_HIP_INTER_DECISION": "mixed"}, frames=frames)
    assert sorted(order) == list(range(N)) and len(packets) == N and packets[-1][1] & 1 and flags_seen[-1] == 1
    for k in range(N):
        y, u, v = recs[k].interior()
        assert np.array_equal(recon[k], np.concatenate([y.ravel(), u.ravel(), v.ravel()])), (k, outs[k]["intra"], outs[k].get("n_intra"))
    with_intra = without = 0
    for k, d in infos.items():
        i, o = d["info"], outs[k]["o"]
        assert d["lf"].tobytes() == o["lf_mi"].tobytes() and np.array_equal(d["q"], o["qcoeff"]) and np.array_equal(d["em"], o["eob_map"]), k
        if outs[k]["intra"]:
            assert i.is_intra and i.decision_source == 0                         # the key frame keeps its own stand-in
            continue
        assert i.decision_source == 3 and i.do_recon, k
        assert d["mc"].tobytes() == outs[k]["mc"].tobytes(), k
        assert int((d["lf"]["is_inter"] == 0).sum()) == outs[k]["n_intra"], k
        with_intra += outs[k]["n_intra"] > 0
        without += outs[k]["n_intra"] == 0
    assert with_intra >= 3 and without >= 1                                      # both the has_intra = 1 and the has_intra = 0 path ran
    # without the variable: today's behaviour, decision_source 0, the default stand-in's chain
    _, recon0, _, _, _, infos0, _, _ = E.run_clip(W, H, N, enc_mode, tune, qp, 1, intra_period, False, frames=frames)
    recs0, outs0 = E.oracle_clip(frames, W, H, N, enc_mode, tune, qp, 1, intra_period, False)
    for k in range(N):
        y, u, v = recs0[k].interior()
        assert np.array_equal(recon0[k], np.concatenate([y.ravel(), u.ravel(), v.ravel()])), k
    assert all(d["info"].decision_source == 0 and (outs0[k]["intra"] or (d["lf"]["is_inter"] == 1).all()) for k, d in infos0.items())
    assert sum(not np.array_equal(recon[k], recon0[k]) for k in API["striped"]) == len(API["striped"])


def test_public_api_rejects_an_unknown_inter_decision():
    import os
    lib = E.shim()
    cfg, h = E.Cfg(), C.c_void_p()
    assert lib.eb_vp9_svt_init_handle(C.byref(h), None, C.byref(cfg)) == 0
    cfg.source_width, cfg.source_height, cfg.enc_mode, cfg.tune, cfg.frame_rate, cfg.intra_period, cfg.qp = 256, 192, 8, 1, 60 << 16, 19, 40
    assert lib.eb_vp9_svt_enc_set_parameter(h, C.byref(cfg)) == 0
    saved = os.environ.get("SVT_HIP_INTER_DECISION")
    os.environ["SVT_HIP_INTER_DECISION"] = "bogus"
    try:
        assert lib.eb_vp9_init_encoder(h) & 0xffffffff == 0x80001005                # EB_ErrorBadParameter
    finally:
        if saved is None:
            os.environ.pop("SVT_HIP_INTER_DECISION", None)
        else:
            os.environ["SVT_HIP_INTER_DECISION"] = saved
    assert lib.eb_vp9_deinit_handle(h) == 0

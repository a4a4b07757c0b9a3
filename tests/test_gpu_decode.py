"""GPU: the reconstruction kernel (svt_hip_recon_batch_device, csrc/recon_kernel.hip) against the forward path's own reconstruction, block
level, and packets to pictures: the device chain from the stand-in decision to the packets, the arena copied to the host, every packet read
by svt_hip_frame_read_host, what it returned uploaded into FRESH buffers, and the decode pass (svt_hip_decode_batch_device) rebuilds the very
prediction, reconstruction (padding included), skip flags and loop-filter masks the encode pass left.  All comparisons exact.  Inputs: tests/decode_model.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import boolcode_model as BM
import decode_model as D
import encdec_model as EM
import frame_model as FM
import modes_inter_model as IM
import svt_testlib as T
from test_gpu_encdec import DevPicture, dev, flags_of, make_inputs, masks_equal
from test_gpu_frame import frame_batch
from test_gpu_md_inter import MdBuffers, md_device
from test_gpu_modes import Tile
from test_gpu_modes_inter import InterBuffers, modes_device
from test_gpu_tokenize import TokBuffers, tokenize_device
from test_tile_read_inter import read_frame

B = T.B
pytestmark = pytest.mark.gpu
GUARD = D.GUARD
KEY = dict(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=0, loop_filter=1)    # every encode-pass flag on


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def block_mask(case):
    m = np.zeros(case["pred"].shape, bool)
    for b, (y, x) in zip(case["blocks"], case["place"]):
        n = T.TX_N[int(b["tx_size"])]
        m[y:y + n, x:x + n] = True
    return m


def recon_from_coefficients(ctx, case, q, eob):
    """svt_hip_recon_batch_device over the case's lists into a plane of guard bytes: (plane, overflow count)"""
    lib = B.load()
    pred, blocks, qt, q_t, eob_t = up(case["pred"]), up(case["blocks"]), up(case["qtabs"]), up(q), up(eob)
    recon = torch.full((case["pred"].size,), GUARD, dtype=torch.uint8, device="cuda")
    over = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cnt = (C.c_int32 * 4)(*[int(v) for v in case["counts"]])
    torch.cuda.synchronize()
    B.check(lib.svt_hip_recon_batch_device(ctx, ptr(pred), ptr(recon), ptr(blocks), cnt, ptr(qt), ptr(q_t), ptr(eob_t), ptr(over)))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    over = over.cpu().numpy()
    assert (over[1:] == 0x5A5A5A5A).all()
    return recon.cpu().numpy().reshape(case["pred"].shape), int(over[0])


@pytest.mark.parametrize("q_index", [0, 120, 255])
def test_kernel_rebuilds_what_the_forward_path_reconstructed(ctx, q_index):
    """48 blocks of every transform size with every type it allows: svt_hip_tq_batch_device with do_recon gives qcoeff, eob and recon;
    svt_hip_recon_batch_device from qcoeff, eob and the same prediction writes the same bytes"""
    lib = B.load()
    case = D.block_case(q_index)
    src, pred, blocks, qt, isc = up(case["src"]), up(case["pred"]), up(case["blocks"]), up(case["qtabs"]), up(case["iscan"])
    recon = torch.full((case["src"].size,), GUARD, dtype=torch.uint8, device="cuda")
    q_t = torch.zeros(case["n_coeff"], dtype=torch.int16, device="cuda")
    dq_t = torch.zeros(case["n_coeff"], dtype=torch.int16, device="cuda")
    eob_t = torch.zeros(len(case["blocks"]), dtype=torch.int16, device="cuda")
    cnt = (C.c_int32 * 4)(*[int(v) for v in case["counts"]])
    torch.cuda.synchronize()
    B.check(lib.svt_hip_tq_batch_device(ctx, ptr(src), ptr(pred), ptr(recon), ptr(blocks), cnt, ptr(qt), ptr(isc), ptr(q_t), ptr(dq_t), ptr(eob_t)))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    want = recon.cpu().numpy().reshape(case["src"].shape)
    q, dq, eob = q_t.cpu().numpy(), dq_t.cpu().numpy(), eob_t.cpu().numpy().view(np.uint16)
    # the inputs are what they were built to be: the oracle's eobs, every threshold side among the DCT blocks, flat and saturated blocks
    for i, (w, g) in enumerate(zip(case["want_eob"], case["groups"])):
        assert w is None or eob[i] == w, (i, g)
    for ts in range(4):
        have = {int(e) for e, g in zip(eob, case["groups"]) if g == (ts, 0)}
        need = set(D.THRESHOLD_EOBS[ts]) - (set(D.UNREACHED_AT_Q0.get(ts, ())) if q_index == 0 else set())
        assert need <= have and 0 in have, (ts, sorted(have))
    wdq, over = D.dequantise(q, case["blocks"], case["qtabs"])
    assert np.array_equal(wdq, dq) and over == 0                          # the numpy rule of the overflow test below is the forward path's
    inside = block_mask(case)
    assert (want[~inside] == GUARD).all() and not (want[inside] == GUARD).all()
    got, overflow = recon_from_coefficients(ctx, case, q, eob)
    assert got.tobytes() == want.tobytes(), int(np.count_nonzero(got != want))
    assert (got[~inside] == GUARD).all()
    assert overflow == 0
    # a block with eob 0 copies the prediction
    for b, (y, x), e in zip(case["blocks"], case["place"], eob):
        if e == 0:
            n = T.TX_N[int(b["tx_size"])]
            assert np.array_equal(got[y:y + n, x:x + n], case["pred"][y:y + n, x:x + n])


def test_overflow_count_of_a_constructed_list(ctx):
    """coefficients of +-32767 among small ones at q index 255: the count is the one numpy computes; eob 0 blocks are not counted"""
    rng = np.random.default_rng(77)
    qt = D.qindex_tables(255)
    _, offs = T.iscan_array()
    stride, per = 4 * 61, 6
    specs = [(ts, int(rng.integers(0, 4)) if ts < 3 else 0) for ts in range(4) for _ in range(per)]
    height = 3 + sum(T.TX_N[ts] + 3 for ts, _ in specs)
    pred = rng.integers(0, 256, (height, stride)).astype(np.uint8)
    blocks = np.zeros(len(specs), dtype=B.TQ_BLOCK_DTYPE)
    place, coeffs, eob, y, pos = [], [], [], 3, 0
    for i, (ts, tt) in enumerate(specs):
        n = T.TX_N[ts]
        x = 4 * (1 + i % 3)
        c = rng.integers(-40, 41, n * n)
        big = rng.random(n * n) < 0.3
        c[big] = rng.choice((-32767, 32767), int(big.sum()))
        e = 0 if i % per == per - 1 else n * n                             # the last block of every size: coefficients present, eob 0
        blocks[i] = (0, y * stride + x, y * stride + x, pos, offs[(ts, tt)], stride, stride, stride, ts, tt, i & 1, 1, 0, 0)
        place.append((y, x)); coeffs.append(c.astype(np.int16)); eob.append(e)
        y, pos = y + n + 3, pos + n * n
    q = np.concatenate(coeffs)
    case = dict(pred=pred, blocks=blocks, qtabs=qt, counts=np.array([per] * 4, np.int32), place=place)
    want = D.dequantise(q, blocks[np.array(eob) != 0], qt)[1]
    assert want > 1000
    got, overflow = recon_from_coefficients(ctx, case, q, np.array(eob, np.uint16))
    assert overflow == want
    inside = block_mask(case)
    assert (got[~inside] == GUARD).all()
    wdq = D.dequantise(q, blocks, qt)[0]
    compared = 0
    for (ts, tt), (yy, x), e, b in zip(specs, place, eob, blocks):
        n = T.TX_N[ts]
        if e == 0:
            assert np.array_equal(got[yy:yy + n, x:x + n], pred[yy:yy + n, x:x + n])
        elif tt == 0 or ts in (0, 3):
            # the bytes too: the inverse DCT and the 4-point ADST are defined C for every int16 input.  The 8x8 and 16x16 ADST blocks stay
            # count-only: at +-32767 their 32-bit sums overflow in the C reference itself, nothing to compare with
            o = int(b["coeff_off"])
            assert np.array_equal(got[yy:yy + n, x:x + n], T.oracle_inv_add(wdq[o:o + n * n], pred[yy:yy + n, x:x + n], ts, tt, e)), (ts, tt)
            compared += 1
    assert compared >= 10                                                  # (the five coded 4x4 and the five coded 32x32 blocks at least)


def test_recon_entry_refusals(ctx):
    lib = B.load()
    t = torch.full((256,), GUARD, dtype=torch.uint8, device="cuda")
    cnt, neg = (C.c_int32 * 4)(1, 0, 0, 0), (C.c_int32 * 4)(1, -1, 0, 0)
    ok = [ctx, ptr(t), ptr(t), ptr(t), cnt, ptr(t), ptr(t), ptr(t), ptr(t)]
    for k in (0, 1, 2, 3, 4, 5, 6, 7):
        a = list(ok)
        a[k] = None
        assert lib.svt_hip_recon_batch_device(*a) != 0, k
    a = list(ok)
    a[4] = neg
    assert lib.svt_hip_recon_batch_device(*a) != 0
    a = list(ok)
    a[6] = C.c_void_p(t.data_ptr() + 2)                                   # coefficients not 16-byte aligned
    assert lib.svt_hip_recon_batch_device(*a) != 0
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == GUARD).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# picture level
# ---------------------------------------------------------------------------------------------------------------------------------------
W, H, Q_INDEX, N_PICS = 136, 72, 120, 2          # partial SBs in both directions; leaves of 8x8, 16x16 and 32x32 from the stand-in decision


@pytest.fixture(scope="module")
def encoded(ctx):
    """the set-up of test_chain_from_the_stand_in_to_the_packets_on_one_stream: stand-in decision -> encode pass (all flags on) -> tokeniser ->
    labelling -> inter mode info -> bool coder -> frame, two B pictures under REFERENCE_SELECT that differ in the restrict flag, nothing
    between the calls.  The arena is copied to the host and svt_hip_frame_read_host reads every packet: `pics` holds what the encode pass left
    on the device, `read` what the reader returned from the bytes alone.  Downloaded once, left unchanged."""
    lib = B.load()
    B.check(lib.svt_hip_boolcode_set_tables(ctx, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(ctx, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    srcs, refs, me = make_inputs(W, H, N_PICS, seed=67)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(Q_INDEX), 0)
    fr, lrf = IM.frame(**IM.B_PICTURE), (IM.LAST, IM.ALTREF)
    # frame_parallel_decoding_mode: a delivered header must keep a decoder from adapting backwards (tests/test_frame_read.py)
    fp = FM.inter(width=W, height=H, reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1), base_qindex=Q_INDEX, filter_level=level,
                  frame_parallel_decoding_mode=1)
    head = FM.host_header_bytes(fp)
    pic, nco = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
    slab_src, slab_pred = torch.zeros(N_PICS * pic, dtype=torch.uint8, device="cuda"), torch.zeros(N_PICS * pic, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(N_PICS * nco, dtype=torch.int16, device="cuda"), torch.zeros(N_PICS * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    blank = (np.zeros((H // 8, W // 8), B.MC_MODE_INFO_DTYPE), np.zeros((H // 8, W // 8), B.LF_MODE_INFO_DTYPE))
    dp = [DevPicture(W, H, srcs[i], refs_dev, blank[0], blank[1], slab_src, slab_pred, slab_q, slab_dq, i, EM.RefPic(W, H)) for i in range(N_PICS)]
    res_t = [dev(m.view(np.uint8)) for m in me]
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
    arr = (B.EncdecPicture * N_PICS)(*[d.struct(refs) for d in dp])
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, N_PICS, W, H, C.byref(work)))
    tbs, vbs, mbs = [TokBuffers(W, H, counts=False) for _ in dp], [MdBuffers(W, H, want_cand=False) for _ in dp], [InterBuffers(W, H) for _ in dp]
    tiles = [Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]
    arena, packets = frame_batch(ctx, tiles, [head] * N_PICS)
    metas = [dict(W=W, H=H, frame=fr, restrict=rs, lrf=lrf) for rs in (0, 1)]
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_md_default_batch_device(ctx, N_PICS, ptrs(res_t), W, H, 300, level, ptrs([d.mc_t for d in dp]), ptrs([d.lf_t for d in dp]), W // 8))
        B.check(lib.svt_hip_encdec_batch_device(ctx, work, N_PICS, arr, W, H, W // 8, Q_INDEX, C.byref(flags), C.byref(thr), EM.PAD, EM.PAD))
        tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t) for d in dp], tbs)
        md_device(ctx, W, H, [vb.struct((d.lf_t, d.mc_t), m, ref_mask=0) for vb, d, m in zip(vbs, dp, metas)])
        modes_device(ctx, W, H, [((d.lf_t, d.mc_t, vb.ext), d.emap_t, tb.tok_off, fr) for d, vb, tb in zip(dp, vbs, tbs)], mbs)
        B.check(lib.svt_hip_boolcode_batch_device(ctx, N_PICS, (B.BoolStream * N_PICS)(*[t.struct for t in tiles])))
        B.check(lib.svt_hip_frame_batch_device(ctx, N_PICS, packets, arena.address, arena.cap, arena.table.data_ptr()))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        cnt = (C.c_int32 * 8)()
        assert lib.svt_hip_encdec_work_status(ctx, work, cnt) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    data, table, _, _, _ = arena.result()                                  # the arena on the host
    pics, read = [], []
    for i, (d, vb, m) in enumerate(zip(dp, vbs, metas)):
        got = vb.result()
        assert got["guards"] and got["status"][0] > 0 and got["status"][2] == 0        # every NEWMV leaf codable faithfully
        pics.append(dict(lf=d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8), mc=d.mc_t.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8),
                         ext=got["ext_out"].copy(), q=d.q_t.cpu().numpy(), emap=d.emap_t.cpu().numpy(), pred=d.pred_t.cpu().numpy(), rec=d.rec_t.cpu().numpy(),
                         lfm=d.lfm_t.cpu().numpy().view(B.LF_MASK_DTYPE)))
        off, size = (int(v) for v in table[i])
        packet = bytes(data[off:off + size])
        assert packet[:len(head)] == head and size > len(head)
        rc, info, out = read_frame(packet, W, H, restrict=m["restrict"], lrf=lrf)
        assert rc == 0, lib.svt_hip_last_error()
        read.append(dict(out, info=info, packet_bytes=size, header_bytes=len(head)))
    return dict(refs=refs, refs_dev=refs_dev, thr=thr, pics=pics, read=read, counts=list(cnt), level=level)


def test_the_reader_returns_from_the_packets_what_the_encode_pass_held(encoded):
    """grids, extension records, eob map and coefficients read from each packet equal the encode pass's device buffers"""
    for p, r in zip(encoded["pics"], encoded["read"]):
        assert r["guards"]
        info, res = r["info"], r["res"]
        assert info.needs_backward_adaptation == 0 and info.interp_filter == B.READ_FILTER_REGULAR and info.tx_mode == 3 and not info.lossless
        assert (info.params.width, info.params.height, info.params.base_qindex, info.params.filter_level) == (W, H, Q_INDEX, encoded["level"])
        assert r["lf_mi"].tobytes() == p["lf"].tobytes(), [f for f in p["lf"].dtype.names if not np.array_equal(r["lf_mi"][f], p["lf"][f])]
        assert r["mc_mi"].tobytes() == p["mc"].tobytes(), [f for f in p["mc"].dtype.names if not np.array_equal(r["mc_mi"][f], p["mc"][f])]
        assert r["ext"].tobytes() == np.ascontiguousarray(p["ext"]).tobytes()
        assert np.array_equal(r["qcoeff"], p["q"]) and np.array_equal(r["eob_map"], p["emap"].view(np.uint16))
        assert res["past_end"] == 0 and res["odd_candidates"] == 0 and res["tile_bytes"] in (r["packet_bytes"] - r["header_bytes"], r["packet_bytes"] - r["header_bytes"] - 1)
        # what the check needs: inter leaves, compound ones among them, all four transform sizes, coded leaves
        assert res["inter_leaves"] > 0 and res["inter_leaves"] == res["leaves"] and res["skipped_leaves"] < res["leaves"] and res["tokens"] > 0
        assert (r["mc_mi"]["ref_list"][:, :, 1] >= 0).any(), "at least one leaf is compound"
        assert (r["ext"]["ref_frame"][:, :, 1] > 0).any() and (r["ext"]["ref_frame"][:, :, 1] == 0).any()
    assert all(encoded["counts"][4 + s] > 0 for s in range(4)), "all four transform sizes occur"


class DecodeBuffers:
    """fresh device buffers of a batch for the decode pass, filled with what the READER returned from the packets; outputs start as junk"""

    def __init__(self, enc, skip_as_coded=True):
        pic, nco = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
        n = len(enc["pics"])
        self.slab_pred = torch.full((n * pic,), 0x3C, dtype=torch.uint8, device="cuda")
        self.slab_q = torch.zeros(n * nco, dtype=torch.int16, device="cuda")
        rng = np.random.default_rng(9)
        self.items = []
        for i, p in enumerate(enc["read"]):
            lf = np.ascontiguousarray(p["lf_mi"]).copy()
            if not skip_as_coded:
                lf["skip"] = 0
            self.slab_q[i * nco:(i + 1) * nco].copy_(torch.from_numpy(np.ascontiguousarray(p["qcoeff"])))
            rec = EM.RefPic(W, H)
            rec.buf[:] = rng.integers(0, 256, rec.buf.size, dtype=np.uint8)      # a recycled buffer holds junk
            self.items.append(dict(lf_t=dev(lf.view(np.uint8)), mc_t=dev(np.ascontiguousarray(p["mc_mi"]).view(np.uint8)), emap_t=dev(np.ascontiguousarray(p["eob_map"]).view(np.int16)), rec=rec, rec_t=dev(rec.buf), rec_init=rec.buf.copy(),
                                   lfm_t=torch.full((T.n_sb(W, H) * 160,), 0x77, dtype=torch.uint8, device="cuda"),
                                   nz_t=torch.full((lf.size,), 7, dtype=torch.uint8, device="cuda"),
                                   pred_t=self.slab_pred[i * pic:(i + 1) * pic], q_t=self.slab_q[i * nco:(i + 1) * nco]))
        self.status = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")

    def structs(self, enc, **over):
        out = []
        for it in self.items:
            p = B.EncdecPicture()
            p.d_mc_mi, p.d_lf_mi = it["mc_t"].data_ptr(), it["lf_t"].data_ptr()
            base = it["pred_t"].data_ptr()
            p.pred.y, p.pred.u, p.pred.v = base, base + W * H, base + W * H + (W // 2) * (H // 2)
            p.pred.y_stride, p.pred.uv_stride, p.pred.width, p.pred.height = W, W // 2, W, H
            p.recon = it["rec"].desc(it["rec_t"].data_ptr())
            for l in range(2):
                p.ref[l] = enc["refs"][l].desc(enc["refs_dev"][l].data_ptr())
            p.d_qcoeff, p.d_eob_map = it["q_t"].data_ptr(), it["emap_t"].data_ptr()
            p.d_lfm, p.d_nz, p.use_subpel = it["lfm_t"].data_ptr(), it["nz_t"].data_ptr(), 1       # src and d_dqcoeff stay NULL: not looked at
            for k, v in over.items():
                setattr(p, k, v)
            out.append(p)
        return (B.EncdecPicture * len(out))(*out)


@pytest.mark.parametrize("skip_as_coded", [True, False])
def test_decode_pass_rebuilds_the_encode_pass_pictures(ctx, encoded, skip_as_coded):
    """packets to pictures: what svt_hip_frame_read_host returned from each packet, uploaded into fresh buffers -> svt_hip_decode_batch_device
    with the same padded references: prediction planes, reconstruction planes including the padding, skip flags and svt_lf_mask records equal the encode pass's.
    skip_as_coded = False: the grid arrives with every skip flag 0 and the pass derives them from the eobs"""
    lib = B.load()
    bufs = DecodeBuffers(encoded, skip_as_coded)
    arr = bufs.structs(encoded)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, N_PICS, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_decode_batch_device(ctx, work, N_PICS, arr, W, H, W // 8, Q_INDEX, C.byref(encoded["thr"]), EM.PAD, EM.PAD, ptr(bufs.status)))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        cnt = (C.c_int32 * 8)()
        assert lib.svt_hip_encdec_work_status(ctx, work, cnt) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    assert list(cnt) == encoded["counts"]
    st = bufs.status.cpu().numpy()
    assert st[0] == 0 and (st[1:] == 0x5A5A5A5A).all()
    for it, p in zip(bufs.items, encoded["pics"]):
        assert np.array_equal(it["pred_t"].cpu().numpy(), p["pred"]), "prediction"
        rec = it["rec_t"].cpu().numpy()
        for name, a, b in zip("yuv", it["rec"].planes(rec), it["rec"].planes(p["rec"])):
            assert a.tobytes() == b.tobytes(), ("reconstruction plane with its padding", name, int(np.count_nonzero(a != b)))
        planes_end = it["rec"].v_base + it["rec"].cpw * it["rec"].cph                 # (the buffer's alignment tail belongs to no plane)
        assert np.array_equal(rec[planes_end:], it["rec_init"][planes_end:])
        lf = it["lf_t"].cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
        assert np.array_equal(lf["skip"], p["lf"]["skip"]), "skip flags"
        for f in ("sb_type", "tx_size", "is_inter", "filter_level", "pad"):
            assert np.array_equal(lf[f], p["lf"][f]), f
        assert masks_equal(it["lfm_t"].cpu().numpy().view(B.LF_MASK_DTYPE), p["lfm"]), "loop-filter masks"
        assert np.array_equal(it["emap_t"].cpu().numpy().view(np.uint16), p["emap"].view(np.uint16)) and np.array_equal(it["q_t"].cpu().numpy(), p["q"])      # inputs stay


def test_decode_pass_reports_an_intra_leaf(ctx, encoded):
    """a grid with an is_inter = 0 leaf although has_intra is 0: reported through svt_hip_encdec_work_status"""
    lib = B.load()
    bufs = DecodeBuffers(encoded)
    lf = np.ascontiguousarray(encoded["read"][1]["lf_mi"]).copy()
    lf["is_inter"][0, 0] = 0
    bufs.items[1]["lf_t"] = dev(lf.view(np.uint8))
    arr = bufs.structs(encoded)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, N_PICS, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_decode_batch_device(ctx, work, N_PICS, arr, W, H, W // 8, Q_INDEX, C.byref(encoded["thr"]), EM.PAD, EM.PAD, ptr(bufs.status)))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) != 0
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0            # (the flag is cleared by the call that reports it)
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)


def test_decode_pass_refusals(ctx, encoded):
    """has_intra, null fields, geometry that differs from the workspace: non-zero, nothing launched, every buffer as it was"""
    lib = B.load()
    bufs = DecodeBuffers(encoded)
    thr = C.byref(encoded["thr"])
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, N_PICS, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        def rc(arr, n=N_PICS, w=W, h=H, stride=W // 8, q=Q_INDEX, status=ptr(bufs.status), wk=work, c=ctx):
            return lib.svt_hip_decode_batch_device(c, wk, n, arr, w, h, stride, q, thr, EM.PAD, EM.PAD, status)
        ok = bufs.structs(encoded)
        assert rc(bufs.structs(encoded, has_intra=1)) == -4                     # SVT_HIP_ERR_UNSUPPORTED
        for field in ("d_mc_mi", "d_lf_mi", "d_qcoeff", "d_eob_map", "d_lfm", "d_nz"):
            assert rc(bufs.structs(encoded, **{field: None})) != 0, field
        for plane in ("pred", "recon"):
            arr = bufs.structs(encoded)
            getattr(arr[1], plane).u = None
            assert rc(arr) != 0, plane
        assert rc(ok, n=0) != 0 and rc(ok, n=N_PICS + 1) != 0 and rc(ok, w=W + 8) != 0 and rc(ok, h=H - 8) != 0 and rc(ok, stride=W // 8 - 1) != 0
        assert rc(ok, q=256) != 0 and rc(None) != 0 and rc(ok, status=None) != 0 and rc(ok, wk=None) != 0 and rc(ok, c=None) != 0
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    assert (bufs.status.cpu().numpy() == 0x5A5A5A5A).all() and (bufs.slab_pred.cpu().numpy() == 0x3C).all()
    for it in bufs.items:
        assert np.array_equal(it["rec_t"].cpu().numpy(), it["rec_init"]) and (it["lfm_t"].cpu().numpy() == 0x77).all() and (it["nz_t"].cpu().numpy() == 7).all()

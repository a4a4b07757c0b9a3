"""GPU: the decode pass's arithmetic on coefficients no forward transform produces (tests/decode_model.py: coeff_edge_cases) -- the int16
wraps of the dequantiser, of every stored step of the inverse, of the row-pass tile and of the column result, the 32x32 halving towards
zero, the eob shortcuts -- through all three launch forms of rc_block_body (csrc/rc_core.h): descriptor lists (svt_hip_recon_batch_device)
against the reference's recorded bytes (tests/golden/recon_edges_reference.npz) and the oracle; position codes
(svt_hip_decode_batch_device) and the intra wavefront (svt_hip_decode_intra_device) against block-by-block CPU walks built on
oracle_inv_txfm_add (decode_model.decode_inter_picture / decode_intra_picture, pinned on the CPU by tests/test_recon_edges.py).  Amplitudes
stay inside the domain in which the C reference is defined.  All comparisons exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_model as D
import encdec_model as M
import svt_testlib as T
from test_gpu_decode import block_mask, recon_from_coefficients
from test_gpu_decode_intra import JUNK, run_decode
from test_gpu_encdec import dev

B = T.B
pytestmark = pytest.mark.gpu
GUARD = D.GUARD


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


# ---------------------------------------------------------------------------------------------------------------------------------------
# descriptor lists
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge():
    """the cases, a block with eob 0 and non-zero coefficients per size behind them, and what every block must reconstruct to: the
    reference's recorded bytes, which the oracle must equal (computed once, left unchanged)"""
    cases = D.coeff_edge_cases()
    g = np.load(T.GOLDEN_DIR + "/recon_edges_reference.npz")
    assert [c["name"] for c in cases] == list(g["names"])
    want, over, pos = [], [], 0
    for c in cases:
        n = T.TX_N[c["tx_size"]]
        dq, o = D.case_dqcoeff(c)
        w = g["recon"][pos:pos + n * n].reshape(n, n)
        assert np.array_equal(T.oracle_inv_add(dq, c["pred"], c["tx_size"], c["tx_type"], c["eob"]), w), c["name"]
        want.append(w); over.append(o)
        pos += n * n
    for ts in range(4):                               # eob 0: coefficients present, not read, not counted; the prediction is copied
        src = next(c for c in cases if c["tx_size"] == ts and c["family"] == "q255")
        cases.append(dict(src, name="eob0/" + src["name"], family="eob0", eob=0))
        want.append(src["pred"]); over.append(0)
    return dict(cases=cases, want=want, over=over)


@pytest.mark.parametrize("reverse", [False, True])
def test_descriptor_lists_equal_the_recorded_reference(ctx, edge, reverse):
    """every case in one launch of svt_hip_recon_batch_device: the bytes inside every block equal the fixture (= the oracle), the guard bytes
    are untouched, the overflow count is decode_model's.  reverse: the same blocks in lists read backwards and cut by two, so other blocks
    share a workgroup and other extreme blocks run beside the idle slots of each size's partly filled last workgroup -- the same bytes per
    block."""
    case = D.edge_block_case(edge["cases"], reverse=reverse, drop=2 if reverse else 0)
    for ts in range(4):                               # more than one workgroup per size, the last one partly filled
        assert case["counts"][ts] % (256 // T.TX_N[ts]) != 0 and case["counts"][ts] > 256 // T.TX_N[ts], (ts, case["counts"])
    want_over = sum(edge["over"][i] for i in case["order"])
    wdq, wover = D.dequantise(case["q"], case["blocks"][case["eob"] != 0], case["qtabs"])       # (the list form counts the same)
    assert wover == want_over and want_over > 1000
    got, overflow = recon_from_coefficients(ctx, case, case["q"], case["eob"])
    bad = []
    for i, (y, x) in zip(case["order"], case["place"]):
        n = T.TX_N[edge["cases"][i]["tx_size"]]
        if not np.array_equal(got[y:y + n, x:x + n], edge["want"][i]):
            bad.append(edge["cases"][i]["name"])
    assert not bad, (len(bad), bad[:12])
    assert (got[~block_mask(case)] == GUARD).all()
    assert overflow == want_over


# ---------------------------------------------------------------------------------------------------------------------------------------
# position codes: inter pictures
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ref_pics(W, H, variant):
    """two padded references per picture: all 0 and all 255 (a compound leaf predicts 128), or noise and all 255"""
    rng = np.random.default_rng(50 + variant)
    a = M.RefPic(W, H, fill=0)
    if variant:
        a.buf[:] = rng.integers(0, 256, a.buf.size, dtype=np.uint8)
        a.set_padded(*[p.copy() for p in a.interior()])
    return a, M.RefPic(W, H, fill=255)


@pytest.mark.parametrize("q_index", [0, 255])
def test_position_codes_on_inter_pictures(ctx, q_index):
    """svt_hip_decode_batch_device on two 128x64 pictures whose grids hold all four transform sizes in luma and chroma; coefficients and
    eob maps crafted from the dense / sparse / peak / shortcuts families (at q index 0 the dequantised values are the families' own, at 255
    half of the blocks wrap); thr NULL, no_pad.  Expected: the oracle's zero-motion prediction plus oracle_inv_txfm_add per block in list
    order; status[0] decode_model's count; the eob list and the skip flags follow the crafted eob map."""
    lib = B.load()
    W, H, n_pics = D.INTER_W, D.INTER_H, 2
    qt = D.qindex_tables(q_index)
    pics, total_over = [], 0
    for v in range(n_pics):
        mc, lf = D.inter_grids(v)
        table, pos, cnt = D.inter_block_table(lf)
        assert {(t[0] != 0, t[3]) for t in table} == {(c, n) for c in (False, True) for n in (4, 8, 16, 32)}
        q, emap, recs = D.crafted_coefficients(table, q_index, W, H, seed=10 * q_index + v)
        # the leaf of every block, for the skip flags: an inter leaf whose eobs are all zero is skipped.  Every third small leaf gets eob 0
        # in all of its blocks (their coefficients stay: not read, not counted)
        nz = np.zeros((H // 8, W // 8), bool)
        for plane, x0, y0, n, _ in table:
            ur, uc = (y0 // 4, x0 // 4) if plane else (y0 // 8, x0 // 8)
            n8 = int(mc[ur, uc]["bw8"])
            ur, uc = ur - ur % n8, uc - uc % n8
            if n8 <= 2 and (ur + uc) // n8 % 3 == 0:
                emap[D.eob_index(plane, x0, y0, W, H)] = 0
            if emap[D.eob_index(plane, x0, y0, W, H)]:
                nz[ur:ur + n8, uc:uc + n8] = True
        assert nz.any() and 4 < np.count_nonzero(~nz) < nz.size // 4
        refs = _ref_pics(W, H, v)
        pred = T.oracle_mc_frame(dict(mi=mc, mi_rows=H // 8, mi_cols=W // 8, refs=[r.planes() for r in refs], pad=M.PAD, use_subpel=1, width=W, height=H))
        rec, over = D.decode_inter_picture(pred, table, W, H, q, emap, qt)
        total_over += over
        pics.append(dict(mc=mc, lf=lf, q=q, emap=emap, refs=refs, pred=pred, rec=rec, skip=~nz, pos=pos, cnt=cnt, table=table))
    assert total_over > 0
    pic_bytes = W * H * 3 // 2
    slab_pred = torch.full((n_pics * pic_bytes,), 0x3C, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), JUNK, dtype=torch.int32, device="cuda")
    keep, arr = [], (B.EncdecPicture * n_pics)()
    for i, p in enumerate(pics):
        rp = M.RefPic(W, H)
        rp.buf[:] = np.random.default_rng(7 + i).integers(0, 256, rp.buf.size, dtype=np.uint8)
        t = dict(mc=dev(p["mc"].view(np.uint8)), lf=dev(p["lf"].view(np.uint8)), q=dev(p["q"]), emap=dev(p["emap"].view(np.int16)), rec=dev(rp.buf),
                 refs=[dev(r.buf) for r in p["refs"]], lfm=torch.full((T.n_sb(W, H) * 160,), 0x77, dtype=torch.uint8, device="cuda"),
                 nz=torch.full((p["lf"].size,), 7, dtype=torch.uint8, device="cuda"), refpic=rp, init=rp.buf.copy())
        keep.append(t)
        a = arr[i]
        a.d_mc_mi, a.d_lf_mi = t["mc"].data_ptr(), t["lf"].data_ptr()
        base = slab_pred.data_ptr() + i * pic_bytes
        a.pred.y, a.pred.u, a.pred.v = base, base + W * H, base + W * H + (W // 2) * (H // 2)
        a.pred.y_stride, a.pred.uv_stride, a.pred.width, a.pred.height = W, W // 2, W, H
        a.recon = rp.desc(t["rec"].data_ptr())
        for l in range(2):
            a.ref[l] = p["refs"][l].desc(t["refs"][l].data_ptr())
        a.d_qcoeff, a.d_eob_map, a.d_lfm, a.d_nz, a.use_subpel, a.no_pad = t["q"].data_ptr(), t["emap"].data_ptr(), t["lfm"].data_ptr(), t["nz"].data_ptr(), 1, 1
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n_pics, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_decode_batch_device(ctx, work, n_pics, arr, W, H, W // 8, q_index, None, M.PAD, M.PAD, C.c_void_p(status.data_ptr())))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        cnt = (C.c_int32 * 8)()
        assert lib.svt_hip_encdec_work_status(ctx, work, cnt) == 0
        total = cnt[3] + cnt[7]
        assert total == sum(len(p["table"]) for p in pics)
        blocks, pos, eob = np.zeros(total, dtype=B.TQ_BLOCK_DTYPE), np.zeros(total, np.uint32), np.zeros(total, np.uint16)
        assert lib.svt_hip_encdec_work_download(ctx, work, blocks.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), eob.ctypes.data_as(C.c_void_p), total) == total
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    st = status.cpu().numpy()
    assert int(st[0]) == total_over and (st[1:] == JUNK).all(), (st, total_over)
    # the eob list, in list order, is the crafted map's entry at every block's position code
    assert sorted(int(p) for p in pos) == sorted(int(c) | i << 24 for i, p in enumerate(pics) for c in p["pos"])
    for pc, e in zip(pos, eob):
        i, plane, y4, x4 = int(pc) >> 24, (int(pc) >> 22) & 3, (int(pc) >> 11) & 0x7FF, int(pc) & 0x7FF
        assert e == pics[i]["emap"][D.eob_index(plane, 4 * x4, 4 * y4, W, H)], hex(int(pc))
    for i, (p, t) in enumerate(zip(pics, keep)):
        got_pred = slab_pred[i * pic_bytes:(i + 1) * pic_bytes].cpu().numpy()
        assert np.array_equal(got_pred, np.concatenate([a.ravel() for a in p["pred"]])), ("prediction", i)
        got = t["rec"].cpu().numpy()
        for name, a, b in zip("yuv", t["refpic"].interior(got), p["rec"]):
            assert np.array_equal(a, b), ("reconstruction", i, name, int(np.count_nonzero(a != b)))
        outside = np.ones(got.size, bool)
        for plane in t["refpic"].interior(outside):
            plane[:] = False
        assert np.array_equal(got[outside], t["init"][outside]), "bytes outside the planes' interiors"
        lf = t["lf"].cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(p["lf"].shape)
        assert np.array_equal(lf["skip"] != 0, p["skip"]), ("skip flags", i)
        for f in ("sb_type", "tx_size", "is_inter", "filter_level", "pad"):
            assert np.array_equal(lf[f], p["lf"][f]), f
        assert np.array_equal(t["q"].cpu().numpy(), p["q"]) and np.array_equal(t["emap"].cpu().numpy().view(np.uint16), p["emap"])      # inputs stay
        assert (t["lfm"].cpu().numpy() == 0x77).all()                        # (thr NULL: no masks)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the intra wavefront
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_index", [0, 255])
def test_intra_wavefront_on_a_crafted_key_frame(ctx, q_index):
    """svt_hip_decode_intra_device (thr NULL, no_pad) on the 64x40 key frame of decode_model.KEY_FRAME: every ADST type at every size with
    amplitudes inside its type's domain, DCT blocks that wrap, eob 0 blocks that hold coefficients.  The reconstructions, saturated at 0
    and 255, are what the neighbours predict from.  1 and 16 workers: prediction and reconstruction equal decode_intra_picture's, status[0]
    its count."""
    W, H, seed = D.KEY_FRAME
    mi = M.gen_intra_grid(seed, W, H, sizes=(4, 8, 16, 32))
    walk = D.intra_walk(mi, W, H)
    q, emap, _ = D.crafted_coefficients([b[:4] + (b[5],) for b in walk], q_index, W, H, seed=q_index)
    pred, rec, over = D.decode_intra_picture(mi, W, H, q, emap, D.qindex_tables(q_index))
    assert over > 0
    for workers in (1, 16):
        d = run_decode(ctx, W, H, mi, q, emap, q_index, None, no_pad=1, workers=workers)
        assert d["rc"] == 0 and int(d["status"][0]) == over and (d["status"][1:] == JUNK).all(), (workers, d["status"], over)
        assert np.array_equal(d["pred"], np.concatenate([p.ravel() for p in pred])), ("prediction", workers)
        for name, a, b in zip("yuv", d["refpic"].interior(d["rec"]), rec):
            assert np.array_equal(a, b), ("reconstruction", workers, name, int(np.count_nonzero(a != b)))
        outside = np.ones(d["rec"].size, bool)
        for plane in d["refpic"].interior(outside):
            plane[:] = False
        assert np.array_equal(d["rec"][outside], d["rec_init"][outside]), "bytes outside the planes' interiors"
        assert np.array_equal(d["q"], q) and np.array_equal(d["emap"], emap)

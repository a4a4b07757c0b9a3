"""GPU: the stage markers of the four encode / decode entries of csrc/encdec.hip, in the order a host sees them through
svt_hip_encdec_work_set_stage_hook.  The batch entries (svt_hip_encdec_batch_device, svt_hip_decode_batch_device) announce MC, LISTS, TQ, SKIP,
LF, PAD, END; the intra entries (svt_hip_encdec_intra_device, svt_hip_decode_intra_device) TQ, SKIP, LF, PAD, END -- every marker once, whether
the loop filter and the padding run or not (a marker names the place in the chain, not a launch).  bench.py and tools/decode_time.py bracket
their stage timings with these markers."""
import ctypes as C

import numpy as np
import pytest
import torch

import encdec_model as M
import svt_testlib as T
from test_gpu_encdec import DevPicture, dev, make_inputs, md_host

B = T.B
pytestmark = pytest.mark.gpu
HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int32)
MC, LISTS, TQ, SKIP, LF, PAD, END = range(7)        # SVT_ENCDEC_STAGE_* of include/svtvp9_hip.h
BATCH_ORDER, INTRA_ORDER = [MC, LISTS, TQ, SKIP, LF, PAD, END], [TQ, SKIP, LF, PAD, END]
W = H = 64
Q_INDEX = 120


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


def stage_flags(on):
    flags, thr = B.EncdecFlags(), B.LfThresh()
    flags.do_recon, flags.apply_loop_filter, flags.pad_reference = 1, int(on), int(on)
    B.load().svt_hip_lf_thresh_init(C.byref(thr), 0)
    return flags, thr


class Recorder:
    """a workspace whose stage hook appends every marker to `seen`"""

    def __init__(self, ctx, n_pics):
        lib = B.load()
        self.ctx, self.work, self.seen = ctx, C.c_void_p(), []
        B.check(lib.svt_hip_encdec_work_create(ctx, n_pics, W, H, C.byref(self.work)))
        self.hook = HOOK(lambda _user, stage: self.seen.append(stage))      # (kept alive as long as the workspace holds it)
        lib.svt_hip_encdec_work_set_stage_hook(self.work, self.hook, None)
        torch.cuda.synchronize()

    def take(self):
        """the markers since the last take, the stream drained and the grid found well-formed"""
        lib = B.load()
        B.check(lib.svt_hip_ctx_synchronize(self.ctx))
        assert lib.svt_hip_encdec_work_status(self.ctx, self.work, None) == 0
        seen, self.seen = self.seen, []
        return seen

    def close(self):
        B.load().svt_hip_encdec_work_destroy(self.ctx, self.work)


@pytest.mark.parametrize("on", [True, False], ids=["lf_pad_on", "lf_pad_off"])
def test_batch_entries_announce_their_stages_in_order(ctx, on):
    """two 64x64 inter pictures (the stand-in decision's grids: every leaf inter) through the encode pass, then its coefficients and eob maps
    through the decode pass on the same buffers"""
    lib = B.load()
    n = 2
    srcs, refs, me = make_inputs(W, H, n, seed=5)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(Q_INDEX), 0)
    grids = [md_host(m, W, H, 300, level) for m in me]
    pic, nco = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
    slab_src, slab_pred = torch.zeros(n * pic, dtype=torch.uint8, device="cuda"), torch.zeros(n * pic, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(n * nco, dtype=torch.int16, device="cuda"), torch.zeros(n * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    dp = [DevPicture(W, H, srcs[i], refs_dev, grids[i][0], grids[i][1], slab_src, slab_pred, slab_q, slab_dq, i, M.RefPic(W, H)) for i in range(n)]
    arr = (B.EncdecPicture * n)(*[d.struct(refs) for d in dp])
    for p in arr:
        p.no_pad = 0 if on else 1                        # (the decode pass has no pad_reference flag: the pictures say it)
    flags, thr = stage_flags(on)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    rec = Recorder(ctx, n)
    try:
        B.check(lib.svt_hip_encdec_batch_device(ctx, rec.work, n, arr, W, H, W // 8, Q_INDEX, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
        assert rec.take() == BATCH_ORDER
        B.check(lib.svt_hip_decode_batch_device(ctx, rec.work, n, arr, W, H, W // 8, Q_INDEX, C.byref(thr) if on else None, M.PAD, M.PAD, C.c_void_p(status.data_ptr())))
        assert rec.take() == BATCH_ORDER
    finally:
        rec.close()


@pytest.mark.parametrize("on", [True, False], ids=["lf_pad_on", "lf_pad_off"])
def test_intra_entries_announce_their_stages_in_order(ctx, on):
    """one 64x64 key frame with blocks of every size through the intra encode entry, then its coefficients and eob map through the intra
    decode entry on the same buffers"""
    lib = B.load()
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(Q_INDEX), 1)
    mi = M.gen_intra_grid(7, W, H, sizes=(4, 8, 16, 32), filter_level=level)
    srcb = dev(np.concatenate([p.ravel() for p in T.gen_yuv(W, H, 7)]))
    predb = torch.zeros_like(srcb)
    nco = T.n_sb(W, H) * B.SB_COEFFS
    q_t, dq_t = torch.zeros(nco, dtype=torch.int16, device="cuda"), torch.zeros(nco, dtype=torch.int16, device="cuda")
    rec_pic = M.RefPic(W, H)
    rec_t, lf_t = dev(rec_pic.buf), dev(np.ascontiguousarray(mi).view(np.uint8))
    emap_t = torch.zeros(M.eob_map_offsets(W, H)[3], dtype=torch.int16, device="cuda")
    lfm_t, nz_t = torch.zeros(T.n_sb(W, H) * 160, dtype=torch.uint8, device="cuda"), torch.zeros(mi.size, dtype=torch.uint8, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")

    def tight(base):
        d = B.YuvPlanes()
        d.y, d.u, d.v = base, base + W * H, base + W * H + (W // 2) * (H // 2)
        d.y_stride, d.uv_stride, d.width, d.height = W, W // 2, W, H
        return d
    p = B.EncdecPicture()
    p.d_lf_mi, p.src, p.pred, p.recon = lf_t.data_ptr(), tight(srcb.data_ptr()), tight(predb.data_ptr()), rec_pic.desc(rec_t.data_ptr())
    p.d_qcoeff, p.d_dqcoeff, p.d_eob_map, p.d_lfm, p.d_nz = q_t.data_ptr(), dq_t.data_ptr(), emap_t.data_ptr(), lfm_t.data_ptr(), nz_t.data_ptr()
    p.no_pad = 0 if on else 1
    flags, thr = stage_flags(on)
    rec = Recorder(ctx, 1)
    try:
        B.check(lib.svt_hip_encdec_intra_device(ctx, rec.work, C.byref(p), W, H, mi.shape[1], Q_INDEX, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
        assert rec.take() == INTRA_ORDER
        B.check(lib.svt_hip_decode_intra_device(ctx, rec.work, C.byref(p), W, H, mi.shape[1], Q_INDEX, C.byref(thr) if on else None, M.PAD, M.PAD,
                                                C.c_void_p(status.data_ptr())))
        assert rec.take() == INTRA_ORDER
    finally:
        rec.close()

"""Times the open-loop intra search on one 2160p picture (T.gen_yuv): the search alone (svt_hip_intra_search_device), the grid builder alone
(svt_hip_md_intra_search_device), and the intra encode pass (svt_hip_encdec_intra_device, deblocking and border included) on the searched
grid against the 16x16 DC stand-in (svt_hip_md_intra_default_device) -- HIP events around each call on the context's stream, inputs
resident, median of the repetitions -- and prints the luma PSNR of both reconstructions at q index 140.  Run on the GPU box."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch

import encdec_model as M
import svt_testlib as T
import test_gpu_intra as TI
from test_gpu_encdec import dev, flags_of

B = T.B
lib = B.load()
REPS = int(os.environ.get("REPS", "20"))
W, H, Q = 3840, 2160, 140
stream = torch.cuda.Stream()
ctx = C.c_void_p()
B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))   # (bench.py's way: events recorded on the same stream)


def timed(fn, reps=REPS):
    """median of `reps` calls, HIP events recorded on the context's stream around each"""
    fn()
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


src = T.gen_yuv(W, H, 11)
srcb = dev(np.concatenate([p.ravel() for p in src]))
planes = B.YuvPlanes()
base = srcb.data_ptr()
planes.y, planes.u, planes.v, planes.y_stride, planes.uv_stride, planes.width, planes.height = base, base + W * H, base + W * H + (W // 2) * (H // 2), W, W // 2, W, H
n_sb = T.n_sb(W, H)
ois_t = torch.zeros(n_sb * B.OIS_PER_SB * 12, dtype=torch.uint8, device="cuda")
lf_s = torch.zeros((H // 8) * (W // 8) * 8, dtype=torch.uint8, device="cuda")
lf_d = torch.zeros_like(lf_s)
ac = lib.svt_hip_vp9_ac_step(Q)
lam, level = 4 * ac, lib.svt_hip_lf_level_from_q(ac, 1)
torch.cuda.synchronize()

search = lambda: B.check(lib.svt_hip_intra_search_device(ctx, C.byref(planes), W, H, C.c_void_p(ois_t.data_ptr())))
grid = lambda: B.check(lib.svt_hip_md_intra_search_device(ctx, C.c_void_p(ois_t.data_ptr()), W, H, C.c_uint32(lam), level, C.c_void_p(lf_s.data_ptr()), W // 8))
dcgrid = lambda: B.check(lib.svt_hip_md_intra_default_device(ctx, W, H, level, C.c_void_p(lf_d.data_ptr()), W // 8))
print("2160p open-loop intra search alone:      median %.3f ms  (min %.3f; target <= 0.5 ms)" % timed(search), flush=True)
print("2160p searched-grid builder alone:       median %.3f ms  (min %.3f)" % timed(grid), flush=True)
print("2160p search + grid builder:             median %.3f ms  (min %.3f)" % timed(lambda: (search(), grid())), flush=True)
print("2160p DC stand-in grid:                  median %.3f ms  (min %.3f)" % timed(dcgrid), flush=True)
B.check(lib.svt_hip_ctx_synchronize(ctx))
mi = lf_s.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
kinds = {st: int(np.sum(mi["sb_type"] == st)) for st in (0, 3, 6, 9)}
print("searched grid: units per block kind (sb_type: count) %s, luma modes used %s" % (kinds, sorted(set(np.unique(mi["pad"][..., 1][mi["sb_type"] > 0]).tolist()))))

flags = flags_of(**TI.KEY)
thr = B.LfThresh()
lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
nco = n_sb * B.SB_COEFFS
q_t = torch.zeros(nco, dtype=torch.int16, device="cuda")
rec = M.RefPic(W, H)
emap_t = torch.zeros(M.eob_map_offsets(W, H)[3], dtype=torch.int16, device="cuda")
lfm_t = torch.zeros(n_sb * 160, dtype=torch.uint8, device="cuda")
nz_t = torch.zeros(W * H // 64, dtype=torch.uint8, device="cuda")
work = C.c_void_p()
B.check(lib.svt_hip_encdec_work_create(ctx, 1, W, H, C.byref(work)))
for name, lf_t in (("searched grid", lf_s), ("16x16 DC stand-in", lf_d)):
    rec_t = dev(rec.buf)
    p = B.EncdecPicture()
    p.d_lf_mi, p.src, p.recon = lf_t.data_ptr(), planes, rec.desc(rec_t.data_ptr())
    p.d_qcoeff, p.d_eob_map, p.d_lfm, p.d_nz = q_t.data_ptr(), emap_t.data_ptr(), lfm_t.data_ptr(), nz_t.data_ptr()
    call = lambda: B.check(lib.svt_hip_encdec_intra_device(ctx, work, C.byref(p), W, H, W // 8, Q, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
    med, mn = timed(call, max(4, REPS // 4))
    assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    y = rec.interior(rec_t.cpu().numpy())[0].astype(np.float64)
    psnr = 10 * np.log10(255.0 ** 2 / np.mean((y - src[0]) ** 2))
    print("2160p intra pass on the %-18s median %.3f ms  (min %.3f)   luma PSNR %.2f dB at q index %d" % (name + ":", med, mn, psnr, Q), flush=True)
lib.svt_hip_encdec_work_destroy(ctx, work)
lib.svt_hip_ctx_destroy(ctx)

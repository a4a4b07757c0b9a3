"""Times the mixed stand-in decision and the batched open-loop intra search on 16 pictures of 2160p (one mini-GOP): HIP events around each
call sequence on the context's stream, inputs resident, median and minimum of the repetitions.
  (a) 16 calls of svt_hip_intra_search_device
  (b) svt_hip_intra_search_batch_device, with_4x4 = 1
  (c) svt_hip_intra_search_batch_device, with_4x4 = 0
  (d) svt_hip_md_mixed_batch_device
  (e) svt_hip_md_default_batch_device on the same ME records
The sources are shifted copies of one T.gen_yuv picture; the ME records are md_mixed_model.random_me's, scaled to the magnitude of the
searched SADs so that both sides win leaves.  Also checks (b) and (c) against (a) and prints the share of intra units (d) produced.  Run on
the GPU box."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch

import md_mixed_model as X
import svt_testlib as T
from test_gpu_encdec import dev

B = T.B
lib = B.load()
REPS = int(os.environ.get("REPS", "20"))
W, H, N, Q = 3840, 2160, 16, 140
stream = torch.cuda.Stream()
ctx = C.c_void_p()
B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))   # (bench.py's way: events recorded on the same stream)


def timed(fn, reps=REPS):
    """median and minimum of `reps` calls, HIP events recorded on the context's stream around each"""
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


y, u, v = T.gen_yuv(W, H, 11)
n_sb, units = T.n_sb(W, H), (H // 8) * (W // 8)
src_t, planes = [], (B.YuvPlanes * N)()
for i in range(N):
    s = (np.roll(y, (8 * i, 16 * i), (0, 1)), np.roll(u, (4 * i, 8 * i), (0, 1)), np.roll(v, (4 * i, 8 * i), (0, 1)))
    t = dev(np.concatenate([p.ravel() for p in s]))
    src_t.append(t)
    d, base = planes[i], t.data_ptr()
    d.y, d.u, d.v, d.y_stride, d.uv_stride, d.width, d.height = base, base + W * H, base + W * H + (W // 2) * (H // 2), W, W // 2, W, H
ois_a = [torch.zeros(n_sb * B.OIS_PER_SB * 12, dtype=torch.uint8, device="cuda") for _ in range(N)]
ois_b = [torch.zeros_like(t) for t in ois_a]
mc_t = [torch.zeros(units * 12, dtype=torch.uint8, device="cuda") for _ in range(N)]
lf_t = [torch.zeros(units * 8, dtype=torch.uint8, device="cuda") for _ in range(N)]
cnt_t = torch.zeros(N, dtype=torch.int32, device="cuda")
ac = lib.svt_hip_vp9_ac_step(Q)
lam, level = 4 * ac, lib.svt_hip_lf_level_from_q(ac, 0)
ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
torch.cuda.synchronize()


def singles():
    for i in range(N):
        B.check(lib.svt_hip_intra_search_device(ctx, C.byref(planes[i]), W, H, C.c_void_p(ois_a[i].data_ptr())))


batch = lambda w4: B.check(lib.svt_hip_intra_search_batch_device(ctx, N, planes, W, H, w4, ptrs(ois_b)))
mixed = lambda: B.check(lib.svt_hip_md_mixed_batch_device(ctx, N, md, W, H, lam, 2 * lam, level, W // 8, C.c_void_p(cnt_t.data_ptr())))
default = lambda: B.check(lib.svt_hip_md_default_batch_device(ctx, N, ptrs(res_t), W, H, lam, level, ptrs(mc_t), ptrs(lf_t), W // 8))

print("(a) 16 x svt_hip_intra_search_device:            median %.3f ms  (min %.3f)" % timed(singles), flush=True)
print("(b) svt_hip_intra_search_batch_device, 4x4 on:   median %.3f ms  (min %.3f)" % timed(lambda: batch(1)), flush=True)
B.check(lib.svt_hip_ctx_synchronize(ctx))
same_b = all(torch.equal(a, b) for a, b in zip(ois_a, ois_b))
print("(c) svt_hip_intra_search_batch_device, 4x4 off:  median %.3f ms  (min %.3f)" % timed(lambda: batch(0)), flush=True)
B.check(lib.svt_hip_ctx_synchronize(ctx))
rec = lambda t: t.view(n_sb, B.OIS_PER_SB * 12)
same_c = all(torch.equal(rec(a)[:, :84 * 12], rec(b)[:, :84 * 12]) for a, b in zip(ois_a, ois_b))
print("records: (b) == (a): %s   (c) records 0..83 == (a): %s" % (same_b, same_c), flush=True)
# ME records of the magnitude of the searched SADs, so that both sides win leaves: 8x8 distortions up to twice the median 8x8 intra SAD
sad8 = ois_a[0].cpu().numpy().view(B.OIS_BLOCK_DTYPE).reshape(n_sb, B.OIS_PER_SB)["sad"][:, 20:84]
scale = float(np.median(sad8[sad8 != B.OIS_NONE])) / 1000.0
res_t = [dev(X.random_me(50 + i, W, H, scale=scale).view(np.uint8).ravel()) for i in range(N)]
md = (B.MdMixedPicture * N)()
for i in range(N):
    md[i].d_results, md[i].d_ois, md[i].d_mc_mi, md[i].d_lf_mi = res_t[i].data_ptr(), ois_b[i].data_ptr(), mc_t[i].data_ptr(), lf_t[i].data_ptr()
torch.cuda.synchronize()
print("(d) svt_hip_md_mixed_batch_device:               median %.3f ms  (min %.3f)" % timed(mixed), flush=True)
B.check(lib.svt_hip_ctx_synchronize(ctx))
print("    intra units: %.1f %% of %d" % (100.0 * float(cnt_t.sum().item()) / (N * units), N * units), flush=True)
print("(e) svt_hip_md_default_batch_device:             median %.3f ms  (min %.3f)" % timed(default), flush=True)
lib.svt_hip_ctx_destroy(ctx)

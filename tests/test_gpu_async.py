"""C-ABI plumbing a non-blocking host needs (GPU): svt_hip_mem_upload_2d_async copies the caller's rows before it returns (the
caller may scribble over them at once) and more uploads than the context has staging buffers still arrive intact and in order;
svt_hip_ctx_marker_record / _query / _wait follow the stream: a marker recorded behind work completes after it, query never blocks,
markers older than the ring are reported complete; the launch descriptors' ring wrapped while the device is still busy with work in
front of the launches; svt_hip_last_kernel_ms answers for one call's pair of events."""
import ctypes as C

import numpy as np
import pytest

import svt_testlib as T

B = T.B
pytestmark = pytest.mark.gpu


def test_async_upload_and_markers():
    import torch
    lib = B.load()
    lib.svt_hip_ctx_marker_query.restype = C.c_int32
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(ctx), 0))
    try:
        W, H, n = 1920, 1080, 12                       # 12 uploads through 4 staging buffers
        rng = np.random.default_rng(1)
        dst = [torch.zeros((H, W + 64), dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        want, markers = [], []
        buf = np.zeros((H, W + 32), np.uint8)          # source rows with their own stride
        for k in range(n):
            buf[:, :W] = rng.integers(0, 256, (H, W), dtype=np.uint8)
            want.append(buf[:, :W].copy())
            B.check(lib.svt_hip_mem_upload_2d_async(ctx, C.c_void_p(dst[k].data_ptr()), C.c_size_t(W + 64), buf.ctypes.data_as(C.c_void_p), C.c_size_t(W + 32),
                                                    C.c_size_t(W), C.c_size_t(H)))
            buf[:] = 0xEE                              # the call has copied the rows: the caller's buffer is its own again
            m = C.c_uint64()
            B.check(lib.svt_hip_ctx_marker_record(ctx, C.byref(m)))
            markers.append(m.value)
        assert markers == list(range(markers[0], markers[0] + n))
        assert lib.svt_hip_ctx_marker_query(ctx, C.c_uint64(markers[-1])) in (0, 1)      # never blocks, never fails
        B.check(lib.svt_hip_ctx_marker_wait(ctx, C.c_uint64(markers[-1])))
        assert all(lib.svt_hip_ctx_marker_query(ctx, C.c_uint64(m)) == 1 for m in markers)   # stream order: everything before it too
        for k in range(n):
            got = dst[k].cpu().numpy()
            assert np.array_equal(got[:, :W], want[k]) and not got[:, W:].any(), k
        assert lib.svt_hip_ctx_marker_query(ctx, C.c_uint64(markers[-1] + 5)) < 0           # a marker never handed out
        for _ in range(1100):                           # wrap the marker ring: old markers stay "complete"
            m = C.c_uint64()
            B.check(lib.svt_hip_ctx_marker_record(ctx, C.byref(m)))
        assert lib.svt_hip_ctx_marker_query(ctx, C.c_uint64(markers[0])) == 1
        B.check(lib.svt_hip_ctx_marker_wait(ctx, C.c_uint64(markers[0])))
    finally:
        lib.svt_hip_ctx_destroy(ctx)


def test_planes_upload_one_slot_one_copy():
    """svt_hip_mem_upload_planes_async: the planes of a picture through one staging slot -- back-to-back tight destinations (Y | Cb | Cr in one
    buffer: one host-to-device copy) and separate, strided destinations; the caller's rows may be overwritten as soon as the call returns,
    and more pictures than staging slots arrive intact."""
    import torch
    lib = B.load()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(ctx), 0))
    try:
        W, H, n = 640, 360, 7
        rng = np.random.default_rng(9)
        P, S = C.c_void_p * 3, C.c_size_t * 3
        wb, rows = (W, W // 2, W // 2), (H, H // 2, H // 2)
        src_st = (W + 16, W // 2 + 8, W // 2)
        tight = [torch.zeros(W * H * 3 // 2, dtype=torch.uint8, device="cuda") for _ in range(n)]
        apart = [[torch.zeros((r, w + 32), dtype=torch.uint8, device="cuda") for w, r in zip(wb, rows)] for _ in range(n)]
        torch.cuda.synchronize()
        bufs = [np.zeros((r, st), np.uint8) for r, st in zip(rows, src_st)]
        want = []
        for k in range(n):
            for b_, w in zip(bufs, wb):
                b_[:, :w] = rng.integers(0, 256, (b_.shape[0], w), dtype=np.uint8)
            want.append([b_[:, :w].copy() for b_, w in zip(bufs, wb)])
            base = tight[k].data_ptr()
            B.check(lib.svt_hip_mem_upload_planes_async(ctx, 3, P(base, base + W * H, base + W * H + W * H // 4), S(*wb), P(*[b_.ctypes.data for b_ in bufs]), S(*src_st),
                                                        S(*wb), S(*rows)))
            B.check(lib.svt_hip_mem_upload_planes_async(ctx, 3, P(*[t.data_ptr() for t in apart[k]]), S(*[w + 32 for w in wb]), P(*[b_.ctypes.data for b_ in bufs]), S(*src_st),
                                                        S(*wb), S(*rows)))
            for b_ in bufs:
                b_[:] = 0xEE                             # the caller reuses its rows at once
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        for k in range(n):
            flat = tight[k].cpu().numpy()
            off = 0
            for j, (w, r) in enumerate(zip(wb, rows)):
                assert np.array_equal(flat[off:off + w * r].reshape(r, w), want[k][j]), (k, j)
                off += w * r
                a = apart[k][j].cpu().numpy()
                assert np.array_equal(a[:, :w], want[k][j]) and not a[:, w:].any(), (k, j)
        # argument checks: a null plane, a destination stride below the width
        assert lib.svt_hip_mem_upload_planes_async(ctx, 3, P(tight[0].data_ptr(), None, None), S(*wb), P(*[b_.ctypes.data for b_ in bufs]), S(*src_st), S(*wb), S(*rows)) != 0
        assert lib.svt_hip_mem_upload_planes_async(ctx, 1, P(tight[0].data_ptr(), None, None), S(W - 1, 0, 0), P(bufs[0].ctypes.data, None, None), S(*src_st), S(*wb), S(*rows)) != 0
    finally:
        lib.svt_hip_ctx_destroy(ctx)


def test_context_warm_up_and_reservations():
    """what a host calls before it starts a clock: svt_hip_ctx_warm / _warm_scratch submit an empty kernel (with a private
    segment of the asked size) and wait; svt_hip_lf_reserve takes the deblocking launches' descriptor buffer at its largest -- a launch behind it
    gives the same pictures as one that grows the buffer on demand; bad arguments are refused; a staging request larger than a ring entry's
    share of the slab still works (the entry grows on its own)."""
    lib = B.load()
    for f in ("svt_hip_ctx_warm", "svt_hip_ctx_warm_scratch", "svt_hip_lf_reserve"):
        getattr(lib, f).restype = C.c_int32
    a, b = C.c_void_p(), C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(a), 0))
    B.check(lib.svt_hip_ctx_create(C.byref(b), 0))
    try:
        assert lib.svt_hip_ctx_warm(a) == 0
        for nbytes in (0, 130, 256, 752, 1024):
            assert lib.svt_hip_ctx_warm_scratch(a, nbytes) == 0
        assert lib.svt_hip_ctx_warm(None) == -1 and lib.svt_hip_ctx_warm_scratch(a, -1) == -1
        assert lib.svt_hip_lf_reserve(a, 4, 136 // 8, 200 // 8) == 0
        assert lib.svt_hip_lf_reserve(a, 0, 17, 25) == -1 and lib.svt_hip_lf_reserve(None, 1, 17, 25) == -1 and lib.svt_hip_lf_reserve(a, 1, 0, 25) == -1
        case = T.make_lf_case(7, 200, 136)
        want = T.oracle_lf_frame(case)
        for ctx in (a, b):   # reserved / grown on demand
            for name, o, g in zip("yuv", want, T.hip_lf_frame(ctx, case)):
                assert np.array_equal(o, g), name
        big = T.make_lf_case(9, 1920, 1088)   # descriptors of 510 SBs: more than the reservation of context a -> the buffer grows
        for name, o, g in zip("yuv", T.oracle_lf_frame(big), T.hip_lf_frame(a, big)):
            assert np.array_equal(o, g), name
    finally:
        lib.svt_hip_ctx_destroy(a)
        lib.svt_hip_ctx_destroy(b)


# ---- the launch descriptors' ring and the timing bracket -------------------------------------------------------------------------
RING = 64             # SVT_CTX_RING (csrc/svt_ctx.h)
FRONT_MATMULS = 24    # 8192^3 float32 products in front of the launches: 322 ms on the MI355X, where the host enqueues 64 launches in 0.9 ms


class _LfCall:
    """one svt_hip_lf_frame_device: planes of its own inside sentinel-filled buffers (its descriptor carries the launch's counters)"""

    def __init__(self, case, lfm_t):
        from test_gpu_lf import _Padded, _padded_desc
        self.case, self.lfm_t, self.planes, self.desc = case, lfm_t, [_Padded(case[p], 0, 0) for p in "yuv"], B.YuvPlanes()
        _padded_desc(self.desc, case, *self.planes)

    def enqueue(self, ctx):
        c = self.case
        return B.load().svt_hip_lf_frame_device(ctx, C.byref(self.desc), C.c_void_p(self.lfm_t.data_ptr()), c["lfm"].shape[1], C.byref(c["thr"]), c["mi_rows"], c["mi_cols"], 0)

    def check(self, want, what):
        for n, p, w in zip("yuv", self.planes, want):
            p.check(w, what, n)


class _McCall:
    """one svt_hip_inter_pred_batch_device of one picture: grid, references and guarded prediction slabs of its own"""
    PAD = (12, 20, 1)

    def __init__(self, case):
        from test_gpu_mc import DevicePictures
        self.dp = DevicePictures([case], pred_pad=self.PAD, mi_slack=3, ref_mod=((1, 2), (3, 1)))

    def enqueue(self, ctx):
        return B.load().svt_hip_inter_pred_batch_device(ctx, 1, self.dp.pics)

    def check(self, want, what):
        from test_gpu_mc import GUARD
        for p, a, e in zip("yuv", self.dp.slab_arrays(0), want):
            full = np.full_like(a, GUARD)
            full[2:2 + e.shape[0], 4 * self.PAD[2]:4 * self.PAD[2] + e.shape[1]] = e
            assert np.array_equal(a, full), (what, p, int(np.sum(a != full)), np.argwhere(a != full)[:6].tolist())


class _MvCall:
    """one svt_hip_mvrefs_batch_device of one picture: guarded outputs of its own"""

    def __init__(self, pic, grids):
        from test_gpu_mvrefs import MvBuffers
        self.pic, self.buf = pic, MvBuffers(pic["W"], pic["H"])
        self.arr = (B.MvrefsPicture * 1)(self.buf.struct(grids, pic))

    def enqueue(self, ctx):
        return B.load().svt_hip_mvrefs_batch_device(ctx, 1, self.arr, self.pic["W"], self.pic["H"], self.pic["W"] // 8)

    def check(self, want, what):
        from test_gpu_mvrefs import same
        same(self.buf.result(), want)


@pytest.fixture(scope="module")
def ring_cases():
    """three cases a stage with what the oracle (deblocking, inter prediction) or the reference (MV references) gives for each: computed
    once, left alone"""
    import mvrefs_model as VM
    lf = [T.make_lf_case(51 + k, 200, 136) for k in range(3)]
    mc = [T.make_mc_case(61 + k, use_subpel=int(k != 1)) for k in range(3)]
    mv = [VM.fixture_picture(n) for n in VM.names() if "72x40" in n][:4]
    assert len(mv) >= 3
    for p, h in zip(mv, [VM.host_mvrefs(p) for p in mv]):     # the reference's records are the host form's too
        assert h["rc"] == 0 and h["status"] == p["status"] and np.array_equal(h["ext_out"], p["ext_out"]) and np.array_equal(h["cand"], p["cand"])
    return dict(lf=[(c, T.oracle_lf_frame(c)) for c in lf], mc=[(c, T.oracle_mc_frame(c)) for c in mc], mv=[(p, p) for p in mv])


def _calls(cases, n):
    """n calls that rotate over the three entry points, each stage cycling through its cases; [(call, expected, label)]"""
    import torch
    from test_gpu_lf import _dev_lfm
    from test_gpu_modes_inter import upload_grids
    lfm = [_dev_lfm(c) for c, _ in cases["lf"]]
    grids = [upload_grids(p) for p, _ in cases["mv"]]
    out = []
    for i in range(n):
        stage, k = ("lf", "mc", "mv")[i % 3], i // 3
        j = k % len(cases[stage])
        case, want = cases[stage][j]
        call = _LfCall(case, lfm[j]) if stage == "lf" else _McCall(case) if stage == "mc" else _MvCall(case, grids[j])
        out.append((call, want, (i, stage, j)))
    torch.cuda.synchronize()
    return out


def test_descriptor_ring_wraps_while_the_host_runs_ahead(ring_cases):
    """150 device-form launches (more than twice the 64 descriptor slots) enqueued without a synchronisation behind device work that is
    still running when the ring wraps: the host then waits for a slot's event, which sits behind the slot's copy, not behind the kernels that
    use the slot -- deblocking keeps its progress counters and ticket in the slot's device twin.  Consecutive descriptors differ in inputs
    and destinations; every call's output equals what its case gives alone."""
    import time
    import torch
    lib = B.load()
    lib.svt_hip_ctx_marker_query.restype = C.c_int32
    stream = torch.cuda.Stream()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))
    try:
        warm = _calls(ring_cases, 3)            # the stages' grow-only buffers exist before the clock starts (growing one waits for the stream)
        for call, _, what in warm:
            assert call.enqueue(ctx) == 0, what
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        calls = _calls(ring_cases, 150)
        a, b = torch.rand((8192, 8192), device="cuda"), torch.rand((8192, 8192), device="cuda")
        c = torch.empty_like(a)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t0.record()
            for _ in range(FRONT_MATMULS):
                torch.mm(a, b, out=c)
            t1.record()
        front = C.c_uint64()
        B.check(lib.svt_hip_ctx_marker_record(ctx, C.byref(front)))
        host0 = time.perf_counter()
        for i, (call, _, what) in enumerate(calls):
            assert call.enqueue(ctx) == 0, what
            if i + 1 == RING:
                host_ring = time.perf_counter() - host0
                # a condition of the test: had the device finished the front work, the ring would never have been under pressure
                assert lib.svt_hip_ctx_marker_query(ctx, front) == 0, "the front work ended before the ring wrapped: FRONT_MATMULS is too small"
        host_all = time.perf_counter() - host0
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        print(f"front work {t0.elapsed_time(t1):.1f} ms; host: {RING} enqueues in {1e3 * host_ring:.1f} ms, {len(calls)} in {1e3 * host_all:.1f} ms")
        for call, want, what in calls:
            call.check(want, what)
    finally:
        lib.svt_hip_ctx_destroy(ctx)


def test_timing_bracket_answers_for_one_call(ring_cases):
    """svt_hip_last_kernel_ms: -1 on a fresh context; the time between the two events of one call after each of the three entry points;
    a call refused before any device work leaves the last bracket as it was"""
    import math
    lib = B.load()
    lib.svt_hip_last_kernel_ms.restype = C.c_float
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(ctx), 0))
    try:
        assert lib.svt_hip_last_kernel_ms(ctx) == -1.0
        for call, want, what in _calls(ring_cases, 3):
            assert call.enqueue(ctx) == 0, what
            ms = lib.svt_hip_last_kernel_ms(ctx)
            assert math.isfinite(ms) and ms >= 0, (what, ms)
            B.check(lib.svt_hip_ctx_synchronize(ctx))
            call.check(want, what)
        assert lib.svt_hip_inter_pred_batch_device(ctx, 0, None) != 0      # refused: no picture
        ms = lib.svt_hip_last_kernel_ms(ctx)
        assert math.isfinite(ms) and ms >= 0, ms
    finally:
        lib.svt_hip_ctx_destroy(ctx)

"""Picture-analysis statistics on the GPU: every output of svt_hip_pa_noise_batch_device, svt_hip_pa_histogram_batch_device and
svt_hip_pa_chroma_mean_batch_device against the numpy model (tests/pa_stats_model.py, pinned to the reference by tests/test_pa_stats.py),
and the optional filter planes against the reference's own filter when oracle/_ref is there.  Integer arithmetic: equality."""
import ctypes as C

import numpy as np
import pytest

import pa_stats_model as M
import svt_testlib as T
import test_pa_stats as TP

B = T.B
pytestmark = pytest.mark.gpu


class Ctx:
    def __enter__(self):
        self.lib, self.ctx = B.load(), C.c_void_p()
        B.check(self.lib.svt_hip_ctx_create(C.byref(self.ctx), 0))
        return self

    def __exit__(self, *a):
        self.lib.svt_hip_ctx_destroy(self.ctx)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _plane(t, shape, pad):
    return B.plane_desc(np.empty((shape[0] + 2 * pad, shape[1] + 2 * pad), np.uint8), pad, pad, ptr=t.data_ptr())


def gpu_noise(c, method, planes, fw, fh, th, luma_height, want_planes=True):
    """planes: the analysed picture of each batch entry -> list of (flags, result record, den, noise)"""
    import torch
    n, pad = len(planes), 8
    dev = torch.device("cuda", 0)
    d_in = [_dev(np.pad(p, pad, mode="edge")) for p in planes]
    pics = (B.PaPicture * n)()
    name = ("full", "sixteenth", "quarter")[method]
    dummy = torch.zeros(16, dtype=torch.uint8, device=dev)
    for i, p in enumerate(planes):
        setattr(pics[i], name, _plane(d_in[i], p.shape, pad))
        if method != M.FULL:  # the full picture gives the SB grid only
            pics[i].full = B.Plane(dummy.data_ptr(), fw, 0, 0, fw, fh)
    nsb = ((fw + 63) // 64) * ((fh + 63) // 64)
    flags = [torch.full((nsb,), 7, dtype=torch.uint8, device=dev) for _ in range(n)]
    res = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device=dev)
    den = [torch.full(p.shape, 0xCD, dtype=torch.uint8, device=dev) for p in planes]
    noi = [torch.full(p.shape, 0xCD, dtype=torch.uint8, device=dev) for p in planes]
    prm = B.PaNoiseParams(method, th, luma_height)
    B.check(c.lib.svt_hip_pa_noise_batch_device(c.ctx, n, pics, C.byref(prm), _ptrs(flags), C.c_void_p(res.data_ptr()),
                                                _ptrs(den) if want_planes else None, _ptrs(noi) if want_planes else None))
    B.check(c.lib.svt_hip_ctx_synchronize(c.ctx))
    r = res.cpu().numpy().view(B.PA_NOISE_RESULT_DTYPE)
    return [(flags[i].cpu().numpy(), r[i], den[i].cpu().numpy(), noi[i].cpu().numpy()) for i in range(n)]


def check_noise(got, want):
    flags, r, den, noise = got
    assert np.array_equal(flags, want["flags"])
    assert (int(r["pic_noise_class"]), int(r["sb_count"]), int(r["pic_noise_variance_sum"])) == \
        (want["pic_noise_class"], want["sb_count"], want["variance_sum"])
    rows, cols = want["region"]
    assert np.array_equal(den[:rows, :cols], want["den"][:rows, :cols]) and np.array_equal(noise[:rows, :cols], want["noise"][:rows, :cols])
    # outside the area the reference's loop filters nothing is written
    assert (den[rows:] == 0xCD).all() and (den[:, cols:] == 0xCD).all() and (noise[rows:] == 0xCD).all() and (noise[:, cols:] == 0xCD).all()


@pytest.mark.parametrize("case", range(len(M.SMALL_NOISE_CASES)))
def test_noise_small_batches_vs_model(case):
    """one launch over the five noise levels: flags 0 and 1, every class the ladder of the precision can give"""
    method, aw, ah, fw, fh, th, lh = M.SMALL_NOISE_CASES[case]
    planes = [M.noise_picture(aw, ah, s) for s in M.SIGMAS]
    with Ctx() as c:
        got = gpu_noise(c, method, planes, fw, fh, th, lh)
        bare = gpu_noise(c, method, planes, fw, fh, th, lh, want_planes=False)
    classes = set()
    for g, b, p in zip(got, bare, planes):
        want = M.detect_noise(method, p, fw, fh, th, lh)
        check_noise(g, want)
        assert np.array_equal(b[0], g[0]) and b[1] == g[1]            # the same decision without the optional planes ...
        assert (b[2] == 0xCD).all() and (b[3] == 0xCD).all()          # ... which are then not touched
        classes.add(want["pic_noise_class"])
    if th == 1:
        assert len(classes) >= 3


# 3840x2160 full precision; 960x540 as the 1/16 of 2160p; 960x540 as the 1/4 of 1080p; 160x90 as the 1/16 of 640x360; and a width
# that is not a multiple of 64 in full precision
BIG = [(M.FULL, 3840, 2160, 3840, 2160, 0, 2160, 8), (M.HALF, 960, 540, 3840, 2160, 0, 2160, 12), (M.QUARTER, 960, 540, 1920, 1080, 1, 1080, 8),
       (M.HALF, 160, 90, 640, 360, 1, 360, 5), (M.FULL, 328, 200, 328, 200, 1, 200, 5)]


@pytest.mark.parametrize("method,aw,ah,fw,fh,th,lh,sigma", BIG)
def test_noise_vs_model_and_reference_filter(method, aw, ah, fw, fh, th, lh, sigma):
    pic = M.noise_picture(aw, ah, sigma)
    want = M.detect_noise(method, pic, fw, fh, th, lh)
    with Ctx() as c:
        got = gpu_noise(c, method, [pic], fw, fh, th, lh)[0]
    check_noise(got, want)
    assert want["flags"].any() and not want["flags"].all()
    if method == M.HALF and (aw, ah) == (960, 540):
        assert want["sb_count"] == 32 * 60 and not want["flags"].reshape(34, 60)[32:].any()  # SB rows 32, 33 are never visited


@TP.needs_ref
@pytest.mark.parametrize("method,aw,ah,fw,fh,th,lh,sigma", BIG)
def test_filter_planes_vs_reference_leaf_functions(method, aw, ah, fw, fh, th, lh, sigma):
    """every sample of the optional planes against the reference's own filter, composed strip by strip as its loops do"""
    pic = M.noise_picture(aw, ah, sigma)
    rows, cols = (ah, aw) if method == M.FULL else ((ah // 64) * 64, (aw // 64) * 64)
    rden, rnoise = TP.ref_weak_filter(pic, rows)
    with Ctx() as c:
        _, _, den, noise = gpu_noise(c, method, [pic], fw, fh, th, lh)[0]
    assert np.array_equal(den[:rows, :cols], rden[:, :cols]) and np.array_equal(noise[:rows, :cols], rnoise[:, :cols])


@pytest.mark.parametrize("w,h,rw,rh", [(200, 136, 4, 4), (200, 136, 3, 2), (3840, 2160, 4, 4), (328, 200, 4, 4)])
def test_histograms_vs_model(w, h, rw, rh):
    import torch
    n, pad, cpad = 2, 68, 34
    dev = torch.device("cuda", 0)
    lumas = [M.noise_picture(w, h, s) for s in (8, 25)]
    cbs, crs = [M.gen_chroma(w // 2, h // 2, 1 + i) for i in range(n)], [M.gen_chroma(w // 2, h // 2, 5 + i) for i in range(n)]
    padded = [np.pad(l, pad, mode="edge") for l in lumas]
    d_full, d_16 = [_dev(p) for p in padded], [_dev(np.pad(l[::4, ::4], 16, mode="edge")) for l in lumas]
    d_cb, d_cr = [_dev(np.pad(a, cpad, mode="edge")) for a in cbs], [_dev(np.pad(a, cpad, mode="edge")) for a in crs]
    pics, pcb, pcr = (B.PaPicture * n)(), (B.Plane * n)(), (B.Plane * n)()
    for i in range(n):
        pics[i].full, pics[i].sixteenth = _plane(d_full[i], (h, w), pad), _plane(d_16[i], (h // 4, w // 4), 16)
        pcb[i], pcr[i] = _plane(d_cb[i], (h // 2, w // 2), cpad), _plane(d_cr[i], (h // 2, w // 2), cpad)
    with Ctx() as c:
        for scd in (0, 1):
            hist = [torch.full((rw * rh * 3 * 256,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
            avr = [torch.full((rw * rh * 3,), 0xCD, dtype=torch.uint8, device=dev) for _ in range(n)]
            avg = [torch.full((3,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(n)]
            B.check(c.lib.svt_hip_pa_histogram_batch_device(c.ctx, n, pics, pcb, pcr, rw, rh, scd, _ptrs(hist), _ptrs(avr), _ptrs(avg)))
            B.check(c.lib.svt_hip_ctx_synchronize(c.ctx))
            for i in range(n):
                mh, mr, ma = M.histograms(lumas[i][::4, ::4], cbs[i], crs[i], w, h, rw, rh, scd, padded[i])
                assert np.array_equal(hist[i].cpu().numpy().view(np.uint32).reshape(rw, rh, 3, 256), mh), (scd, i)
                assert np.array_equal(avr[i].cpu().numpy().reshape(rw, rh, 3), mr), (scd, i)
                assert list(avg[i].cpu().numpy()) == [a if a is not None else 0xEE for a in ma], (scd, i)
                assert int(mh.sum()) == ((256 * 3 * rw * rh + (w // 4) * (h // 4) + 2 * sum(
                    len(range(0, (rwo >> 1), 4)) * len(range(0, (rho >> 1), 4))
                    for rwo in [w // rw] * (rw - 1) + [w - (rw - 1) * (w // rw)] for rho in [h // rh] * (rh - 1) + [h - (rh - 1) * (h // rh)])) << 4)


@pytest.mark.parametrize("w,h", [(200, 136), (3840, 2160), (328, 200)])
def test_chroma_means_vs_model(w, h):
    import torch
    n, cpad = 2, 34
    dev = torch.device("cuda", 0)
    cbs, crs = [M.gen_chroma(w // 2, h // 2, 3 + i) for i in range(n)], [M.gen_chroma(w // 2, h // 2, 7 + i) for i in range(n)]
    d_cb, d_cr = [_dev(np.pad(a, cpad, mode="edge")) for a in cbs], [_dev(np.pad(a, cpad, mode="edge")) for a in crs]
    pcb, pcr = (B.Plane * n)(), (B.Plane * n)()
    for i in range(n):
        pcb[i], pcr[i] = _plane(d_cb[i], (h // 2, w // 2), cpad), _plane(d_cr[i], (h // 2, w // 2), cpad)
    nsb = T.n_sb(w, h)
    ocb = [torch.full((nsb * 21,), 0xCD, dtype=torch.uint8, device=dev) for _ in range(n)]
    ocr = [torch.full((nsb * 21,), 0xCD, dtype=torch.uint8, device=dev) for _ in range(n)]
    with Ctx() as c:
        B.check(c.lib.svt_hip_pa_chroma_mean_batch_device(c.ctx, n, pcb, pcr, w, h, _ptrs(ocb), _ptrs(ocr)))
        B.check(c.lib.svt_hip_ctx_synchronize(c.ctx))
    for i in range(n):
        mcb, mcr = M.chroma_means(cbs[i], crs[i], w, h)
        assert np.array_equal(ocb[i].cpu().numpy().reshape(nsb, 21), mcb) and np.array_equal(ocr[i].cpu().numpy().reshape(nsb, 21), mcr)
        assert mcb.any() and (w % 64 == 0 or not mcb.reshape(-1, (w + 63) // 64, 21)[:, -1].any())

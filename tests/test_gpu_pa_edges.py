"""Picture analysis on the GPU at the edges: batches of unlike pictures, contents at the ceilings of the arithmetic, planes with odd
origins and strides whose padding is noise, SB counts that leave a workgroup partly filled -- every output of the five entry points
(noise, histograms, chroma means, block mean / variance, padded planes) against the numpy model, the oracle and what the reference
recorded (tests/golden/pa_edges_reference.npz; tests/test_pa_edges.py pins the model and the oracle to it).

Every output is a slice of a larger device tensor with GUARD bytes of a pattern on both sides, which must come back unchanged; every
input plane lies inside a larger tensor of seeded noise, never at its edge.  Integer arithmetic: equality."""
import ctypes as C

import numpy as np
import pytest

import pa_stats_model as M
import svt_testlib as T
import test_pa as TPA
import test_pa_edges as E
from test_gpu_pa_stats import Ctx

B = T.B
pytestmark = pytest.mark.gpu
GUARD = 256


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


class Out:
    """`nbytes` of output at `off` bytes past a GUARD-byte band, another band behind it; everything holds a position-dependent pattern"""
    def __init__(self, nbytes, off=0):
        torch, dev = _torch()
        self.n, self.lo = nbytes, GUARD + off
        self.before = ((np.arange(self.lo + nbytes + GUARD, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8)
        self.t = torch.from_numpy(self.before).to(dev)
        self.ptr = self.t.data_ptr() + self.lo

    def get(self, dtype=np.uint8):
        """-> the output bytes, after checking that both guard bands are as they were"""
        a = self.t.cpu().numpy()
        assert np.array_equal(a[:self.lo], self.before[:self.lo]), "bytes before the output were written"
        assert np.array_equal(a[self.lo + self.n:], self.before[self.lo + self.n:]), "bytes behind the output were written"
        return a[self.lo:self.lo + self.n].view(dtype)

    def untouched(self):
        return self.before[self.lo:self.lo + self.n]


class In:
    """a host buffer `off` bytes past a GUARD-byte band of seeded noise on the device, another band behind it"""
    def __init__(self, buf, off=0, seed=0):
        torch, dev = _torch()
        a = np.random.default_rng(500 + seed).integers(0, 256, GUARD + off + buf.size + GUARD, dtype=np.uint8)
        a[GUARD + off:GUARD + off + buf.size] = buf.ravel()
        self.t = torch.from_numpy(a).to(dev)
        self.ptr = self.t.data_ptr() + GUARD + off

    def plane(self, buf, ox, oy, w, h):
        return B.Plane(self.ptr, buf.shape[1], ox, oy, w, h)


def _ptrs(outs):
    return (C.c_void_p * len(outs))(*[o.ptr for o in outs])


# ----------------------------------------------------------------------------------------------------------------------------------
# noise detection
# ----------------------------------------------------------------------------------------------------------------------------------
def gpu_noise(c, method, items, th, luma_height, want_planes=True):
    """items: (analysed picture, full width, full height, origin_x, origin_y, stride) of each batch entry, every entry with a geometry
    of its own -> list of (flags, result record, den, noise, untouched den, untouched noise)"""
    n = len(items)
    pics = (B.PaPicture * n)()
    name = ("full", "sixteenth", "quarter")[method]
    dummy = Out(16)
    ins, flags, den, noi = [], [], [], []
    for i, (p, fw, fh, ox, oy, stride) in enumerate(items):
        buf = M.hostile_plane(p, ox, oy, stride, i)
        ins.append(In(buf, i % 4, i))
        setattr(pics[i], name, ins[i].plane(buf, ox, oy, p.shape[1], p.shape[0]))
        if method != M.FULL:  # the full picture gives the SB grid only
            pics[i].full = B.Plane(dummy.ptr, fw, 0, 0, fw, fh)
        flags.append(Out(T.n_sb(fw, fh), i % 3))
        den.append(Out(p.size, i % 2))
        noi.append(Out(p.size, (i + 1) % 2))
    res = Out(16 * n)
    prm = B.PaNoiseParams(method, th, luma_height)
    B.check(c.lib.svt_hip_pa_noise_batch_device(c.ctx, n, pics, C.byref(prm), _ptrs(flags), C.c_void_p(res.ptr),
                                                _ptrs(den) if want_planes else None, _ptrs(noi) if want_planes else None))
    B.check(c.lib.svt_hip_ctx_synchronize(c.ctx))
    r = res.get().view(B.PA_NOISE_RESULT_DTYPE)
    return [(flags[i].get(), r[i], den[i].get().reshape(items[i][0].shape), noi[i].get().reshape(items[i][0].shape),
             den[i].untouched().reshape(items[i][0].shape), noi[i].untouched().reshape(items[i][0].shape)) for i in range(n)]


def check_noise(got, want, want_planes=True):
    flags, r, den, noise, den0, noise0 = got
    assert np.array_equal(flags, want["flags"])
    assert (int(r["pic_noise_class"]), int(r["sb_count"]), int(r["pic_noise_variance_sum"])) == \
        (want["pic_noise_class"], want["sb_count"], want["variance_sum"])
    rows, cols = want["region"] if want_planes else (0, 0)
    assert np.array_equal(den[:rows, :cols], want["den"][:rows, :cols]) and np.array_equal(noise[:rows, :cols], want["noise"][:rows, :cols])
    # outside the area the reference's loop filters (everywhere, without the optional planes) nothing is written
    assert np.array_equal(den[rows:], den0[rows:]) and np.array_equal(den[:, cols:], den0[:, cols:])
    assert np.array_equal(noise[rows:], noise0[rows:]) and np.array_equal(noise[:, cols:], noise0[:, cols:])


# (analysed width, height, full width, height) of each entry: full precision 1, 16, 6 and 6 tiles; half 6, 1 and 9; quarter 6, 1 and 6
UNLIKE_NOISE = {M.FULL: ((64, 64, 64, 64), (200, 196, 200, 196), (72, 136, 72, 136), (328, 64, 328, 64)),
                M.HALF: ((136, 72, 544, 288), (64, 64, 256, 256), (160, 136, 640, 544)),
                M.QUARTER: ((136, 72, 272, 144), (64, 64, 128, 128), (160, 136, 320, 272))}


@pytest.mark.parametrize("method", (M.FULL, M.HALF, M.QUARTER))
@pytest.mark.parametrize("want_planes", (True, False))
def test_noise_unlike_batch(method, want_planes):
    """one launch over pictures of unequal tile counts: the job lookup of every workgroup, flags and sums of each picture in its own place"""
    sigmas = (12, 5, 25, 8)
    items = [(M.noise_picture(aw, ah, sigmas[i]), fw, fh, 8 + i, 4 + 2 * i, aw + 2 * (8 + i) + (0, 3, 8, 5)[i])
             for i, (aw, ah, fw, fh) in enumerate(UNLIKE_NOISE[method])]
    with Ctx() as c:
        got = gpu_noise(c, method, items, 1, 1080, want_planes)
    some = []
    for g, (p, fw, fh, *_) in zip(got, items):
        want = M.detect_noise(method, p, fw, fh, 1, 1080)
        check_noise(g, want, want_planes)
        some.append(want["flags"])
    some = np.concatenate(some)
    assert (some == 1).any() and (some == 0).any()


@pytest.mark.parametrize("method", (M.FULL, M.HALF, M.QUARTER))
@pytest.mark.parametrize("th", (0, 1))
def test_noise_ceilings(method, th):
    """every ceiling picture in one batch, for a luma_height on each side of 720 and of 1080: model and recorded reference"""
    _, aw, ah, fw, fh = next(g for g in M.EDGE_NOISE_GEOMETRIES if g[0] == method)
    with Ctx() as c:
        for li, lh in enumerate(M.EDGE_LUMA_HEIGHTS):
            want = [E.edge_noise(kind, method, th, lh) for kind in M.LUMA_KINDS]
            got = gpu_noise(c, method, [(p, fw, fh, 16, 16, aw + 32) for p, _ in want], th, lh, want_planes=li != 1)
            for kind, g, (_, w) in zip(M.LUMA_KINDS, got, want):
                check_noise(g, w, li != 1)
                E.check_noise_vs_golden(kind, method, th, lh, g[0], int(g[1]["pic_noise_class"]), int(g[1]["pic_noise_variance_sum"]),
                                        int(g[1]["sb_count"]))


@pytest.mark.parametrize("method,aw,ah,fw,fh", [(M.FULL, 200, 136, 200, 136), (M.HALF, 160, 136, 640, 544), (M.QUARTER, 160, 136, 320, 272)])
def test_noise_odd_planes(method, aw, ah, fw, fh):
    """origins and strides that put the tile loads at every residue modulo 4; the padding is noise, so the clamped ring and the
    incomplete-tile path must read the picture alone"""
    items = []
    for i, ((ox, oy), slack) in enumerate(zip(((1, 3), (7, 2), (13, 9)), (1, 3, 6))):
        for p in (M.noise_picture(aw, ah, (8, 12, 25)[i]), M.edge_luma("random", aw, ah, i)):
            items.append((p, fw, fh, ox, oy, aw + 2 * ox + slack))
    with Ctx() as c:
        got = gpu_noise(c, method, items, 0, 1080)
    for g, (p, *_) in zip(got, items):
        check_noise(g, M.detect_noise(method, p, fw, fh, 0, 1080))


# ----------------------------------------------------------------------------------------------------------------------------------
# histograms and averages
# ----------------------------------------------------------------------------------------------------------------------------------
def gpu_histograms(c, cases, rw, rh, scd):
    """cases: (w, h, padded full luma buffer, (ox, oy), luma, cb, cr) per batch entry -> list of (hist, avg_region, avg, untouched avg)"""
    n = len(cases)
    pics, pcb, pcr = (B.PaPicture * n)(), (B.Plane * n)(), (B.Plane * n)()
    keep, hist, avr, avg = [], [], [], []
    for i, (w, h, buf, (ox, oy), luma, cb, cr) in enumerate(cases):
        b16 = M.hostile_plane(luma[::4, ::4], 5, 3, w // 4 + 13, 70 + i)
        bcb, bcr = M.hostile_plane(cb, 9, 5, w // 2 + 19, 80 + i), M.hostile_plane(cr, 3, 11, w // 2 + 9, 90 + i)
        ins = [In(buf, (i + 1) % 4, 4 * i), In(b16, i % 4, 4 * i + 1), In(bcb, (i + 2) % 4, 4 * i + 2), In(bcr, (i + 3) % 4, 4 * i + 3)]
        keep.append(ins)
        pics[i].full, pics[i].sixteenth = ins[0].plane(buf, ox, oy, w, h), ins[1].plane(b16, 5, 3, w // 4, h // 4)
        pcb[i], pcr[i] = ins[2].plane(bcb, 9, 5, w // 2, h // 2), ins[3].plane(bcr, 3, 11, w // 2, h // 2)
        hist.append(Out(rw * rh * 3 * 256 * 4))
        avr.append(Out(rw * rh * 3, i % 3))
        avg.append(Out(3, i % 2))
    B.check(c.lib.svt_hip_pa_histogram_batch_device(c.ctx, n, pics, pcb, pcr, rw, rh, scd, _ptrs(hist), _ptrs(avr), _ptrs(avg)))
    B.check(c.lib.svt_hip_ctx_synchronize(c.ctx))
    return [(hist[i].get(np.uint32).reshape(rw, rh, 3, 256), avr[i].get().reshape(rw, rh, 3), avg[i].get(), avg[i].untouched()) for i in range(n)]


def check_histograms(c, entries, rw, rh):
    """entries: (case index into EDGE_HIST_CASES + EDGE_HIST_MODEL_ONLY, chroma kind) of each batch entry, for scd_mode 0 and 1"""
    all_cases = M.EDGE_HIST_CASES + M.EDGE_HIST_MODEL_ONLY
    cases, keys = [], []
    for ci, kind in entries:
        k, luma, buf, origin, cb, cr = E.hist_case(ci, kind)
        assert all_cases[ci][2:] == (rw, rh)
        cases.append(all_cases[ci][:2] + (buf, origin, luma, cb, cr))
        keys.append(k if ci < len(M.EDGE_HIST_CASES) else None)
    for scd in (0, 1):
        got = gpu_histograms(c, cases, rw, rh, scd)
        for (w, h, buf, _, luma, cb, cr), k, (hist, avr, avg, avg0) in zip(cases, keys, got):
            mh, mr, ma = M.histograms(luma[::4, ::4], cb, cr, w, h, rw, rh, scd, buf)
            assert np.array_equal(hist, mh) and np.array_equal(avr, mr), (k, scd)
            assert list(avg) == [a if a is not None else int(avg0[i]) for i, a in enumerate(ma)], (k, scd)  # scd_mode 0 writes entry 0 alone
            if k is not None:  # the wrapped averages as the reference recorded them
                g = E.golden()
                assert np.array_equal(hist, g[k + "|hist"]) and np.array_equal(avr, g[k + f"|{scd}|avg_region"]), (k, scd)
                assert list(avg)[:1 if scd == 0 else 3] == list(g[k + f"|{scd}|avg"])[:1 if scd == 0 else 3], (k, scd)


@pytest.mark.parametrize("rw,rh", [(3, 2), (4, 4)])
def test_histograms_unlike_batch(rw, rh):
    """200x136, 72x40 and 328x200 in one call, saturated / zero / random chroma rotating through them"""
    cis = [i for i, c in enumerate(M.EDGE_HIST_CASES) if c[2:] == (rw, rh)]
    assert [M.EDGE_HIST_CASES[i][:2] for i in cis] == [(200, 136), (72, 40), (328, 200)]
    with Ctx() as c:
        for rot in range(3):
            check_histograms(c, [(ci, M.CHROMA_KINDS[(j + rot) % 3]) for j, ci in enumerate(cis)], rw, rh)


@pytest.mark.parametrize("ci", [len(M.EDGE_HIST_CASES) - 1, len(M.EDGE_HIST_CASES), len(M.EDGE_HIST_CASES) + 1])
def test_histograms_region_counts(ci):
    """1 x 1 regions; 8 x 8 on 200x136, where a luma region is 25 wide and the chroma origin (i * 25) >> 1 truncates; 5 x 3 on 328x200"""
    rw, rh = (M.EDGE_HIST_CASES + M.EDGE_HIST_MODEL_ONLY)[ci][2:]
    with Ctx() as c:
        check_histograms(c, [(ci, kind) for kind in M.CHROMA_KINDS], rw, rh)


# ----------------------------------------------------------------------------------------------------------------------------------
# chroma block means
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(M.EDGE_SB_SIZES)))
@pytest.mark.parametrize("kinds", (("random",), M.CHROMA_KINDS))
def test_chroma_means_partial_workgroups(si, kinds):
    """1, 3, 6 and 24 SBs, four to a workgroup: the n_sb * 21 outputs, and the guard bytes behind them"""
    w, h = M.EDGE_SB_SIZES[si]
    n, nsb = len(kinds), T.n_sb(w, h)
    pcb, pcr = (B.Plane * n)(), (B.Plane * n)()
    keep, ocb, ocr, want = [], [], [], []
    for i, kind in enumerate(kinds):
        k, cb, cr = E.cmean_case(si, kind)
        want.append((k, cb, cr))
        bcb, bcr = M.hostile_plane(cb, 7, 3, w // 2 + 14 + 1, 20 + i), M.hostile_plane(cr, 5, 9, w // 2 + 10 + 3, 30 + i)
        keep.append((In(bcb, 1 + i, i), In(bcr, 3 - i, 10 + i)))
        pcb[i], pcr[i] = keep[i][0].plane(bcb, 7, 3, w // 2, h // 2), keep[i][1].plane(bcr, 5, 9, w // 2, h // 2)
        ocb.append(Out(nsb * 21, i))
        ocr.append(Out(nsb * 21, 2 - i))
    with Ctx() as c:
        B.check(c.lib.svt_hip_pa_chroma_mean_batch_device(c.ctx, n, pcb, pcr, w, h, _ptrs(ocb), _ptrs(ocr)))
        B.check(c.lib.svt_hip_ctx_synchronize(c.ctx))
    for i, (k, cb, cr) in enumerate(want):
        got_cb, got_cr = ocb[i].get().reshape(nsb, 21), ocr[i].get().reshape(nsb, 21)
        mcb, mcr = M.chroma_means(cb, cr, w, h)
        assert np.array_equal(got_cb, mcb) and np.array_equal(got_cr, mcr), k
        assert np.array_equal(got_cb, E.golden()[k + "|cb"]) and np.array_equal(got_cr, E.golden()[k + "|cr"]), k


# ----------------------------------------------------------------------------------------------------------------------------------
# block mean and variance
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(M.EDGE_SB_SIZES)))
@pytest.mark.parametrize("kind", M.EDGE_MEANVAR_KINDS)
def test_mean_variance_partial_workgroups(si, kind):
    """the same SB counts through svt_pa_meanvar_kernel, all-255 and 0 | 255 blocks among the contents: oracle, numpy and reference"""
    w, h = M.EDGE_SB_SIZES[si]
    k, buf, ox, oy = E.meanvar_case(si, kind)
    nsb = T.n_sb(w, h)
    src, dm, dv = In(buf, 1 + si % 3, si), Out(nsb * 85, 1), Out(nsb * 85 * 2)
    pl = src.plane(buf, ox, oy, w, h)
    with Ctx() as c:
        B.check(c.lib.svt_hip_pa_mean_variance_device(c.ctx, C.byref(pl), C.c_void_p(dm.ptr), C.c_void_p(dv.ptr)))
        B.check(c.lib.svt_hip_ctx_synchronize(c.ctx))
    mean, var = dm.get().reshape(nsb, 85), dv.get(np.uint16).reshape(nsb, 85)
    for name, (wm, wv) in (("oracle", E.oracle_meanvar(buf, ox, oy, w, h)), ("numpy", TPA._numpy_meanvar(buf[oy:, ox:], 0, w, h)),
                           ("reference", (E.golden()[k + "|mean"], E.golden()[k + "|var"]))):
        assert np.array_equal(mean, wm) and np.array_equal(var, wv), (k, name)


# ----------------------------------------------------------------------------------------------------------------------------------
# padded and decimated planes
# ----------------------------------------------------------------------------------------------------------------------------------
PREPARE_SIZES = ((8, 8), (72, 64), (136, 72), (24, 16))
PREPARE_ORIGINS = ((36, 68), (20, 7), (9, 13))  # (origin_x, origin_y) of the full, quarter and sixteenth plane


@pytest.mark.parametrize("quarter", (1, 0))
def test_prepare_unlike_batch_odd_planes(quarter):
    """four sizes in one launch; source rows W + 13 apart starting 1, 2 and 3 bytes into their allocation; destination planes with
    origin_x != origin_y and a stride of width + 2 * origin_x + 5: every vector load and store at an address of any residue"""
    n = len(PREPARE_SIZES)
    outs, ptrs, strides = (B.PaPicture * n)(), (C.c_void_p * n)(), (C.c_int32 * n)()
    keep, dst, lumas = [], [], []
    for i, (w, h) in enumerate(PREPARE_SIZES):
        luma = M.edge_luma("random", w, h, 50 + i)
        src = M.hostile_plane(luma, 0, 0, w + 13, 50 + i)
        keep.append(In(src, 1 + i % 3, 50 + i))
        ptrs[i], strides[i] = keep[i].ptr, w + 13
        lumas.append((luma, src))
        planes = []
        for s, name in enumerate(("full", "quarter", "sixteenth")):
            (px, py), dw, dh = PREPARE_ORIGINS[s], w >> s, h >> s
            stride = dw + 2 * px + 5
            o = Out(stride * (dh + 2 * py), (i + s) % 4)
            setattr(outs[i], name, B.Plane(o.ptr, stride, px, py, dw, dh))
            planes.append((o, stride))
        dst.append(planes)
    with Ctx() as c:
        B.check(c.lib.svt_hip_pa_prepare_batch_device(c.ctx, n, ptrs, strides, outs, quarter))
        B.check(c.lib.svt_hip_ctx_synchronize(c.ctx))
    for i, (w, h) in enumerate(PREPARE_SIZES):
        luma, src = lumas[i]
        # the oracle on host planes of the same geometry (it copies whole rows of `stride` bytes up and down: the slack is its own)
        host = [np.zeros((o.n // stride, stride), np.uint8) for o, stride in dst[i]]
        d = B.PaPicture()
        for s, name in enumerate(("full", "quarter", "sixteenth")):
            setattr(d, name, B.Plane(host[s].ctypes.data, host[s].shape[1], *PREPARE_ORIGINS[s], w >> s, h >> s))
        assert T.oracle().svt_oracle_pa_prepare(src.ctypes.data_as(C.c_void_p), src.strides[0], C.byref(d), quarter) == 0
        for s in range(3):
            o, stride = dst[i][s]
            got, before = o.get().reshape(-1, stride), o.untouched().reshape(-1, stride)
            if s == 1 and not quarter:
                assert np.array_equal(got, before), (i, "the quarter plane was not asked for")
                continue
            (px, py), tw = PREPARE_ORIGINS[s], (w >> s) + 2 * PREPARE_ORIGINS[s][0]
            want = np.pad(luma[::1 << s, ::1 << s], ((py, py), (px, px)), mode="edge")
            assert np.array_equal(got[:, :tw], want), (i, s)
            assert np.array_equal(got[:, :tw], host[s][:, :tw]), (i, s, "oracle")
            assert np.array_equal(got[:, tw:], before[:, tw:]), (i, s, "stride slack written")

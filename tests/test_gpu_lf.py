"""GPU parity: HIP in-loop deblocking of whole frames (through the C ABI) vs the oracle, bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import svt_testlib as T

B = T.B
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


@pytest.mark.parametrize("w,h,seed", [(192, 128, 1), (200, 136, 2), (328, 200, 3), (64, 64, 4), (72, 72, 5), (648, 360, 7), (72, 136, 8)])
@pytest.mark.parametrize("sharp", [0, 4])
def test_lf_frame_vs_oracle(ctx, w, h, seed, sharp):
    case = T.make_lf_case(seed, w, h, sharp)
    o = T.oracle_lf_frame(case)
    g = T.hip_lf_frame(ctx, case)
    for n, a, b in zip("yuv", o, g):
        assert np.array_equal(a, b), (n, int(np.sum(a != b)), np.argwhere(a != b)[:6].tolist())
    assert np.mean(o[0] != case["y"]) > 0.02  # the filter really did something


def test_lf_y_only_and_repeatability(ctx):
    case = T.make_lf_case(9, 1280, 720)
    o = T.oracle_lf_frame(case, y_only=True)
    g = T.hip_lf_frame(ctx, case, y_only=True)
    assert np.array_equal(o[0], g[0]) and np.array_equal(g[1], case["u"]) and np.array_equal(g[2], case["v"])
    # the SB wavefront must give the same answer every time (ordering bugs show up as run-to-run differences)
    full = T.oracle_lf_frame(case)
    for _ in range(5):
        g = T.hip_lf_frame(ctx, case)
        assert all(np.array_equal(a, b) for a, b in zip(full, g))


@pytest.mark.parametrize("sizes", [((328, 200), (136, 64), (256, 192)),
                                   ((328, 200), (136, 64), (256, 192), (640, 360), (72, 72), (200, 136), (648, 264))])
def test_lf_batch_of_different_pictures(ctx, sizes):
    """svt_hip_lf_batch_device: pictures of different sizes (1 .. 6 SB rows; partial SBs) in one launch -- the persistent
    workgroups interleave their rows by ticket; every picture must come out as if filtered alone.  Three pictures run on the latency
    instance of the kernel (every SB row resident, seam rows handed to the row below early), seven on the throughput instance."""
    import torch
    lib = B.load()
    cases = [T.make_lf_case(21 + k, w, h) for k, (w, h) in enumerate(sizes)]
    n = len(cases)
    keep, descs = [], (B.YuvPlanes * n)()

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        keep.append(t)
        return t

    planes, lfms = [], []
    for k, c in enumerate(cases):
        y, u, v = dev(c["y"]), dev(c["u"]), dev(c["v"])
        planes.append((y, u, v))
        lfms.append(dev(c["lfm"]))
        d = descs[k]
        d.y, d.u, d.v = y.data_ptr(), u.data_ptr(), v.data_ptr()
        d.y_stride, d.uv_stride, d.width, d.height = c["y"].shape[1], c["u"].shape[1], c["y"].shape[1], c["y"].shape[0]
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in lfms])
    arr = lambda vals: (C.c_int32 * n)(*vals)
    B.check(lib.svt_hip_lf_batch_device(ctx, n, descs, ptrs, arr([c["lfm"].shape[1] for c in cases]), C.byref(cases[0]["thr"]),
                                        arr([c["mi_rows"] for c in cases]), arr([c["mi_cols"] for c in cases]), 0))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    for c, (y, u, v) in zip(cases, planes):
        oy, ou, ov = T.oracle_lf_frame(c)
        assert np.array_equal(y.cpu().numpy().reshape(oy.shape), oy)
        assert np.array_equal(u.cpu().numpy().reshape(ou.shape), ou) and np.array_equal(v.cpu().numpy().reshape(ov.shape), ov)


# ---------------------------------------------------------------------------------------------------------------------------------
# the extremes list (svt_testlib.LF_EXTREMES_CASES; what it reaches: tests/test_lf_census.py), planes inside padded buffers, thin and
# ragged pictures, refused alignments
# ---------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5
GUARD = 16  # guard rows above and below a plane, and at least as many columns left and right of it


def _diff(what, n, a, b):
    """assertion message (a string: pytest prints it whole): plane, number of differing samples, the first coordinates [row, column]"""
    return f"{what}: plane {n}, {int(np.sum(a != b))} differ, first at {np.argwhere(a != b)[:6].tolist()}"


@pytest.fixture(scope="module")
def extremes():
    """{case tuple: (case, the oracle's planes)}, computed once and left alone"""
    out = {}
    for c in T.LF_EXTREMES_CASES:
        case = T.make_lf_extremes_case(*c)
        out[c] = (case, T.oracle_lf_frame(case))
    return out


def test_lf_extremes_vs_reference_golden(ctx, extremes):
    """svt_hip_lf_frame on the random-walk pictures: the reference's own bytes (tests/golden/lf_extremes_reference.npz) and the oracle"""
    g = np.load(os.path.join(T.ROOT, "tests", "golden", "lf_extremes_reference.npz"))
    for c, (case, o) in extremes.items():
        got = T.hip_lf_frame(ctx, case)
        for n, a, b in zip("yuv", o, got):
            ref = g[n + "|" + T.lf_extremes_key(c)]
            assert np.array_equal(ref, b), _diff((c, "golden"), n, ref, b)
            assert np.array_equal(a, b), _diff((c, "oracle"), n, a, b)
        assert np.any(o[0] != case["y"])  # the filter did something (how much and what: tests/test_lf_census.py)


class _Padded:
    """one plane inside a larger device buffer full of SENTINEL: GUARD rows above and below, stride > width with stride % 8 == smod,
    sample (0, 0) at an address that is amod modulo 8 (smod, amod in {0, 4} are what the launcher accepts besides 8-byte alignment;
    skew puts a refused, non-multiple-of-4 address or stride there instead)"""

    def __init__(self, plane, smod, amod, skew_addr=0, skew_stride=0):
        import torch
        self.h, self.w = plane.shape
        self.stride = (self.w + 2 * GUARD + 7) // 8 * 8 + smod + skew_stride
        self.host = np.full((self.h + 2 * GUARD + 1) * self.stride + 16, SENTINEL, np.uint8)
        self.buf = torch.empty(self.host.size, dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        self.off = GUARD * self.stride + GUARD
        self.off += (amod - (base + self.off)) % 8 + skew_addr
        assert (base + self.off) % 8 == (amod + skew_addr) % 8 and self.stride % 8 == (smod + skew_stride) % 8
        assert self.off % self.stride >= GUARD and self.stride - self.off % self.stride - self.w >= GUARD - 8
        self.ptr = base + self.off
        self.view()[:] = plane
        self.buf.copy_(torch.from_numpy(self.host))

    def view(self, flat=None):
        flat = self.host if flat is None else flat
        return np.lib.stride_tricks.as_strided(flat[self.off:], (self.h, self.w), (self.stride, 1))

    def check(self, want, what, n):
        """the interior is `want`, every other byte of the buffer is still SENTINEL"""
        got = self.buf.cpu().numpy()
        inner = self.view(got)
        assert np.array_equal(inner, want), _diff(what, n, want, inner)
        outside = got.copy()
        self.view(outside)[:] = SENTINEL
        bad = np.flatnonzero(outside != SENTINEL)
        assert bad.size == 0, f"{what}: plane {n}, {bad.size} bytes outside the picture changed, first at (row, column) {[divmod(int(i) - self.off, self.stride) for i in bad[:6]]}"


def _padded_desc(d, case, py, pu, pv):
    d.y, d.u, d.v = py.ptr, pu.ptr, pv.ptr
    d.y_stride, d.uv_stride, d.width, d.height = py.stride, pu.stride, case["y"].shape[1], case["y"].shape[0]


def _dev_lfm(case):
    import torch
    return torch.from_numpy(np.ascontiguousarray(case["lfm"]).view(np.uint8).reshape(-1)).cuda()


@pytest.fixture(scope="module")
def geometry_cases():
    """136x72: chroma width 68 = 4 mod 8 (the last SB holds 4 chroma columns); 128x72: 0 mod 8"""
    out = []
    for seed, w, h in ((31, 136, 72), (32, 128, 72)):
        case = T.make_lf_extremes_case(seed, w, h, 0, seed & 1)
        out.append((case, T.oracle_lf_frame(case)))
    return out


def test_lf_padded_offset_planes(ctx, geometry_cases):
    """svt_hip_lf_frame_device as the encode pass calls it: planes inside padded pictures.  Every accepted combination of stride and
    origin alignment (0 or 4 modulo 8, luma and chroma independently) x chroma width 0 or 4 modulo 8: the interior equals the oracle on
    tight planes and not one byte outside width x height changes.  The copy unit (8 or 4 bytes) follows the alignment; a chroma width
    of 4 modulo 8 must not take the 8-byte unit."""
    lib = B.load()
    for case, o in geometry_cases:
        lfm = _dev_lfm(case)
        for ys, ya, cs, ca in [(a, b, c, d) for a in (0, 4) for b in (0, 4) for c in (0, 4) for d in (0, 4)]:
            what = (case["y"].shape[::-1], "y stride/origin mod 8", ys, ya, "uv", cs, ca)
            pl = [_Padded(case["y"], ys, ya), _Padded(case["u"], cs, ca), _Padded(case["v"], cs, ca)]
            d = B.YuvPlanes()
            _padded_desc(d, case, *pl)
            B.check(lib.svt_hip_lf_frame_device(ctx, C.byref(d), C.c_void_p(lfm.data_ptr()), case["lfm"].shape[1], C.byref(case["thr"]),
                                                case["mi_rows"], case["mi_cols"], 0))
            B.check(lib.svt_hip_ctx_synchronize(ctx))
            for n, p, want in zip("yuv", pl, o):
                p.check(want, what, n)


def test_lf_padded_planes_in_a_batch(ctx):
    """the same through svt_hip_lf_batch_device: pictures of different geometry in one launch, 8-byte aligned strides and origins, chroma
    widths 100, 68 (4 columns in the last SB) and 44 (12 columns in the last SB)"""
    lib = B.load()
    cases = [T.make_lf_extremes_case(41 + k, w, h, 0, k & 1) for k, (w, h) in enumerate(((200, 136), (136, 72), (88, 72)))]
    n = len(cases)
    descs, lfms, planes = (B.YuvPlanes * n)(), [_dev_lfm(c) for c in cases], []
    for k, c in enumerate(cases):
        planes.append([_Padded(c[p], 0, 0) for p in "yuv"])
        _padded_desc(descs[k], c, *planes[k])
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in lfms])
    arr = lambda vals: (C.c_int32 * n)(*vals)
    B.check(lib.svt_hip_lf_batch_device(ctx, n, descs, ptrs, arr([c["lfm"].shape[1] for c in cases]), C.byref(cases[0]["thr"]),
                                        arr([c["mi_rows"] for c in cases]), arr([c["mi_cols"] for c in cases]), 0))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    for c, pl in zip(cases, planes):
        for nm, p, want in zip("yuv", pl, T.oracle_lf_frame(c)):
            p.check(want, c["y"].shape[::-1], nm)


def test_lf_thin_and_ragged_pictures(ctx, extremes):
    """5 blocks in the only SB row / column (104x40, 40x104) and pictures one block high / wide (72x8: one band, 4 chroma rows; 8x72): the
    launcher takes them all (tight planes: a chroma stride of 4 bytes for the 8-wide picture)"""
    for size in ((104, 40), (40, 104), (72, 8), (8, 72)):
        (c,) = [c for c in extremes if (c[1], c[2]) == size]
        case, o = extremes[c]
        for n, a, b in zip("yuv", o, T.hip_lf_frame(ctx, case)):
            assert np.array_equal(a, b), _diff(size, n, a, b)
        o1 = T.oracle_lf_frame(case, y_only=True)
        g1 = T.hip_lf_frame(ctx, case, y_only=True)
        assert all(np.array_equal(a, b) for a, b in zip(o1, g1)), (size, "y_only")


def test_lf_rejects_misaligned_planes(ctx, geometry_cases):
    """a plane address or a stride that is no multiple of 4 is refused with SVT_HIP_ERR_BAD_PARAMETER before anything is launched: the
    buffers keep their content, padding included"""
    lib = B.load()
    case, _ = geometry_cases[0]
    lfm = _dev_lfm(case)
    SVT_HIP_ERR_BAD_PARAMETER = -1
    ok, addr1, addr2, addr3, stride2 = {}, dict(skew_addr=1), dict(skew_addr=2), dict(skew_addr=3), dict(skew_stride=2)
    # per plane (y, u, v); the two chroma planes share one stride
    for skew in ((addr2, ok, ok), (addr1, ok, ok), (stride2, ok, ok), (ok, addr2, ok), (ok, ok, addr3), (ok, stride2, stride2)):
        pl = [_Padded(case[p], 0, 0, **k) for p, k in zip("yuv", skew)]
        d = B.YuvPlanes()
        _padded_desc(d, case, *pl)
        rc = lib.svt_hip_lf_frame_device(ctx, C.byref(d), C.c_void_p(lfm.data_ptr()), case["lfm"].shape[1], C.byref(case["thr"]),
                                         case["mi_rows"], case["mi_cols"], 0)
        assert rc == SVT_HIP_ERR_BAD_PARAMETER, f"{skew}: rc {rc}"
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        for p, src in zip(pl, "yuv"):
            p.check(case[src], skew, src)

"""GPU parity: HIP inter prediction (8-tap motion compensation, through the C ABI) vs the oracle and the golden
fixture produced by the reference's own inter_prediction(), bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import mc_model as M
import svt_testlib as T
from gen_golden import MC_GOLDEN_CASES

B = T.B
pytestmark = pytest.mark.gpu
GOLD = os.path.join(T.GOLDEN_DIR, "mc_reference.npz")


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


def _same(a, b):
    for name, x, y in zip("yuv", a, b):
        assert np.array_equal(x, y), (name, int(np.sum(x != y)), np.argwhere(x != y)[:6].tolist())


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("use_subpel", [1, 0])
def test_mc_vs_oracle(ctx, seed, use_subpel):
    case = T.make_mc_case(seed, use_subpel=use_subpel)
    _same(T.hip_mc_frame(ctx, case), T.oracle_mc_frame(case))


@pytest.mark.parametrize("w,h", [(64, 64), (136, 72), (264, 200), (520, 264)])
def test_mc_ragged_sizes_and_far_mvs(ctx, w, h):
    """pictures that are not multiples of 64 (partial superblocks, partial 32-unit workgroups) and MVs that the
    reference clamps to the picture border"""
    case = T.make_mc_case(31 + w, width=w, height=h, mv_range=600)
    _same(T.hip_mc_frame(ctx, case), T.oracle_mc_frame(case))


@pytest.mark.parametrize("seed,w,h,sub", MC_GOLDEN_CASES)
def test_mc_vs_reference_golden(ctx, seed, w, h, sub):
    g = np.load(GOLD)
    case = T.make_mc_case(seed, width=w, height=h, use_subpel=sub)
    got = T.hip_mc_frame(ctx, case)
    my, mc = T.mc_inter_masks(case)
    for p, a, m in zip("yuv", got, (my, mc, mc)):
        assert np.array_equal(a[m], g[f"{p}|{seed}|{w}|{h}|{sub}"][m]), p
        assert (a[~m] == 0x5A).all()


def test_mc_all_phases_every_block_size(ctx):
    """every (x, y) filter phase pair on every square block size: 256 phase pairs spread over the blocks"""
    case = T.make_mc_case(77, width=512, height=256, rect=False, intra_share=0.0)
    mi = case["mi"]
    k = 0
    for r in range(case["mi_rows"]):
        for c in range(case["mi_cols"]):
            if r % mi[r, c]["bh8"] == 0 and c % mi[r, c]["bw8"] == 0:
                h8, w8 = int(mi[r, c]["bh8"]), int(mi[r, c]["bw8"])
                mi[r:r + h8, c:c + w8]["mv_row"] = (((k >> 4) & 15) - 40, (k & 15) + 24)       # 1/8 sample: 16 phases each ...
                mi[r:r + h8, c:c + w8]["mv_col"] = ((k & 15) + 16, ((k >> 4) & 15) - 56)
                k += 1
    cen = M.mc_census(case)
    assert len({(c[6], c[7]) for c in cen if c[0] == 1}) == 256   # the MVs above do give chroma all 16 x 16 (sx, sy) pairs
    _same(T.hip_mc_frame(ctx, case), T.oracle_mc_frame(case))


def test_mc_batch_device_two_pictures(ctx):
    """svt_hip_inter_pred_batch_device: two pictures of different sizes in one launch, device pointers"""
    import torch
    lib = B.load()
    cases = [T.make_mc_case(41, width=192, height=128), T.make_mc_case(42, width=136, height=72, use_subpel=0)]
    keep, pics = [], (B.McPicture * 2)()

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        keep.append(t)
        return t

    outs = []
    for i, case in enumerate(cases):
        W, H, pad = case["width"], case["height"], case["pad"]
        pics[i].d_mi = dev(case["mi"]).data_ptr()
        pics[i].mi_stride, pics[i].mi_rows, pics[i].mi_cols, pics[i].use_subpel = case["mi_cols"], case["mi_rows"], case["mi_cols"], case["use_subpel"]
        for l, (y, u, v) in enumerate(case["refs"]):
            ty, tu, tv = dev(y), dev(u), dev(v)
            r = pics[i].ref[l]
            r.y = ty.data_ptr() + pad * y.shape[1] + pad
            r.u = tu.data_ptr() + (pad // 2) * u.shape[1] + pad // 2
            r.v = tv.data_ptr() + (pad // 2) * v.shape[1] + pad // 2
            r.y_stride, r.uv_stride, r.width, r.height = y.shape[1], u.shape[1], W, H
        o = [dev(np.full((H, W), 0x5A, np.uint8)), dev(np.full((H // 2, W // 2), 0x5A, np.uint8)), dev(np.full((H // 2, W // 2), 0x5A, np.uint8))]
        outs.append(o)
        p = pics[i].pred
        p.y, p.u, p.v, p.y_stride, p.uv_stride, p.width, p.height = o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), W, W // 2, W, H
    B.check(lib.svt_hip_inter_pred_batch_device(ctx, 2, pics))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    for case, o in zip(cases, outs):
        W, H = case["width"], case["height"]
        got = [o[0].cpu().numpy().reshape(H, W), o[1].cpu().numpy().reshape(H // 2, W // 2), o[2].cpu().numpy().reshape(H // 2, W // 2)]
        _same(got, T.oracle_mc_frame(case))


# ---- constructed cases: wave shortcuts, phases x load shifts, filter ceilings, clamp bounds, thin pictures ----------------------
@pytest.mark.parametrize("name", T.MC_EDGE_CASES)
def test_mc_edge_cases_vs_oracle(ctx, name):
    """what each case reaches is asserted on the CPU by tests/test_mc_model.py"""
    for case in T.make_mc_edge_case(name):
        got, exp = T.hip_mc_frame(ctx, case), T.oracle_mc_frame(case)
        for p, a, b, m in zip("yuv", got, exp, _masks3(case)):
            assert np.array_equal(a, b), (case["key"], p, int(np.sum(a != b)), np.argwhere(a != b)[:6].tolist())
            assert (a[~m] == 0x5A).all(), (case["key"], p)


@pytest.mark.parametrize("name", T.MC_EDGE_CASES)
def test_mc_edge_cases_vs_reference_golden(ctx, name):
    g = np.load(T.MC_EDGE_GOLD)
    for case, ref in zip(T.make_mc_edge_case(name), T.mc_edge_unpack(g, name)):
        got = T.hip_mc_frame(ctx, case)
        for p, a, b, m in zip("yuv", got, ref, _masks3(case)):
            assert np.array_equal(a[m], b[m]), (case["key"], p)
            assert (a[~m] == 0x5A).all(), (case["key"], p)


def _masks3(case):
    my, mc = T.mc_inter_masks(case)
    return my, mc, mc


# ---- the device form: strided and offset planes, batches, rejections -----------------------------------------------------------
GUARD = 0x5A
SLACK_MV = (24, -40)  # the MV of the records between mi_cols and mi_stride


class DevicePictures:
    """McPicture descriptors of cases for svt_hip_inter_pred_batch_device, every buffer laid out on request:
    pred_pad = (extra bytes of y_stride, of uv_stride, k): prediction planes inside slabs filled with GUARD, two rows above and below,
               sample (0, 0) 4 k bytes into its row
    mi_slack: mi_stride - mi_cols; the slack records are valid 8x8 inter blocks with SLACK_MV, so that a wrong stride gives wrong
              samples while every read stays where a valid grid sends it
    ref_mod[l] = (stride mod 4, address of the padded plane's first byte mod 4) of list l; the bytes between the rows' ends and the
                 stride, and 64 bytes before and after the plane, are noise"""

    def __init__(self, cases, pred_pad=(0, 0, 0), mi_slack=0, ref_mod=((0, 0), (0, 0))):
        import torch
        self.torch, self.cases, self.keep, self.slabs = torch, cases, [], []
        self.pics = (B.McPicture * len(cases))()
        rng = np.random.default_rng(5)
        for i, case in enumerate(cases):
            W, H, pad, pic = case["width"], case["height"], case["pad"], self.pics[i]
            mi = np.zeros((case["mi_rows"], case["mi_cols"] + mi_slack), dtype=B.MC_MODE_INFO_DTYPE)
            mi["bw8"], mi["bh8"], mi["ref_list"] = 1, 1, (0, -1)
            mi["mv_row"], mi["mv_col"] = SLACK_MV[0], SLACK_MV[1]
            mi[:, :case["mi_cols"]] = case["mi"]
            pic.d_mi = self._dev(mi.view(np.uint8).reshape(-1)).data_ptr()
            pic.mi_stride, pic.mi_rows, pic.mi_cols, pic.use_subpel = case["mi_cols"] + mi_slack, case["mi_rows"], case["mi_cols"], case["use_subpel"]
            for l, planes in enumerate(case["refs"]):
                smod, bmod = ref_mod[l]
                ptrs, strides = [], []
                for s, a in zip((0, 1, 1), planes):
                    stride = a.shape[1] + (smod - a.shape[1]) % 4
                    rows = rng.integers(0, 256, (a.shape[0], stride), dtype=np.uint8)
                    rows[:, :a.shape[1]] = a
                    lead = 64 + bmod
                    t = self._dev(np.concatenate([rng.integers(0, 256, lead, dtype=np.uint8), rows.reshape(-1), rng.integers(0, 256, 64, dtype=np.uint8)]))
                    assert t.data_ptr() % 4 == 0
                    ptrs.append(t.data_ptr() + lead + (pad >> s) * stride + (pad >> s))
                    strides.append(stride)
                r = pic.ref[l]
                r.y, r.u, r.v, r.y_stride, r.uv_stride, r.width, r.height = ptrs[0], ptrs[1], ptrs[2], strides[0], strides[1], W, H
                assert strides[1] == strides[2]
            ey, euv, k = pred_pad
            slabs = []
            for s, extra in zip((0, 1, 1), (ey, euv, euv)):
                stride = (W >> s) + extra
                assert 4 * k + (W >> s) <= stride
                t = self._dev(np.full(((H >> s) + 4, stride), GUARD, np.uint8).reshape(-1))
                slabs.append((t, stride, 2 * stride + 4 * k))
            self.slabs.append(slabs)
            p = pic.pred
            p.y, p.u, p.v = (t.data_ptr() + org for t, _, org in slabs)
            p.y_stride, p.uv_stride, p.width, p.height = slabs[0][1], slabs[1][1], W, H
        self.pred_pad = pred_pad

    def _dev(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.keep.append(t)
        return t

    def slab_arrays(self, i):
        return [t.cpu().numpy().reshape(-1, stride) for t, stride, _ in self.slabs[i]]

    def assert_untouched(self):
        for i in range(len(self.cases)):
            for a in self.slab_arrays(i):
                assert (a == GUARD).all()

    def assert_equal_oracle(self):
        """the picture rectangle is the oracle's prediction (GUARD where a unit is not inter); every other byte of the slab is GUARD"""
        k = self.pred_pad[2]
        for i, case in enumerate(self.cases):
            exp = T.oracle_mc_frame(case)
            inter = T.mc_inter_masks(case)
            for p, a, e, m in zip("yuv", self.slab_arrays(i), exp, (inter[0], inter[1], inter[1])):
                want = np.full_like(a, GUARD)
                want[2:2 + e.shape[0], 4 * k:4 * k + e.shape[1]] = e
                assert (e[~m] == GUARD).all()
                assert np.array_equal(a, want), (i, case.get("key"), p, int(np.sum(a != want)), np.argwhere(a != want)[:6].tolist())


def _run(ctx, dp, n=None):
    lib = B.load()
    rc = lib.svt_hip_inter_pred_batch_device(ctx, len(dp.cases) if n is None else n, dp.pics)
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    return rc


def _strided_cases():
    """pictures of the constructed cases that between them hold every wave mode, phase and shift, clamped blocks of the largest and
    smallest size, intra units, and a picture narrower than a workgroup"""
    clamps = T.make_mc_edge_case("clamps")
    by_key = {c["key"]: c for c in clamps}
    return [T.make_mc_edge_case("phases")[0], T.make_mc_edge_case("wave_modes")[0], by_key["clamps|8x8|0|1"], by_key["clamps|8x8|1|0"], by_key["clamps|1x1|0|1"],
            T.make_mc_case(9, width=136, height=72, mv_range=600), T.make_mc_edge_case("thin")[0]]


@pytest.mark.parametrize("smod,bmod,k", [(1, 1, 1), (2, 3, 2), (3, 2, 3), (0, 0, 0)])
def test_mc_device_form_strided_and_offset(ctx, smod, bmod, k):
    """prediction planes inside guarded slabs with strides beyond the width, mi_stride beyond mi_cols, reference strides and base
    addresses of every residue modulo 4 (so every load shift moves), the two lists laid out differently"""
    cases = _strided_cases()
    assert any((c["mi"]["ref_list"][:, :, 0] < 0).any() for c in cases)
    other = (smod % 3 + 1, bmod % 3 + 1)
    dp = DevicePictures(cases, pred_pad=(12, 20, k), mi_slack=3, ref_mod=((smod, bmod), other))
    assert _run(ctx, dp) == 0
    dp.assert_equal_oracle()


def test_mc_batch_five_pictures_of_unequal_width(ctx):
    """2, 1, 1, 3 and 1 workgroups per mode-info row in one launch whose work-item count (3 x 25 x 5) is no multiple of 8; the
    smallest picture is neither first nor last"""
    dims = ((264, 72), (8, 8), (136, 200), (520, 40), (64, 64))
    cases = [T.make_mc_case(60 + i, width=w, height=h, mv_range=48 if i % 2 else 600, use_subpel=1 - (i == 2)) for i, (w, h) in enumerate(dims)]
    assert [(c["mi_cols"] + 31) // 32 for c in cases] == [2, 1, 1, 3, 1]
    xblocks, max_rows = max((c["mi_cols"] + 31) // 32 for c in cases), max(c["mi_rows"] for c in cases)
    assert (xblocks * max_rows * len(cases)) % 8
    dp = DevicePictures(cases, pred_pad=(12, 20, 1), mi_slack=3, ref_mod=((1, 2), (3, 1)))
    assert _run(ctx, dp) == 0
    dp.assert_equal_oracle()


def test_mc_batch_32_pictures(ctx):
    """the largest batch the encode pass sends: 32 pictures with distinct grids and references"""
    cases, grids, seed = [], set(), 100
    while len(cases) < 32:      # a 64x64 picture can be one block: seeds that repeat a grid are passed over
        case = T.make_mc_case(seed, width=64, height=64, use_subpel=int(len(cases) % 4 != 3))
        seed += 1
        if case["mi"].tobytes() not in grids:
            grids.add(case["mi"].tobytes())
            cases.append(case)
    assert seed < 140
    dp = DevicePictures(cases, pred_pad=(12, 20, 2), mi_slack=1, ref_mod=((2, 1), (0, 3)))
    assert _run(ctx, dp) == 0
    dp.assert_equal_oracle()


def test_mc_batch_rejects_bad_descriptors(ctx):
    """SVT_HIP_ERR_BAD_PARAMETER, nothing written, and the context still good for the next call"""
    cases = [T.make_mc_case(51, width=64, height=64), T.make_mc_case(52, width=72, height=40)]
    dp = DevicePictures(cases, pred_pad=(12, 20, 1), mi_slack=3, ref_mod=((1, 1), (2, 3)))

    def bad(edit, n=None):
        saved = bytes(dp.pics)
        edit(dp.pics[1])
        rc = _run(ctx, dp, n)
        C.memmove(dp.pics, saved, len(saved))
        assert rc == -1, rc     # SVT_HIP_ERR_BAD_PARAMETER
        dp.assert_untouched()

    for plane in "yuv":
        for skew in (1, 2, 3):
            bad(lambda p: setattr(p.pred, plane, getattr(p.pred, plane) + skew))
    for stride in ("y_stride", "uv_stride"):
        for skew in (1, 2):
            bad(lambda p: setattr(p.pred, stride, getattr(p.pred, stride) + skew))
    bad(lambda p: setattr(p, "mi_stride", p.mi_cols - 1))
    for l in (0, 1):
        for plane in "yuv":
            bad(lambda p: setattr(p.ref[l], plane, None))
    bad(lambda p: None, n=0)
    bad(lambda p: None, n=-1)
    assert _run(ctx, dp) == 0
    dp.assert_equal_oracle()

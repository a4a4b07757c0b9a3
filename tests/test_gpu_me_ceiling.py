"""GPU parity at the ceilings of the ME kernels' packed arithmetic: HIP == the oracle run one call per SB (svt_testlib.oracle_me_picture_per_sb),
bit-exact in every field me_results_equal compares plus the rate-control SADs, on the pictures of tests/me_ceiling.py -- sums of N samples at
N * 255, 0.4 % below the capacity of the 16-bit halves, the (sad << 16 | position) / (sad << 12 | position) keys and the signed packed half-pel
filter the device forms rely on (most of them exist on the device only: the host emulation cannot stand in).  tests/test_me_ceiling.py proves,
without the kernels, that the pictures reach those values.  The neighbours of ME that share the primitives (the stand-alone SAD search, the
zero-motion SAD, the SB statistics) get the same pictures against their own oracles."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import me_ceiling as K
import me_configs as MC
import svt_testlib as T
from test_gpu_me import hip_me_picture
from test_me_ceiling import LISTS_LAYERS, params, pics_of

B = T.B
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


def check(ctx, pics, p, nl, what=None):
    ref1 = pics[2] if nl == 2 else None
    o, orc = T.oracle_me_picture_per_sb(pics[1], pics[0], ref1, p)
    g, grc = hip_me_picture(ctx, pics[1], pics[0], ref1, p)
    bad = T.me_results_equal(o, g, nl)
    if bad:
        idx = np.argwhere(o[bad[0]] != g[bad[0]])
        detail = [(int(sb), int(pu), o[sb, pu].tolist()[:11], g[sb, pu].tolist()[:11]) for sb, pu in idx[:4]]
        raise AssertionError(f"{what}: {bad} mismatches={len(idx)} first={idx[:16].tolist()} detail={detail}")
    assert np.array_equal(orc, grc), (what, "rate-control SADs", np.argwhere(orc != grc)[:8].tolist())


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(MC.PRESETS))
@pytest.mark.parametrize("kind", K.KINDS)
def test_me_presets_at_the_ceiling(ctx, kind, name, size):
    pics = pics_of(kind, size)
    for nl, tl in LISTS_LAYERS:
        check(ctx, pics, params(name, nl, tl), nl, (kind, name, size, nl, tl))


@pytest.mark.parametrize("wh", [(64, 32), (48, 48), (32, 64), (64, 64), (40, 56), (16, 127)])
@pytest.mark.parametrize("kind", ["black_white", "dented", "blocks", "taps"])
def test_me_c5_large_areas_at_the_ceiling(ctx, kind, wh):
    """BASELINE C5 (SSD refinement, every PU refined) with the search areas of test_me_large_search_areas_full_pel_layouts: both fused full-pel
    layouts (the 16x16-PU one walking runs, the 8x8-block one with two groups per iteration), and on the partial SBs of 200 x 136, whose clipped
    areas have tail columns, the unfused sad8 / sum16 / sum32 path; both 8x8 modes, the three fractional-search metrics."""
    pics = pics_of(kind, K.SIZES[0])
    for nl, tl in ((2, 2), (1, 0)):
        for cu8 in (0, 1):
            for method in (0, 1, 2):
                p = MC.preset_c5(nl, tl)
                p.search_area_width, p.search_area_height = wh
                p.cu8x8_mode, p.fractional_search_method = cu8, method
                check(ctx, pics, p, nl, (kind, wh, nl, tl, cu8, method))


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ["dented", "hme"])
def test_me_variants_at_the_ceiling(ctx, kind, size):
    pics = pics_of(kind, size)
    for nl, tl in ((1, 0), (2, 2)):
        for variant in (MC.variant_full_sad_all_pus, MC.variant_l0_only_4quadrants, MC.variant_wide_search):
            check(ctx, pics, variant(nl, tl), nl, (kind, variant.__name__, nl, tl))
    for tl in (1, 3):
        check(ctx, pics, MC.variant_same_poc(tl), 2, (kind, "variant_same_poc", tl))


def check_whole_columns_size(ctx, want_instance):
    """every kind at the size of whole SB columns with the 2160p enc-mode-8 preset; want_instance: what svt_hip_me_last_instance has to report"""
    lib = B.load()
    lib.svt_hip_me_last_instance.argtypes = [C.c_void_p]
    for kind in K.KINDS:
        pics = pics_of(kind, K.SIZE_FAST)
        for nl, tl in LISTS_LAYERS:
            check(ctx, pics, MC.preset("c3_2160p_m8", nl, tl), nl, (kind, K.SIZE_FAST, nl, tl, want_instance))
            inst = lib.svt_hip_me_last_instance(ctx)
            assert (inst == 101) == (want_instance == 101), (kind, nl, tl, inst)


def test_me_specialised_instance_at_the_ceiling(ctx):
    """csrc/me_fast.h's driver (instance 101 serves pictures of whole SB columns with the 2160p enc-mode-8 parameters)"""
    assert not os.environ.get("SVT_HIP_ME_NOFAST")
    check_whole_columns_size(ctx, 101)


def test_me_generic_instance_at_the_ceiling_same_pictures():
    """the same pictures through the generic driver (SVT_HIP_ME_NOFAST; a fresh process: the choice is latched at the first launch)"""
    code = ("import sys; sys.path.insert(0, 'tests'); import ctypes as C; import svt_testlib as T, test_gpu_me_ceiling as G; B = T.B; lib = B.load();"
            "c = C.c_void_p(); B.check(lib.svt_hip_ctx_create(C.byref(c), 0)); G.check_whole_columns_size(c, 0); lib.svt_hip_ctx_destroy(c); print('CEILING OK')")
    env = dict(os.environ)
    env["SVT_HIP_ME_NOFAST"] = "1"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CEILING OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("size", [(256, 192), K.SIZES[0]], ids=lambda s: "%dx%d" % s)
def test_me_batch_layers_mixing_ceiling_and_ordinary_pictures(ctx, size):
    """svt_hip_me_batch_layers_device: one launch holding black_white, dented and a smooth clip, with different list counts / layers per picture
    -- a picture's sums must not depend on the picture beside it (256 x 192: the specialised driver; 200 x 136: the generic one)"""
    import torch
    lib = B.load()
    dev = torch.device("cuda", 0)
    w, h = size
    bw, dent, smooth = K.content("black_white", w, h), K.content("dented", w, h), T.gen_clip_subpel(w, h, 3, 31)
    pool = [T.PaPic(f) for f in (bw[0], bw[1], dent[1], smooth[0], smooth[1], smooth[2])]
    keep = []

    def dev_desc(pa):
        d = B.PaPicture()
        for name, (a, pad) in zip(("full", "quarter", "sixteenth"), pa.planes()):
            t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            keep.append(t)
            pl = B.Plane()
            pl.buf, pl.stride, pl.origin_x, pl.origin_y = t.data_ptr(), t.shape[1], pad, pad
            pl.width, pl.height = t.shape[1] - 2 * pad, t.shape[0] - 2 * pad
            setattr(d, name, pl)
        return d

    d = [dev_desc(p_) for p_ in pool]
    nsb = T.n_sb(w, h)
    # cur, ref0, ref1, (lists, layer, same_poc): ceiling pictures beside ordinary ones, and a smooth picture predicted from a black one
    cases = [(1, 0, 0, (2, 0, 0)), (4, 3, 5, (2, 2, 0)), (2, 0, 0, (1, 3, 0)), (4, 3, 5, (1, 0, 0)), (2, 0, 0, (2, 1, 0)), (4, 0, 3, (2, 4, 0)), (1, 0, 0, (2, 3, 1))]
    n = len(cases)
    prm = (B.MeParams * n)()
    for i, (_, _, _, (nl, tl, sp)) in enumerate(cases):
        p = MC.preset("c3_2160p_m8", nl, tl)
        p.same_ref_poc = sp
        prm[i] = p
    cur = (B.PaPicture * n)(*[d[c_] for c_, _, _, _ in cases])
    r0 = (B.PaPicture * n)(*[d[a] for _, a, _, _ in cases])
    r1 = (B.PaPicture * n)(*[d[b] for _, _, b, _ in cases])
    res = [torch.zeros((nsb, 85 * 10), dtype=torch.int32, device=dev) for _ in range(n)]
    rp = (C.c_void_p * n)(*[t.data_ptr() for t in res])
    B.check(lib.svt_hip_me_batch_layers_device(ctx, n, cur, r0, r1, prm, rp, None))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    for i, (c_, a, b, (nl, tl, sp)) in enumerate(cases):
        g = res[i].cpu().numpy().view(B.ME_RESULT_DTYPE).reshape(nsb, 85)
        o, _ = T.oracle_me_picture_per_sb(pool[c_], pool[a], pool[b] if nl == 2 else None, prm[i])
        assert not T.me_results_equal(o, g, nl), (i, nl, tl, sp, T.me_results_equal(o, g, nl))


@pytest.mark.skipif(not T.have_ref("ref_me_sb"), reason="oracle/_ref/ref_me_sb not built (reference absent at build time)")
@pytest.mark.parametrize("name", list(MC.PRESETS))
@pytest.mark.parametrize("kind", ["dented", "blocks", "taps"])
def test_hip_me_vs_reference_motion_estimate_sb_at_the_ceiling(ctx, kind, name):
    """HIP against the reference's own motion_estimate_sb (oracle/_ref/ref_me_sb), no oracle in between, per SB range; these kinds stay below
    MAX_SAD_VALUE in the 64x64 PU, so the reference's output does not depend on where a range starts"""
    size = K.SIZE_FAST if name == "c3_2160p_m8" else K.SIZES[0]
    pics = pics_of(kind, size)
    nsb = T.n_sb(*size)
    for nl, tl in LISTS_LAYERS:
        p = params(name, nl, tl)
        r1 = pics[2] if nl == 2 else None
        g, _ = hip_me_picture(ctx, pics[1], pics[0], r1, p)
        for s0 in range(0, nsb, 5):
            s1 = min(nsb, s0 + 5)
            r, _ = T.ref_me_picture(pics[1], pics[0], r1, p, s0, s1)
            bad = T.me_results_equal(r[s0:s1], g[s0:s1], nl)
            assert not bad, (kind, name, nl, tl, s0, s1, bad)


# ---- the neighbours of ME that share its primitives -----------------------------------------------------------------------------------------------
def test_sad_loop_at_the_ceiling(ctx):
    case, want = T.make_sad_loop_ceiling_case()
    o = T.oracle_sad_loop_case(case)
    assert np.array_equal(o, want)
    assert np.array_equal(T.hip_sad_loop_case(ctx, case), o)


@pytest.mark.parametrize("w,h,res", [(328, 200, 0), (1920, 1080, 2), (3840, 2160, 3)])
@pytest.mark.parametrize("kind", ["black_white", "dented", "hme"])
def test_zz_sad_at_the_ceiling(ctx, kind, w, h, res):
    f = K.content(kind, w, h, 7)
    cur, prev = T.PaPic(f[1]), T.PaPic(f[0])
    o = T.oracle_me_zz_sad(cur, prev, res)
    g = T.hip_me_zz_sad(ctx, cur, prev, res)
    assert np.array_equal(o[0], g[0]) and np.array_equal(o[1], g[1])
    assert (o[0] == 16 * 16 * 255).any()          # a 16x16 block of the 1/16 plane, all samples 255 apart (the dents are not among the decimated samples)


@pytest.mark.parametrize("res,tl,slice_type,rc", [(0, 0, 2, 1), (3, 2, 0, 1), (3, 0, 1, 0), (2, 3, 0, 1)])
def test_sb_stats_fed_with_ceiling_me_results(ctx, res, tl, slice_type, rc):
    """svt_hip_me_sb_stats_device on the ME results of black_white: the largest distortions there are in every interval decision"""
    w, h = K.SIZE_FAST
    pics = pics_of("black_white", (w, h))
    o, orc = T.oracle_me_picture_per_sb(pics[1], pics[0], None, MC.preset("c3_2160p_m8", 1, 0))
    case = T.make_sb_stats_case(17, w, h, res, tl, slice_type, 1, rc)
    case["res"], case["rcme"] = o, orc
    a, ah, af = T.oracle_me_sb_stats(case)
    g, gh, gf = T.hip_me_sb_stats(ctx, case)
    for f in a.dtype.names:
        assert np.array_equal(a[f], g[f]), f
    assert np.array_equal(ah, gh) and af == gf

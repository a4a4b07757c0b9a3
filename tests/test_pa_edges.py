"""Picture-analysis statistics at the edges, CPU side: the numpy model (tests/pa_stats_model.py), the oracle's block mean / variance and
test_pa's numpy form of it against what the reference's own composite functions produced for the edge pictures
(tests/golden/pa_edges_reference.npz, written by tests/gen_golden_pa_stats.py through oracle/ref_pastats_driver.c), and the conditions
the edge pictures are there to produce.  Integer arithmetic: equality."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import pa_stats_model as M
import svt_testlib as T
import test_pa as TPA
import test_pa_stats as TP

B = T.B
GOLDEN = os.path.join(T.ROOT, "tests", "golden", "pa_edges_reference.npz")


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def edge_noise(kind, method, th, lh):
    """the model's decision for a ceiling picture (computed once, shared with the GPU tests) -> (picture, result)"""
    _, aw, ah, fw, fh = next(c for c in M.EDGE_NOISE_GEOMETRIES if c[0] == method)
    pic = M.edge_luma(kind, aw, ah, M.LUMA_KINDS.index(kind))
    pic.setflags(write=False)
    return pic, M.detect_noise(method, pic, fw, fh, th, lh)


def check_noise_vs_golden(kind, method, th, lh, flags, cls, var_sum, count):
    g, k = golden(), f"noise|{kind}|{method}|{th}|{lh}"
    assert np.array_equal(flags, g[k + "|flags"]), k
    assert cls == int(g[k + "|class"]), k
    assert (var_sum / count if count else 0.0) == float(g[k + "|var_float"]), k  # pic_noise_variance_float = sum / count


@pytest.mark.parametrize("method", (M.FULL, M.HALF, M.QUARTER))
def test_model_noise_vs_recorded_reference(method):
    n = 0
    for kind in M.LUMA_KINDS:
        for th in (0, 1):
            for lh in M.EDGE_LUMA_HEIGHTS:
                pic, r = edge_noise(kind, method, th, lh)
                assert TP._crc(pic) == int(golden()[f"noise|{kind}|{method}|crc"])
                check_noise_vs_golden(kind, method, th, lh, r["flags"], r["pic_noise_class"], r["variance_sum"], r["sb_count"])
                n += 1
    assert n == 48


def test_model_filter_planes_vs_recorded_reference():
    for kind in ("random", "checker"):
        pic = M.edge_luma(kind, 136, 72, 1)
        assert TP._crc(pic) == int(golden()[f"filter|{kind}|crc"])
        den, noise = M.weak_filter(pic)
        assert np.array_equal(den, golden()[f"filter|{kind}|den"]) and np.array_equal(noise, golden()[f"filter|{kind}|noise"])


def hist_case(ci, kind):
    """-> (key, luma, padded buffer, (ox, oy), cb, cr) of EDGE_HIST_CASES[ci] / EDGE_HIST_MODEL_ONLY[ci - len(..)] with chroma `kind`"""
    cases = M.EDGE_HIST_CASES + M.EDGE_HIST_MODEL_ONLY
    w, h, rw, rh = cases[ci]
    return (f"hist|{w}x{h}|{rw}x{rh}|{kind}",) + M.edge_hist_planes(w, h, kind, 10 * ci + M.CHROMA_KINDS.index(kind))


@pytest.mark.parametrize("ci", range(len(M.EDGE_HIST_CASES)))
def test_model_histograms_vs_recorded_reference(ci):
    w, h, rw, rh = M.EDGE_HIST_CASES[ci]
    g = golden()
    for kind in M.CHROMA_KINDS:
        k, luma, buf, _, cb, cr = hist_case(ci, kind)
        assert TP._crc(np.concatenate([buf.ravel(), cb.ravel(), cr.ravel()])) == int(g[k + "|crc"])
        for scd in (0, 1):
            hist, avg_region, avg = M.histograms(luma[::4, ::4], cb, cr, w, h, rw, rh, scd, buf)
            assert np.array_equal(hist, g[k + "|hist"]), (k, scd)
            assert np.array_equal(avg_region, g[k + f"|{scd}|avg_region"]), (k, scd)
            assert [a if a is not None else 0xEE for a in avg] == list(g[k + f"|{scd}|avg"]), (k, scd)


def cmean_case(si, kind):
    w, h = M.EDGE_SB_SIZES[si]
    return f"cmean|{w}x{h}|{kind}", M.edge_chroma(kind, w // 2, h // 2, 20 + si), M.edge_chroma(kind, w // 2, h // 2, 30 + si)


@pytest.mark.parametrize("si", range(len(M.EDGE_SB_SIZES)))
def test_model_chroma_means_vs_recorded_reference(si):
    w, h = M.EDGE_SB_SIZES[si]
    for kind in M.CHROMA_KINDS:
        k, cb, cr = cmean_case(si, kind)
        assert TP._crc(np.concatenate([cb.ravel(), cr.ravel()])) == int(golden()[k + "|crc"])
        mcb, mcr = M.chroma_means(cb, cr, w, h)
        assert np.array_equal(mcb, golden()[k + "|cb"]) and np.array_equal(mcr, golden()[k + "|cr"]), k
        if kind == "saturated":
            nx = (w + 63) // 64
            for sb in range(T.n_sb(w, h)):  # 255 in every complete SB, 0 in the others
                assert (mcb[sb] == (255 if (sb % nx) * 64 + 64 <= w and (sb // nx) * 64 + 64 <= h else 0)).all()


def meanvar_case(si, kind):
    w, h = M.EDGE_SB_SIZES[si]
    return (f"meanvar|{w}x{h}|{kind}",) + M.edge_meanvar_plane(kind, w, h, 4 * si + M.EDGE_MEANVAR_KINDS.index(kind))


def oracle_meanvar(buf, ox, oy, w, h):
    n = T.n_sb(w, h)
    mean, var = np.zeros((n, 85), np.uint8), np.zeros((n, 85), np.uint16)
    pl = B.Plane(buf.ctypes.data, buf.strides[0], ox, oy, w, h)
    assert T.oracle().svt_oracle_pa_mean_variance(C.byref(pl), mean.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p)) == 0
    return mean, var


@pytest.mark.parametrize("si", range(len(M.EDGE_SB_SIZES)))
def test_oracle_and_numpy_meanvar_vs_recorded_reference(si):
    w, h = M.EDGE_SB_SIZES[si]
    for kind in M.EDGE_MEANVAR_KINDS:
        k, buf, ox, oy = meanvar_case(si, kind)
        assert TP._crc(buf) == int(golden()[k + "|crc"])
        gm, gv = golden()[k + "|mean"], golden()[k + "|var"]
        om, ov = oracle_meanvar(buf, ox, oy, w, h)
        assert np.array_equal(om, gm) and np.array_equal(ov, gv), k
        nm, nv = TPA._numpy_meanvar(buf[oy:, ox:], 0, w, h)
        assert np.array_equal(nm, gm) and np.array_equal(nv, gv), k
    _, buf, ox, oy = meanvar_case(si, "halves")
    assert golden()[f"meanvar|{w}x{h}|halves|var"][0, 21] == (255 * 255) >> 2  # 0 | 255 in equal parts: the largest 8x8 variance


def test_inputs_exercise_the_cases():
    """What the edge pictures are there for, stated on the model alone."""
    some_128 = False
    for method in (M.FULL, M.HALF, M.QUARTER):
        flags, classes = [], set()
        for kind in M.LUMA_KINDS:
            for th in (0, 1):
                for lh in M.EDGE_LUMA_HEIGHTS:
                    _, r = edge_noise(kind, method, th, lh)
                    flags.append(r["flags"])
                    classes.add(r["pic_noise_class"])
                    some_128 = some_128 or r["noise"].max() == 128
                    assert r["noise"].max() <= 128  # in - (4 in + neighbours) / 8 with in <= 255
        flags = np.concatenate(flags)
        assert (flags == 1).any() and (flags == 0).any(), method      # in each precision: flags of both values ...
        assert M.CLASS_3_1 in classes and M.CLASS_1 in classes, method  # ... and the top class (next to the bottom one)
    assert some_128                                                    # some noise sample equals the filter's ceiling
    # some 8x8 block is all 255: its mean of squares << 16 is 4 261 478 400, and four of them no longer fit 32 bits
    white = M.edge_luma("white", 200, 196)
    m, q = M._sums8x8(white[:8, :8], True)
    assert int(q[0, 0]) == 255 * 255 << 16 == 4261478400 and 4 * int(q[0, 0]) >= 1 << 32
    # the conditions written down when the cases were chosen
    r = edge_noise("checker", M.FULL, 1, 720)[1]
    assert np.array_equal(r["flags"].reshape(4, 4), np.array([[0, 0, 0, 0], [0, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]))
    assert (r["pic_noise_class"], r["sb_count"]) == (M.CLASS_3_1, 9)
    for method in (M.HALF, M.QUARTER):
        r = edge_noise("checker", method, 1, 1080)[1]
        assert (r["flags"] == 1).any() and (r["flags"] == 0).any() and r["pic_noise_class"] == M.CLASS_3_1
    # saturated chroma: the region average exceeds 255 and wraps through the (uint8_t) cast; min(255, ..) would give another value
    wrapped = {}
    for ci, (w, h, rw, rh) in enumerate(M.EDGE_HIST_CASES + M.EDGE_HIST_MODEL_ONLY):
        _, luma, buf, _, cb, cr = hist_case(ci, "saturated")
        _, avg_region, _ = M.histograms(luma[::4, ::4], cb, cr, w, h, rw, rh, 1, buf)
        wrapped[(w, h, rw, rh)] = sorted(set(avg_region[:, :, 1].ravel().tolist()))
        for i in range(rw):
            for j in range(rh):
                wo, ho = w // rw + (w - rw * (w // rw) if i == rw - 1 else 0), h // rh + (h - rh * (h // rh) if j == rh - 1 else 0)
                s = 255 * len(range(0, wo >> 1, 4)) * len(range(0, ho >> 1, 4)) << 4
                unwrapped = (s + ((wo * ho) >> 3)) // ((wo * ho) >> 2)
                assert int(avg_region[i, j, 1]) == unwrapped & 255
    assert wrapped[(72, 40, 3, 2)] == [50] and wrapped[(200, 136, 3, 2)] == [30, 39]
    assert min(wrapped[(328, 200, 5, 3)]) == 10 and max(wrapped[(328, 200, 5, 3)]) == 39
    assert any(v != [255] for v in wrapped.values())  # (min(255, unwrapped) is 255 wherever the value wrapped)
    assert (200 // 8) % 2 == 1                        # an odd region width: the chroma origin (i * region) >> 1 truncates
    # the SB counts that leave a last workgroup of four partly filled, and one that does not
    assert sorted(T.n_sb(w, h) % 4 for w, h in M.EDGE_SB_SIZES) == [0, 1, 2, 3]

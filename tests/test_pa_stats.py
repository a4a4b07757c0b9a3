"""Picture-analysis statistics (noise detection, histograms, chroma means), CPU side: the numpy model of tests/pa_stats_model.py
against the reference -- its leaf functions called live (oracle/_ref/libsvtref_pa.so, when present) and the recorded outputs of
its leaf and composite functions (tests/golden/pa_stats_reference.npz) -- and the host-side parameter derivation."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import pa_stats_model as M
import svt_testlib as T

B = T.B
REF_PA = os.path.join(T.REF_DIR, "libsvtref_pa.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_PA), reason="oracle/_ref/libsvtref_pa.so not built")
GOLDEN = os.path.join(T.ROOT, "tests", "golden", "pa_stats_reference.npz")


class RefPicture(C.Structure):
    """EbPictureBufferDesc (Codec/EbPictureBufferDesc.h:27-60)"""
    _fields_ = ([(n, C.c_void_p) for n in ("buffer_y", "buffer_cb", "buffer_cr", "bit_inc_y", "bit_inc_cb", "bit_inc_cr")] +
                [(n, C.c_uint16) for n in ("stride_y", "stride_cb", "stride_cr", "stride_bit_inc_y", "stride_bit_inc_cb", "stride_bit_inc_cr",
                                           "origin_x", "origin_y", "width", "height", "max_width", "max_height")] +
                [("bit_depth", C.c_int), ("luma_size", C.c_uint32), ("chroma_size", C.c_uint32), ("packed_flag", C.c_uint8)])


def _desc(arr, pad, w, h):
    d = RefPicture()
    d.buffer_y, d.stride_y, d.origin_x, d.origin_y, d.width, d.height = arr.ctypes.data, arr.strides[0], pad, pad, w, h
    return d


def ref_weak_filter(pic, rows=None):
    """The reference's own weak luma filter over the first `rows` rows of `pic` (a multiple of 64, or all of it), composed as its detect
    loops do: per 64-row strip the AVX2 form over the whole 64-column blocks, then the C form for a last partial column.
    -> (denoised, noise) with the noise strips stacked into a plane."""
    ref = C.CDLL(REF_PA, mode=1)
    h, w = pic.shape
    rows = h if rows is None else rows
    pad = 16
    src = np.pad(pic, pad, mode="edge")
    den = np.full_like(src, 0xCD)
    noise = np.zeros((rows, w), np.uint8)
    strip = np.full((64 + 2 * pad, w + 2 * pad), 0xCD, np.uint8)
    d_in, d_den, d_strip = _desc(src, pad, w, h), _desc(den, pad, w, h), _desc(strip, pad, w, 64)
    for y in range(0, rows, 64):
        ref.eb_vp9_noise_extract_luma_weak_avx2_intrin(C.byref(d_in), C.byref(d_den), C.byref(d_strip), C.c_uint32(y), C.c_uint32(0))
        if w % 64:
            ref.eb_vp9_noise_extract_luma_weak(C.byref(d_in), C.byref(d_den), C.byref(d_strip), C.c_uint32(y), C.c_uint32((w // 64) * 64))
        n = min(64, rows - y)
        noise[y:y + n] = strip[pad:pad + n, pad:pad + w]
    return den[pad:pad + rows, pad:pad + w].copy(), noise


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


@needs_ref
@pytest.mark.parametrize("w,h,sigma", [(200, 136, 8), (192, 128, 25), (64, 64, 5), (130, 70, 12)])
def test_model_filter_vs_reference_leaf_functions(w, h, sigma):
    pic = M.noise_picture(w, h, sigma)
    den, noise = M.weak_filter(pic)
    rden, rnoise = ref_weak_filter(pic)
    assert np.array_equal(den, rden) and np.array_equal(noise, rnoise)
    assert noise.max() > 0 and (den != pic).any()


@needs_ref
def test_reference_c_and_avx2_filters_agree_on_whole_columns():
    ref = C.CDLL(REF_PA, mode=1)
    pic = M.noise_picture(192, 128, 12)
    a = ref_weak_filter(pic)
    pad, (h, w) = 16, pic.shape
    src, den, strip = np.pad(pic, pad, mode="edge"), np.zeros((h + 32, w + 32), np.uint8), np.zeros((96, w + 32), np.uint8)
    for y in (0, 64):
        ref.eb_vp9_noise_extract_luma_weak(C.byref(_desc(src, pad, w, h)), C.byref(_desc(den, pad, w, h)), C.byref(_desc(strip, pad, w, 64)),
                                           C.c_uint32(y), C.c_uint32(0))
        assert np.array_equal(strip[pad:pad + 64, pad:pad + w], a[1][y:y + 64])
    assert np.array_equal(den[pad:pad + h, pad:pad + w], a[0])


@needs_ref
def test_model_block_means_vs_reference_leaf_functions():
    ref = C.CDLL(REF_PA, mode=1)
    for f in ("compute_mean", "compute_mean_of_squared_values", "eb_vp9_compute_sub_mean8x8_sse2_intrin",
              "eb_vp9_compute_subd_mean_of_squared_values8x8_sse2_intrin", "eb_vp9_compute_mean8x8_avx2_intrin",
              "eb_vp9_compute_mean_of_squared_values8x8_sse2_intrin"):
        getattr(ref, f).restype = C.c_uint64
    rng = np.random.default_rng(4)
    for _ in range(40):
        a = rng.integers(0, 256, (8, 40), dtype=np.uint8)
        p, s = C.c_void_p(a.ctypes.data + 3), a.strides[0]
        blk = a[:, 3:11]
        (m,), (q,) = (x.ravel() for x in M._sums8x8(blk, False))
        assert int(m) == ref.compute_mean(p, s, 8, 8) == ref.eb_vp9_compute_mean8x8_avx2_intrin(p, s, 8, 8)
        assert int(q) == ref.compute_mean_of_squared_values(p, s, 8, 8) == ref.eb_vp9_compute_mean_of_squared_values8x8_sse2_intrin(p, s, 8, 8)
        (m,), (q,) = (x.ravel() for x in M._sums8x8(blk, True))
        assert int(m) == ref.eb_vp9_compute_sub_mean8x8_sse2_intrin(p, C.c_uint16(s))
        assert int(q) == ref.eb_vp9_compute_subd_mean_of_squared_values8x8_sse2_intrin(p, C.c_uint16(s))


@needs_ref
@pytest.mark.parametrize("kind", M.LUMA_KINDS)
def test_model_filter_vs_reference_leaf_functions_at_the_ceilings(kind):
    """the ceiling pictures through both forms of the reference's filter, at widths with a partial last column"""
    top = 0
    for w, h in ((200, 196), (136, 72), (130, 70)):
        pic = M.edge_luma(kind, w, h, 3)
        den, noise = M.weak_filter(pic)
        rden, rnoise = ref_weak_filter(pic)
        assert np.array_equal(den, rden) and np.array_equal(noise, rnoise), (w, h)
        top = max(top, int(noise.max()))
    # a lone 255 among zeros: 255 - ((4 * 255) >> 3) = 128, the largest noise sample there is
    assert top == {"white": 0, "black": 0, "checker": 128, "speck": 128, "stripes_even": 64, "stripes_odd": 64, "halves": 32}.get(kind, top)


@needs_ref
def test_model_block_means_vs_reference_leaf_functions_at_the_ceilings():
    """8x8 blocks of the ceiling pictures, the all-255 block (mean of squares << 16 = 4 261 478 400) among them"""
    ref = C.CDLL(REF_PA, mode=1)
    fs = ("compute_mean", "compute_mean_of_squared_values", "eb_vp9_compute_sub_mean8x8_sse2_intrin",
          "eb_vp9_compute_subd_mean_of_squared_values8x8_sse2_intrin", "eb_vp9_compute_mean8x8_avx2_intrin",
          "eb_vp9_compute_mean_of_squared_values8x8_sse2_intrin")
    for f in fs:
        getattr(ref, f).restype = C.c_uint64
    for kind in M.LUMA_KINDS:
        a = M.edge_luma(kind, 40, 9, 5)
        for off in (0, 3):  # aligned and not
            p, s, blk = C.c_void_p(a.ctypes.data + a.strides[0] + off), a.strides[0], a[1:9, off:off + 8]
            (m,), (q,) = (x.ravel() for x in M._sums8x8(blk, False))
            assert int(m) == ref.compute_mean(p, s, 8, 8) == ref.eb_vp9_compute_mean8x8_avx2_intrin(p, s, 8, 8), kind
            assert int(q) == ref.compute_mean_of_squared_values(p, s, 8, 8) == ref.eb_vp9_compute_mean_of_squared_values8x8_sse2_intrin(p, s, 8, 8), kind
            (m,), (q,) = (x.ravel() for x in M._sums8x8(blk, True))
            assert int(m) == ref.eb_vp9_compute_sub_mean8x8_sse2_intrin(p, C.c_uint16(s)), kind
            assert int(q) == ref.eb_vp9_compute_subd_mean_of_squared_values8x8_sse2_intrin(p, C.c_uint16(s)), kind
            if kind == "white":
                assert int(q) == 4261478400 and int(m) == 255 << 8


def test_model_vs_recorded_reference_outputs():
    """The fixture holds what the reference produced for pictures this test regenerates (M.noise_picture / M.gen_chroma; their CRCs are
    stored beside the outputs): the planes of its weak filter, and the outputs of detect_input_picture_noise, sub_sample_detect_noise,
    quarter_sample_detect_noise, the two histogram functions + calculate_input_average_intensity and compute_chroma_block_mean."""
    g = np.load(GOLDEN)
    for w, h, sigma in ((200, 136, 8), (192, 128, 25)):
        pic = M.noise_picture(w, h, sigma)
        assert _crc(pic) == int(g[f"leaf_{w}x{h}_crc"])
        den, noise = M.weak_filter(pic)
        assert np.array_equal(den, g[f"leaf_{w}x{h}_den"]) and np.array_equal(noise, g[f"leaf_{w}x{h}_noise"])
    n = 0
    for ci, (method, aw, ah, fw, fh, th, lh) in enumerate(M.SMALL_NOISE_CASES):
        for sigma in M.SIGMAS:
            pic = M.noise_picture(aw, ah, sigma)
            k = f"noise_{ci}_{sigma}"
            assert _crc(pic) == int(g[k + "_crc"])
            r = M.detect_noise(method, pic, fw, fh, th, lh)
            assert np.array_equal(r["flags"], g[k + "_flags"]), k
            assert r["pic_noise_class"] == int(g[k + "_class"]), k
            want = float(g[k + "_var_float"])  # context_ptr->pic_noise_variance_float = sum / count
            assert (r["variance_sum"] / r["sb_count"] if r["sb_count"] else 0.0) == want, k
            n += 1
    assert n == 30
    for (w, h, rw, rh) in ((200, 136, 4, 4), (200, 136, 3, 2)):
        luma, cb, cr = M.noise_picture(w, h, 8), M.gen_chroma(w // 2, h // 2, 1), M.gen_chroma(w // 2, h // 2, 2)
        for scd in (0, 1):
            k = f"hist_{w}x{h}_{rw}x{rh}_{scd}"
            assert _crc(np.concatenate([luma.ravel(), cb.ravel(), cr.ravel()])) == int(g[k + "_crc"])
            padded = g[k + "_padded"]  # the reference driver's padded luma buffer (scd_mode 0 reads it from its first byte)
            hist, avg_region, avg = M.histograms(luma[::4, ::4], cb, cr, w, h, rw, rh, scd, padded)
            assert np.array_equal(hist, g[k + "_hist"]), k
            assert np.array_equal(avg_region, g[k + "_avg_region"]), k
            assert [a if a is not None else 0xEE for a in avg] == list(g[k + "_avg"]), k  # 0xEE: what the driver put there before the call
    cb, cr = M.gen_chroma(100, 68, 3), M.gen_chroma(100, 68, 4)
    mcb, mcr = M.chroma_means(cb, cr, 200, 136)
    assert np.array_equal(mcb, g["cmean_cb"]) and np.array_equal(mcr, g["cmean_cr"])
    for sb in range(12):  # 200 x 136 = 4 x 3 SBs: SB column 3 and SB row 2 are incomplete
        assert mcb[sb].any() == (sb % 4 < 3 and sb // 4 < 2) == mcr[sb].any()


def test_inputs_exercise_the_decision():
    """The test pictures make every branch of the decision happen, in each precision: flagged and unflagged SBs, three or more classes."""
    for method in (M.FULL, M.HALF, M.QUARTER):
        classes, flags = set(), []
        for case in M.SMALL_NOISE_CASES:
            if case[0] != method:
                continue
            for sigma in M.SIGMAS:
                r = M.detect_noise(method, M.noise_picture(case[1], case[2], sigma), *case[3:])
                classes.add(r["pic_noise_class"])
                flags.append(r["flags"])
        flags = np.concatenate(flags)
        assert (flags == 1).any() and (flags == 0).any(), method
        assert len(classes) >= 3, (method, classes)
    assert (200 // 4) % 4 and (136 // 4) % 4  # the histogram case has a remainder in both directions
    assert 200 % 64 and 136 % 64            # and the chroma-mean case has incomplete SBs


# the noise fields of eb_vp9_signal_derivation_pre_analysis_sq / _oq / _vmaf (Codec/EbResourceCoordinationProcess.c:297-328, :365-393,
# :433-437), written out from the text: per tune, enc_mode -> (method, th) for the input-resolution classes below 1080p, 1080p and 4K
def _derive_table(tune, mode, res):
    if tune == 2:
        return M.QUARTER, 1
    if tune == 0:
        method = M.FULL if res < 2 or mode <= 8 else (M.QUARTER if res == 2 else M.HALF)
        return method, 0 if mode <= 8 else 1
    method = M.FULL if res < 2 or mode <= 3 else (M.QUARTER if res == 2 else M.HALF)
    th = 0 if mode <= 3 else ((1 if res <= 2 else 0) if mode <= 8 else 1)
    return method, th


# five picture sizes: 480p and 720p (576p-or-lower and 1080i range), 1080p twice (its lower and upper part), 2160p
@pytest.mark.parametrize("w,h,res", [(720, 480, 0), (1280, 720, 1), (1920, 1080, 2), (2048, 1080, 2), (3840, 2160, 3)])
def test_noise_params_derive(w, h, res):
    assert B.load().svt_hip_input_resolution(w, h) == res
    for tune in range(3):
        for mode in range(13):
            p = B.pa_noise_params_derive(tune, mode, w, h)
            assert (p.method, p.noise_detection_th, p.luma_height) == (*_derive_table(tune, mode, res), h), (tune, mode, w, h)
    # the headline configuration: 2160p, enc-mode 8, tune 1 -> half precision on the 1/16 picture, threshold index 0
    p = B.pa_noise_params_derive(1, 8, 3840, 2160)
    assert (p.method, p.noise_detection_th) == (M.HALF, 0)
    q = B.PaNoiseParams()
    assert B.load().svt_hip_pa_noise_params_derive(C.byref(q), 3, 0, 64, 64) != 0
    assert B.load().svt_hip_pa_noise_params_derive(C.byref(q), 0, 13, 64, 64) != 0

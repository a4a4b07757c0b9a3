"""Writes tests/golden/pa_edges_reference.npz: what the reference's own picture-analysis statistics produce for the edge pictures of
tests/pa_stats_model.py.  Needs oracle/_ref/ref_pa_stats and oracle/_ref/libsvtref_pa.so (`make -C oracle ref`, where the reference's
sources are); the tests that read the fixture need neither.

    python tests/gen_golden_pa_stats.py                    write the fixture
    python tests/gen_golden_pa_stats.py --check-existing   recompute every array of tests/golden/pa_stats_reference.npz and compare

The driver (oracle/ref_pastats_driver.c) runs the reference's static composite functions; every case is run with the C / SSE2 forms
(eb_vp9_ASM_TYPES = 0) and with the AVX2 forms (3), and the two must agree.  Only outputs and the CRCs of the inputs are stored: the
tests regenerate the inputs.  The two filter-plane cases come from the reference's leaf filter, as tests/test_pa_stats.py calls it."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pa_stats_model as M  # noqa: E402
import svt_testlib as T  # noqa: E402
import test_pa_stats as TP  # noqa: E402

DRIVER = os.path.join(T.REF_DIR, "ref_pa_stats")
OUT = os.path.join(T.ROOT, "tests", "golden", "pa_edges_reference.npz")
ASM = (0, 3)


def _plane(buf, ox, oy):
    assert buf.flags.c_contiguous and buf.dtype == np.uint8
    return struct.pack("<4i", buf.shape[1], ox, oy, buf.shape[0]) + buf.tobytes()


def _run(kind, ints, planes, asm):
    with tempfile.TemporaryDirectory() as d:
        req, rsp = os.path.join(d, "req"), os.path.join(d, "rsp")
        with open(req, "wb") as f:
            f.write(struct.pack(f"<{3 + len(ints)}i", 0x53505653, kind, asm, *ints) + b"".join(planes))
        subprocess.check_call([DRIVER, req, rsp])
        with open(rsp, "rb") as f:
            return f.read()


def _both(kind, ints, planes, parse):
    """the case under both instruction-set selections; the parsed outputs must agree"""
    outs = [parse(_run(kind, ints, planes, asm)) for asm in ASM]
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b), ("the reference's C and AVX2 forms differ", kind, ints)
    return outs[0]


def ref_noise(method, buf, ox, oy, aw, ah, fw, fh, th, luma_height):
    """-> flags, class, pic_noise_variance_float (a plane of any padding: the filter reads the picture alone)"""
    n_sb = ((fw + 63) // 64) * ((fh + 63) // 64)

    def parse(b):
        cls, _, var = struct.unpack_from("<iid", b, n_sb)
        return np.frombuffer(b, np.uint8, n_sb).copy(), np.uint32(cls), np.float64(var)
    return _both(1, (method, fw, fh, th, luma_height, aw, ah), (_plane(buf, ox, oy),), parse)


def ref_hist(w, h, rw, rh, scd, full_buf, ox, oy, y16, cb, cr):
    """-> hist [rw][rh][3][256], avg_region [rw][rh][3], avg [3].  Cb / Cr go into buffers whose origin is the luma's >> 1."""
    pc = [np.pad(c, ((oy >> 1, oy >> 1), (ox >> 1, ox >> 1)), mode="edge") for c in (cb, cr)]
    n = rw * rh * 3

    def parse(b):
        return (np.frombuffer(b, np.uint32, n * 256).reshape(rw, rh, 3, 256).copy(), np.frombuffer(b, np.uint8, n, n * 1024).reshape(rw, rh, 3).copy(),
                np.frombuffer(b, np.uint8, 3, n * 1025).copy())
    return _both(2, (w, h, rw, rh, scd), (_plane(full_buf, ox, oy), _plane(np.pad(y16, 4, mode="edge"), 4, 4), _plane(pc[0], ox >> 1, oy >> 1),
                                          _plane(pc[1], ox >> 1, oy >> 1)), parse)


def ref_chroma_means(w, h, cb, cr):
    ox, oy = 12, 6
    pc = [M.hostile_plane(c, ox >> 1, oy >> 1, w // 2 + ox + 3, 40 + i) for i, c in enumerate((cb, cr))]
    n = T.n_sb(w, h) * 21

    def parse(b):
        return np.frombuffer(b, np.uint8, n).reshape(-1, 21).copy(), np.frombuffer(b, np.uint8, n, n).reshape(-1, 21).copy()
    return _both(3, (w, h, ox, oy), (_plane(pc[0], ox >> 1, oy >> 1), _plane(pc[1], ox >> 1, oy >> 1)), parse)


def ref_meanvar(w, h, buf, ox, oy):
    n = T.n_sb(w, h) * 85

    def parse(b):
        return np.frombuffer(b, np.uint8, n).reshape(-1, 85).copy(), np.frombuffer(b, np.uint16, n, n).reshape(-1, 85).copy()
    return _both(4, (w, h), (_plane(buf, ox, oy),), parse)


def generate():
    g = {}
    for ki, kind in enumerate(M.LUMA_KINDS):
        for method, aw, ah, fw, fh in M.EDGE_NOISE_GEOMETRIES:
            pic = M.edge_luma(kind, aw, ah, ki)
            buf = M.hostile_plane(pic, 13, 9, aw + 29, ki)
            g[f"noise|{kind}|{method}|crc"] = np.uint32(TP._crc(pic))
            for th in (0, 1):
                for lh in M.EDGE_LUMA_HEIGHTS:
                    k = f"noise|{kind}|{method}|{th}|{lh}"
                    g[k + "|flags"], g[k + "|class"], g[k + "|var_float"] = ref_noise(method, buf, 13, 9, aw, ah, fw, fh, th, lh)
    for kind in ("random", "checker"):  # the one small case with filter planes: every sample of both, from both forms of the leaf filter
        pic = M.edge_luma(kind, 136, 72, 1)
        g[f"filter|{kind}|crc"] = np.uint32(TP._crc(pic))
        g[f"filter|{kind}|den"], g[f"filter|{kind}|noise"] = TP.ref_weak_filter(pic)
    for ci, (w, h, rw, rh) in enumerate(M.EDGE_HIST_CASES):
        for ki, kind in enumerate(M.CHROMA_KINDS):
            luma, buf, (ox, oy), cb, cr = M.edge_hist_planes(w, h, kind, 10 * ci + ki)
            k = f"hist|{w}x{h}|{rw}x{rh}|{kind}"
            g[k + "|crc"] = np.uint32(TP._crc(np.concatenate([buf.ravel(), cb.ravel(), cr.ravel()])))
            for scd in (0, 1):
                hist, g[k + f"|{scd}|avg_region"], g[k + f"|{scd}|avg"] = ref_hist(w, h, rw, rh, scd, buf, ox, oy, luma[::4, ::4], cb, cr)
                assert scd == 0 or np.array_equal(hist, g[k + "|hist"])
                g[k + "|hist"] = hist
    for si, (w, h) in enumerate(M.EDGE_SB_SIZES):
        for ki, kind in enumerate(M.CHROMA_KINDS):
            cb, cr = M.edge_chroma(kind, w // 2, h // 2, 20 + si), M.edge_chroma(kind, w // 2, h // 2, 30 + si)
            k = f"cmean|{w}x{h}|{kind}"
            g[k + "|crc"] = np.uint32(TP._crc(np.concatenate([cb.ravel(), cr.ravel()])))
            g[k + "|cb"], g[k + "|cr"] = ref_chroma_means(w, h, cb, cr)
        for ki, kind in enumerate(M.EDGE_MEANVAR_KINDS):
            buf, ox, oy = M.edge_meanvar_plane(kind, w, h, 4 * si + ki)
            k = f"meanvar|{w}x{h}|{kind}"
            g[k + "|crc"] = np.uint32(TP._crc(buf))
            g[k + "|mean"], g[k + "|var"] = ref_meanvar(w, h, buf, ox, oy)
    np.savez_compressed(OUT, **g)
    print(f"{OUT}: {len(g)} arrays, {os.path.getsize(OUT)} bytes")


def check_existing():
    """every array of pa_stats_reference.npz again, through the committed driver (and the leaf filter for the two filter planes)"""
    g = np.load(TP.GOLDEN)
    bad, seen = [], set()

    def cmp(key, val):
        seen.add(key)
        if not np.array_equal(np.asarray(val), g[key]):
            bad.append(key)
    for w, h, sigma in ((200, 136, 8), (192, 128, 25)):
        pic = M.noise_picture(w, h, sigma)
        den, noise = TP.ref_weak_filter(pic)
        cmp(f"leaf_{w}x{h}_crc", TP._crc(pic)), cmp(f"leaf_{w}x{h}_den", den), cmp(f"leaf_{w}x{h}_noise", noise)
    for ci, (method, aw, ah, fw, fh, th, lh) in enumerate(M.SMALL_NOISE_CASES):
        for sigma in M.SIGMAS:
            pic = M.noise_picture(aw, ah, sigma)
            flags, cls, var = ref_noise(method, np.pad(pic, 16, mode="edge"), 16, 16, aw, ah, fw, fh, th, lh)
            k = f"noise_{ci}_{sigma}"
            cmp(k + "_crc", TP._crc(pic)), cmp(k + "_flags", flags), cmp(k + "_class", cls), cmp(k + "_var_float", var)
    for (w, h, rw, rh) in ((200, 136, 4, 4), (200, 136, 3, 2)):
        luma, cb, cr = M.noise_picture(w, h, 8), M.gen_chroma(w // 2, h // 2, 1), M.gen_chroma(w // 2, h // 2, 2)
        for scd in (0, 1):
            k = f"hist_{w}x{h}_{rw}x{rh}_{scd}"
            padded = np.ascontiguousarray(g[k + "_padded"])  # the old driver's padded luma buffer: an input, taken as recorded
            seen.add(k + "_padded")
            pad = (padded.shape[0] - h) // 2
            assert np.array_equal(padded[pad:pad + h, pad:pad + w], luma)
            hist, avg_region, avg = ref_hist(w, h, rw, rh, scd, padded, pad, pad, luma[::4, ::4], cb, cr)
            cmp(k + "_crc", TP._crc(np.concatenate([luma.ravel(), cb.ravel(), cr.ravel()])))
            cmp(k + "_hist", hist), cmp(k + "_avg_region", avg_region), cmp(k + "_avg", avg)
    mcb, mcr = ref_chroma_means(200, 136, M.gen_chroma(100, 68, 3), M.gen_chroma(100, 68, 4))
    cmp("cmean_cb", mcb), cmp("cmean_cr", mcr)
    missing = sorted(set(g.files) - seen)
    print(f"pa_stats_reference.npz: {len(seen)} arrays recomputed, {len(bad)} differ {bad}, {len(missing)} not covered {missing}")
    return 1 if bad or missing else 0


if __name__ == "__main__":
    if not os.path.exists(DRIVER) or not os.path.exists(TP.REF_PA):
        sys.exit("oracle/_ref/ref_pa_stats and libsvtref_pa.so are needed: make -C oracle ref")
    sys.exit(check_existing() if "--check-existing" in sys.argv[1:] else generate())

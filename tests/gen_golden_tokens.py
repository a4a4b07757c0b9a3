"""Writes tests/golden/tokens_reference.npz: three small pictures (inter, intra, mixed) as the encode pass leaves them -- grid with skip
flags, coefficients, eob map -- and what the REFERENCE's eb_vp9_tokenize_sb makes of them, block by block in the entropy coder's order:
token, extra bits, probability row and coef_counts.  The reference runs in tests/c/ref_tokenize_driver.c, compiled here against the
reference's headers into a temporary directory and linked with the objects `make -C oracle ref` builds; only inputs and recorded
results are stored.

    python tests/gen_golden_tokens.py            (needs the reference sources and oracle/_ref)
"""
import ctypes as C
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encdec_model as M      # noqa: E402
import me_configs as MC       # noqa: E402
import svt_testlib as T       # noqa: E402
import tokenize_model as TM   # noqa: E402

B = T.B
REF = os.environ.get("SVT_REFERENCE", "/root/reference")
OUT = os.path.join(T.GOLDEN_DIR, "tokens_reference.npz")
W, H = 136, 72
# (kind, seed, q index, lambda of the stand-in decision): the q indices leave a share of the blocks without coefficients (skipped) and
# still reach every token class; the large lambda merges the two whole SBs of the inter picture into 64x64 blocks (32x32 chroma transforms)
PICTURES = (("inter", 31, 100, 30000), ("intra", 32, 40, 0), ("mixed", 33, 120, 300))


def _chroma(y, k):
    u = (y[::2, ::2].astype(np.int32) // 2 + 32 + 8 * k).astype(np.uint8)
    v = (255 - y[::2, ::2] // 2 - (y[1::2, 1::2] // 4)).astype(np.uint8)
    return u, v


def make_picture(kind, seed, q_index, lam):
    """(lf_mi with skip flags, qcoeff, eob map) of one picture out of the oracle's encode pass"""
    lib = B.load()
    cfg = dict(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=0, loop_filter=1)
    c, flags = B.EncdecFlagsConfig(**cfg), B.EncdecFlags()
    assert lib.svt_hip_encdec_flags_derive(C.byref(c), C.byref(flags)) == 0
    thr = B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    frames = T.gen_clip_subpel(W, H, 3, seed)
    src = (frames[1],) + _chroma(frames[1], 1)
    if kind == "intra":
        lf = M.gen_intra_grid(seed, W, H, sizes=(4, 8, 16, 32), filter_level=level)
        o = M.oracle_intra_chain(src, lf, q_index, flags, thr)
        return o["lf_mi"], o["qcoeff"], o["eob_map"]
    refs = [M.RefPic(W, H).set_padded(frames[k], *_chroma(frames[k], k)) for k in (0, 2)]
    pics = [T.PaPic(f) for f in frames]
    me = T.oracle_me_picture_mt(pics[1], pics[0], pics[2], MC.preset("c2_1080p_m8", 2, 1))[0]
    mc = np.zeros((H // 8, W // 8), dtype=B.MC_MODE_INFO_DTYPE)
    lf = np.zeros((H // 8, W // 8), dtype=B.LF_MODE_INFO_DTYPE)
    assert lib.svt_hip_md_default_picture(me.ctypes.data_as(C.c_void_p), W, H, lam, level, mc.ctypes.data_as(C.c_void_p), lf.ctypes.data_as(C.c_void_p), W // 8) == 0
    if kind == "mixed":
        lf, mc, n = M.make_mixed(seed, lf, mc, share=0.35, level=level)
        assert n > 0
    o = M.oracle_encdec_picture(src, refs, mc, lf, q_index, flags, thr)
    return o["lf_mi"], o["qcoeff"], o["eob_map"]


def build_driver(td):
    rs = os.path.join(REF, "Source")
    rl = os.path.join(rs, "Lib")
    obj = os.path.join(T.REF_DIR, "obj")
    exe = os.path.join(td, "ref_tokenize")
    inc = [os.path.join(T.REF_DIR, "gen"), os.path.join(rs, "API")] + [os.path.join(rl, d) for d in ("VPX", "Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    objs = [os.path.join(obj, n + ".o") for n in ("vp9_tokenize", "vp9_entropy", "vp9_blockd", "vp9_scan", "vp9_common_data", "vp9_reconintra")]
    cmd = ["gcc", "-std=gnu99", "-O2", "-w"] + [f"-I{d}" for d in inc] + ["-no-pie", "-Wl,-z,lazy", "-Wl,--unresolved-symbols=ignore-all", "-o", exe,
                                                                      os.path.join(T.ROOT, "tests", "c", "ref_tokenize_driver.c")] + objs + ["-lm"]
    subprocess.check_call(cmd)
    return exe


def ref_tokenize(exe, td, lf_mi, qcoeff, eob_map):
    """the reference's tokens per transform block: (plane, x4, y4, n, tokens[n], extras[n], rows[n]) lists + counts + seconds"""
    req, rsp = os.path.join(td, "req.bin"), os.path.join(td, "rsp.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<3i", 0x4b4f5453, W, H))
        f.write(np.ascontiguousarray(lf_mi[:, :W // 8]).tobytes())
        f.write(np.ascontiguousarray(qcoeff, np.int16).tobytes())
        f.write(np.ascontiguousarray(eob_map, np.uint16).tobytes())
    subprocess.check_call([exe, req, rsp])
    raw = np.frombuffer(open(rsp, "rb").read(), np.uint8)
    words = raw[:(raw.size - 8) // 4 * 4].view(np.int32)
    nb, pos = int(words[0]), 1
    blk, tok = [], []
    for _ in range(nb):
        p, x4, y4, n = (int(v) for v in words[pos:pos + 4])
        pos += 4
        blk.append((p, x4, y4, n))
        tok.append(words[pos:pos + 3 * n].reshape(n, 3))
        pos += 3 * n
    counts = words[pos:pos + TM.N_COUNTS].view(np.uint32).copy()
    seconds = float(raw[(pos + TM.N_COUNTS) * 4:(pos + TM.N_COUNTS) * 4 + 8].view(np.float64)[0])
    return np.array(blk, np.int32).reshape(-1, 4), (np.concatenate(tok) if tok else np.zeros((0, 3), np.int32)), counts, seconds


def coverage(pictures):
    """what the reference's own output covers; every entry must hold (tests/test_tokenize.py repeats this on the committed file)"""
    sizes, inter, types, ctxs, tokens, full, skip_left, skip_above = set(), set(), set(), set(), set(), 0, 0, 0
    for p in pictures:
        lf, emap = p["lf_mi"], p["eob_map"]
        model = {(b["plane"], b["x4"], b["y4"]): b for b in TM.picture_blocks(lf, emap, W, H)}
        off = 0
        for plane, x4, y4, n in p["blocks"]:
            m = model[(int(plane), int(x4), int(y4))]
            rows, toks = p["tokens"][off:off + n, 2], p["tokens"][off:off + n, 0]
            off += n
            ts, ptype, is_inter = int(rows[0]) // 144, (int(rows[0]) // 72) % 2, (int(rows[0]) // 36) % 2
            sizes.add((ts, ptype)); inter.add(is_inter); ctxs.add(int(rows[0]) % 6); tokens |= set(int(t) for t in toks)
            if plane == 0:
                types.add((ts, m["tt"]))
            full += int(n == 16 << (2 * ts) and toks[-1] != TM.EOB_TOKEN)
        sk = lf["skip"][:, :W // 8].astype(bool)
        skip_left += int((sk[:, :-1] & ~sk[:, 1:]).sum())
        skip_above += int((sk[:-1] & ~sk[1:]).sum())
    return dict(sizes=sizes, inter=inter, types=types, ctxs=ctxs, tokens=tokens, full=full, skip_left=skip_left, skip_above=skip_above)


def check_coverage(cov):
    assert cov["sizes"] == {(ts, pt) for ts in range(4) for pt in range(2)}, cov["sizes"]
    assert cov["inter"] == {0, 1}
    assert cov["types"] >= {(ts, tt) for ts in range(3) for tt in range(4)}, cov["types"]
    assert cov["ctxs"] == {0, 1, 2}
    assert cov["tokens"] == set(range(12)), cov["tokens"]
    assert cov["full"] >= 1 and cov["skip_left"] >= 1 and cov["skip_above"] >= 1, cov


def main():
    out, pictures = {}, []
    with tempfile.TemporaryDirectory() as td:
        exe = build_driver(td)
        for k, (kind, seed, q_index, lam) in enumerate(PICTURES):
            lf, q, emap = make_picture(kind, seed, q_index, lam)
            lf = np.ascontiguousarray(lf[:, :W // 8])
            blocks, tokens, counts, seconds = ref_tokenize(exe, td, lf, q, emap)
            print(f"{kind}: {len(blocks)} transform blocks, {len(tokens)} tokens, {int(lf['skip'].sum())} skipped units, reference {seconds * 1e3:.3f} ms")
            pictures.append(dict(lf_mi=lf, qcoeff=q, eob_map=emap, blocks=blocks, tokens=tokens, counts=counts))
            out[f"lf_mi|{k}"], out[f"qcoeff|{k}"], out[f"eob_map|{k}"] = lf.view(np.uint8), q, emap
            out[f"blocks|{k}"], out[f"counts|{k}"] = blocks.astype(np.int16), counts
            out[f"token|{k}"], out[f"extra|{k}"], out[f"row|{k}"] = tokens[:, 0].astype(np.uint8), tokens[:, 1].astype(np.uint16), tokens[:, 2].astype(np.uint16)
    cov = coverage(pictures)
    print({k: (sorted(v) if isinstance(v, set) else v) for k, v in cov.items()})
    check_coverage(cov)
    out["size"] = np.array([W, H], np.int32)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

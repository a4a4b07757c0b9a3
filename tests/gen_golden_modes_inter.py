"""Writes tests/golden/modes_inter_reference.npz: the seeded inter pictures of tests/modes_inter_model.py -- the three grids, the frame
parameters, coefficients, eob map -- and what the REFERENCE makes of them: the bytes of the whole tile (write_partition,
pack_inter_mode_mvs and pack_mb_tokens per block between eb_vp9_start_encode and eb_vp9_stop_encode), the bytes of the mode-info bools
alone (the same walk, tokens left out), the frame-context tables it codes with (eb_vp9_init_mode_probs, eb_vp9_init_mv_probs), the
compound references eb_vp9_setup_compound_reference_mode derives, and the seconds one pass of its tile coding took.  The token records
sent to the reference come from svt_hip_tokenize_picture, the host form tests/golden/tokens_reference.npz pins to the reference.  The
reference runs in tests/c/ref_modes_inter_driver.c, compiled here against the reference's headers into a temporary directory and linked
with the objects `make -C oracle ref` builds; only inputs and recorded results are stored.

The driver notes, with the reference's own context functions, under which contexts and with which symbols the reference coded; the
generator fails unless those notes reach everything tests/modes_inter_model.py:coverage_complete names.

    python tests/gen_golden_modes_inter.py            (needs the reference sources and oracle/_ref)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boolcode_model as BM        # noqa: E402
import modes_inter_model as IM     # noqa: E402
import modes_model as MM           # noqa: E402
import svt_testlib as T            # noqa: E402
import tokenize_model as TM        # noqa: E402

REF = os.environ.get("SVT_REFERENCE", "/root/reference")


def build_driver(td):
    rs = os.path.join(REF, "Source")
    rl = os.path.join(rs, "Lib")
    obj = os.path.join(T.REF_DIR, "obj")
    exe = os.path.join(td, "ref_modes_inter")
    inc = [os.path.join(T.REF_DIR, "gen"), os.path.join(rs, "API")] + [os.path.join(rl, d) for d in ("VPX", "Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    objs = [os.path.join(obj, n + ".o") for n in ("vp9_tokenize", "vp9_entropy", "vp9_treewriter", "vp9_common_data", "vp9_blockd")]
    cmd = ["gcc", "-std=gnu99", "-O2", "-w"] + [f"-I{d}" for d in inc] + ["-no-pie", "-Wl,-z,lazy", "-Wl,--unresolved-symbols=ignore-all", "-o", exe,
                                                                      os.path.join(T.ROOT, "tests", "c", "ref_modes_inter_driver.c")] + objs + ["-lm"]
    subprocess.check_call(cmd)
    return exe


def run_reference(exe, td, pictures):
    """pictures: [(picture dict, token records, runs)] -> (tables, [compound references], [tile bytes], [mode-info bytes], [seconds], coverage)"""
    req, rsp = os.path.join(td, "req.bin"), os.path.join(td, "rsp.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<2i", 0x49444f4d, len(pictures)))
        for p, tokens, runs in pictures:
            fr = p["frame"]
            f.write(struct.pack("<9i", p["W"], p["H"], len(tokens), fr["reference_mode"], fr["allow_hp"], *fr["sign_bias"]))
            for k in ("lf_mi", "mc_mi", "ext"):
                f.write(np.ascontiguousarray(p[k]).tobytes())
            tok, row, extra = BM.unpack(tokens)
            # the reference holds EXTRABIT as int16
            f.write(np.stack([tok, extra.astype(np.uint16).view(np.int16).astype(np.int64), row], axis=1).astype("<i4").tobytes())
            f.write(np.ascontiguousarray(runs, "<i4").tobytes())
    subprocess.check_call([exe, req, rsp])
    raw = open(rsp, "rb").read()
    tables, pos = {}, 0
    for name, shape in IM.TABLE_SHAPES + (("coef_probs", (1728,)), ("pareto", (255, 8)), ("cat_probs", (6, 14))):
        n = int(np.prod(shape))
        tables[name] = np.frombuffer(raw, np.uint8, n, pos).reshape(shape).copy()
        pos += n
    refs, tiles, modes, secs = [], [], [], []
    for _ in pictures:
        refs.append(struct.unpack_from("<3i", raw, pos))
        pos += 12
        for dst in (tiles, modes):
            size = struct.unpack_from("<I", raw, pos)[0]
            dst.append(np.frombuffer(raw, np.uint8, size, pos + 4).copy())
            pos += 4 + size
        secs.append(struct.unpack_from("<d", raw, pos)[0])
        pos += 8
    words = np.frombuffer(raw, "<u4", len(IM.COVER_KEYS), pos)
    assert pos + 4 * len(IM.COVER_KEYS) == len(raw)
    cov = {k: {b for b in range(32) if (int(w) >> b) & 1} for k, w in zip(IM.COVER_KEYS, words)}
    cov["mode"] = {10 + b for b in cov["mode"]}          # the driver notes INTER_OFFSET(mode)
    return tables, refs, tiles, modes, secs, cov


def main():
    made, pictures = [], []
    for name, W, H, kind, seed, fr, p_intra in IM.PICTURES:
        p = IM.make_picture(W, H, kind, seed, fr, p_intra)
        tok = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], W, H, counts=False)
        runs = MM.leaf_runs(p["lf_mi"], tok["tok_off"], p["eob_map"], W, H)
        assert int(runs[..., 1].sum()) == len(tok["tokens"])        # every token belongs to exactly one leaf
        made.append((name, p))
        pictures.append((p, tok["tokens"], runs))
    with tempfile.TemporaryDirectory() as td:
        tables, refs, tiles, modes, secs, ref_cov = run_reference(build_driver(td), td, pictures)
    # the tables the bool coder's fixture holds are the same reference tables
    for n in ("coef_probs", "pareto", "cat_probs"):
        assert np.array_equal(tables[n], BM.fixture()[n]), n
    out = {n: tables[n] for n, _ in IM.TABLE_SHAPES}
    model_cov = {}
    for (name, p), ref, tile, mode, sec in zip(made, refs, tiles, modes, secs):
        fr = p["frame"]
        assert (fr["comp_fixed_ref"], *fr["comp_var_ref"]) == tuple(ref), (name, ref)      # the reference's own derivation
        recs, leaves = IM.serial_walk(p, tables, model_cov)
        print(f"{name}: {len(leaves)} leaves, {len(recs)} mode-info bools, tile {len(tile)} bytes, mode info alone {len(mode)} bytes, reference {sec * 1e6:.1f} us")
        out[f"size|{name}"] = np.array([p["W"], p["H"]], np.int32)
        out[f"frame|{name}"] = np.array([fr["reference_mode"], fr["allow_hp"], *fr["sign_bias"], fr["comp_fixed_ref"], *fr["comp_var_ref"]], np.int32)
        for k in ("lf_mi", "mc_mi", "ext"):
            out[f"{k}|{name}"] = np.ascontiguousarray(p[k]).view(np.uint8)
        out[f"qcoeff|{name}"], out[f"eob_map|{name}"] = p["qcoeff"], p["eob_map"]
        out[f"tile_bytes|{name}"], out[f"modes_bytes|{name}"] = tile, mode
    out["names"] = np.array([m[0] for m in made])
    out["seconds"] = np.array(secs, np.float64)
    out["coverage"] = np.array([sum(1 << (b - (10 if k == "mode" else 0)) for b in ref_cov[k]) for k in IM.COVER_KEYS], np.uint32)
    print("reference:", {k: sorted(v) for k, v in ref_cov.items()})
    missing = IM.coverage_complete(ref_cov)
    assert not missing, f"the reference did not meet: {missing}"
    assert {k: set(v) for k, v in model_cov.items()} == ref_cov, "the model's notes differ from the reference's"
    np.savez_compressed(IM.GOLD, **out)
    print(IM.GOLD, os.path.getsize(IM.GOLD), "bytes")


if __name__ == "__main__":
    main()

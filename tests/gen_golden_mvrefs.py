"""Writes tests/golden/mvrefs_reference.npz: the seeded pictures of tests/mvrefs_model.py -- the three grids, the restrict flag, the sign
biases -- and what the REFERENCE derives from them: eb_vp9_find_mv_refs' two candidates, return value and mode context for every leaf
of 8x8 or larger and every reference frame, and the seconds one pass over the picture took.  The reference runs in
tests/c/ref_mvrefs_driver.c, compiled here against the reference's headers into a temporary directory; only inputs and recorded results
are stored.

The model (mvrefs_model.find_mv_refs) must equal the reference for every leaf, reference frame and picture; its coverage notes, pinned
to the reference that way, must reach everything mvrefs_model.coverage_complete names.  The self-consistent pictures carry the derived
reference MVs and mode contexts in their extension records; for them the reference's tile bytes are recorded too, by the driver of
tests/gen_golden_modes_inter.py (write_partition, pack_inter_mode_mvs, pack_mb_tokens between eb_vp9_start_encode and
eb_vp9_stop_encode).

    python tests/gen_golden_mvrefs.py            (needs the reference sources and oracle/_ref)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_modes_inter as GI   # noqa: E402
import modes_inter_model as IM        # noqa: E402
import modes_model as MM              # noqa: E402
import mvrefs_model as M              # noqa: E402
import svt_testlib as T               # noqa: E402
import tokenize_model as TM           # noqa: E402

B = T.B


def build_driver(td):
    rs = os.path.join(GI.REF, "Source")
    rl = os.path.join(rs, "Lib")
    exe = os.path.join(td, "ref_mvrefs")
    inc = [os.path.join(T.REF_DIR, "gen"), os.path.join(rs, "API")] + [os.path.join(rl, d) for d in ("VPX", "Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    cmd = ["gcc", "-std=gnu99", "-O2", "-w"] + [f"-I{d}" for d in inc] + ["-no-pie", "-Wl,-z,lazy", "-Wl,--unresolved-symbols=ignore-all", "-o", exe,
                                                                      os.path.join(T.ROOT, "tests", "c", "ref_mvrefs_driver.c"), os.path.join(T.REF_DIR, "obj", "vp9_common_data.o"), "-lm"]
    subprocess.check_call(cmd)
    return exe


def run_reference(exe, td, pictures):
    """[picture dict] -> ([candidate records of every unit], [seconds])"""
    req, rsp = os.path.join(td, "mvr_req.bin"), os.path.join(td, "mvr_rsp.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<2i", 0x5246564d, len(pictures)))
        for p in pictures:
            f.write(struct.pack("<7i", p["W"], p["H"], p["restrict"], *p["frame"]["sign_bias"]))
            for k in ("lf_mi", "mc_mi", "ext"):
                f.write(np.ascontiguousarray(p[k]).tobytes())
    subprocess.check_call([exe, req, rsp])
    raw = open(rsp, "rb").read()
    cands, secs, pos = [], [], 0
    for p in pictures:
        shape = (p["H"] // 8, p["W"] // 8)
        n = shape[0] * shape[1]
        cands.append(np.frombuffer(raw, B.MVREF_CAND_DTYPE, n, pos).reshape(shape).copy())
        pos += 32 * n
        secs.append(struct.unpack_from("<d", raw, pos)[0])
        pos += 8
    assert pos == len(raw)
    return cands, secs


def main():
    pics = M.build_pictures()
    names = list(pics)
    cov = M.new_cover()
    model = [M.derive_picture(pics[n], cov) for n in names]
    consistent = [n for n in names if pics[n]["consistent"]]
    toks = {}
    for n in consistent:
        p = pics[n]
        assert np.array_equal(model[names.index(n)]["ext_out"], p["ext"]), n       # the extension records hold exactly what is derived
        assert model[names.index(n)]["status"][0] == 0, n
        tok = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], counts=False)
        runs = MM.leaf_runs(p["lf_mi"], tok["tok_off"], p["eob_map"], p["W"], p["H"])
        assert int(runs[..., 1].sum()) == len(tok["tokens"])
        toks[n] = (p, tok["tokens"], runs)
    with tempfile.TemporaryDirectory() as td:
        cands, secs = run_reference(build_driver(td), td, [pics[n] for n in names])
        tables, refs, tiles, _, _, _ = GI.run_reference(GI.build_driver(td), td, [toks[n] for n in consistent])
    for n, _ in IM.TABLE_SHAPES:                                                   # the tables the inter stage's fixture holds
        assert np.array_equal(tables[n], IM.fixture()[n]), n
    out = {}
    for n, m, ref, sec in zip(names, model, cands, secs):
        p = pics[n]
        bad = np.argwhere(m["cand"] != ref)
        assert not len(bad), (n, bad[:4], m["cand"][tuple(bad[0])], ref[tuple(bad[0])])          # model == reference, every leaf and frame
        leaves = int((ref["count"][..., 0] != 0xFF).sum())
        print(f"{n}: {leaves} leaves of 8x8 or larger, status {m['status']}, reference {sec * 1e6:.1f} us")
        out[f"size|{n}"] = np.array([p["W"], p["H"]], np.int32)
        out[f"params|{n}"] = np.array([p["restrict"], *p["frame"]["sign_bias"], p["frame"]["reference_mode"], p["consistent"]], np.int32)
        for k in ("lf_mi", "mc_mi", "ext"):
            out[f"{k}|{n}"] = np.ascontiguousarray(p[k]).view(np.uint8)
        out[f"cand|{n}"] = ref.view(np.uint8)
        out[f"ext_out|{n}"] = np.ascontiguousarray(m["ext_out"]).view(np.uint8)     # (a function of the grid and the reference's records above)
        out[f"status|{n}"] = np.array(m["status"], np.uint32)
    for n, ref, tile in zip(consistent, refs, tiles):
        p = pics[n]
        fr = p["frame"]
        assert (fr["comp_fixed_ref"], *fr["comp_var_ref"]) == tuple(ref), (n, ref)
        idx = np.flatnonzero(p["qcoeff"]).astype(np.uint32)
        out[f"q_idx|{n}"], out[f"q_val|{n}"], out[f"eob_map|{n}"], out[f"tile_bytes|{n}"] = idx, p["qcoeff"][idx], p["eob_map"], tile
        print(f"{n}: tile {len(tile)} bytes")
    out["names"] = np.array(names)
    out["seconds"] = np.array(secs, np.float64)
    print("coverage:", {k: sorted(v, key=str) for k, v in cov.items()})
    missing = M.coverage_complete(cov)
    assert not missing, f"the fixture does not meet: {missing}"
    np.savez_compressed(M.GOLD, **out)
    print(M.GOLD, os.path.getsize(M.GOLD), "bytes")


if __name__ == "__main__":
    main()

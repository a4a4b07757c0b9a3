"""Writes tests/golden/md_inter_reference.npz: the seeded pictures of tests/md_inter_model.py (GOLDEN) -- the two grids, the frame
parameters, list_ref_frame, coefficients, eob map -- and what the REFERENCE makes of them: the extension records that come out of
eb_vp9_find_mv_refs per leaf and reference frame and the four-way comparison on its int_mv values (tests/c/ref_md_inter_driver.c), and
the bytes of the tile it writes for those records -- write_partition, pack_inter_mode_mvs and pack_mb_tokens per block between
eb_vp9_start_encode and eb_vp9_stop_encode, by the driver of tests/gen_golden_modes_inter.py.  Next to each tile the byte count of the
same picture with every inter leaf labelled NEWMV is recorded (coded by the same driver): a record of what the labels save on these
pictures, not a claim about real content.  Both drivers are compiled here against the reference's headers into a temporary directory;
only inputs and recorded results are stored.

The model (md_inter_model.label_picture) must give the reference's records for every picture.

    python tests/gen_golden_md_inter.py            (needs the reference sources and oracle/_ref)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_modes_inter as GI   # noqa: E402
import md_inter_model as D            # noqa: E402
import modes_inter_model as IM        # noqa: E402
import modes_model as MM              # noqa: E402
import svt_testlib as T               # noqa: E402
import tokenize_model as TM           # noqa: E402

B = T.B


def build_driver(td):
    rs = os.path.join(GI.REF, "Source")
    rl = os.path.join(rs, "Lib")
    exe = os.path.join(td, "ref_md_inter")
    inc = [os.path.join(T.REF_DIR, "gen"), os.path.join(rs, "API")] + [os.path.join(rl, d) for d in ("VPX", "Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    cmd = ["gcc", "-std=gnu99", "-O2", "-w"] + [f"-I{d}" for d in inc] + ["-no-pie", "-Wl,-z,lazy", "-Wl,--unresolved-symbols=ignore-all", "-o", exe,
                                                                      os.path.join(T.ROOT, "tests", "c", "ref_md_inter_driver.c"), os.path.join(T.REF_DIR, "obj", "vp9_common_data.o"), "-lm"]
    subprocess.check_call(cmd)
    return exe


def run_reference(exe, td, pictures):
    """[picture dict] -> [the labelled extension records of every unit]"""
    req, rsp = os.path.join(td, "mdi_req.bin"), os.path.join(td, "mdi_rsp.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<2i", 0x49444d4c, len(pictures)))
        for p in pictures:
            f.write(struct.pack("<9i", p["W"], p["H"], p["restrict"], *p["frame"]["sign_bias"], *p["lrf"]))
            for k in ("lf_mi", "mc_mi"):
                f.write(np.ascontiguousarray(p[k]).tobytes())
    subprocess.check_call([exe, req, rsp])
    raw = open(rsp, "rb").read()
    exts, pos = [], 0
    for p in pictures:
        shape = (p["H"] // 8, p["W"] // 8)
        n = shape[0] * shape[1]
        exts.append(np.frombuffer(raw, B.MI_INTER_EXT_DTYPE, n, pos).reshape(shape).copy())
        pos += 12 * n
    assert pos == len(raw)
    return exts


def main():
    pics = D.build_golden_pictures()
    names = list(pics)
    with tempfile.TemporaryDirectory() as td:
        exts = run_reference(build_driver(td), td, [pics[n] for n in names])
        jobs = []
        for n, ext in zip(names, exts):
            p = pics[n]
            m = D.label_picture(p)
            assert np.array_equal(m["ext_out"], ext), n                            # model == reference, every record
            assert not m["unfaithful"], n
            tok = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], counts=False)
            runs = MM.leaf_runs(p["lf_mi"], tok["tok_off"], p["eob_map"], p["W"], p["H"])
            assert int(runs[..., 1].sum()) == len(tok["tokens"])
            jobs.append((dict(p, ext=ext), tok["tokens"], runs))
            jobs.append((dict(p, ext=D.all_newmv(p, ext)), tok["tokens"], runs))
        tables, refs, tiles, _, _, _ = GI.run_reference(GI.build_driver(td), td, jobs)
    for n, _ in IM.TABLE_SHAPES:                                                   # the tables the inter stage's fixture holds
        assert np.array_equal(tables[n], IM.fixture()[n]), n
    out = {}
    for i, (n, ext) in enumerate(zip(names, exts)):
        p, fr = pics[n], pics[n]["frame"]
        assert (fr["comp_fixed_ref"], *fr["comp_var_ref"]) == tuple(refs[2 * i]), (n, refs[2 * i])
        tile, plain = tiles[2 * i], tiles[2 * i + 1]
        modes = ext["mode"][ext["mode"] >= 10]
        print(f"{n}: {len(modes)} inter leaves, labels {[int((modes == v).sum()) for v in (10, 11, 12, 13)]}, tile {len(tile)} bytes, labelled all-NEWMV {len(plain)} bytes")
        out[f"size|{n}"] = np.array([p["W"], p["H"]], np.int32)
        out[f"params|{n}"] = np.array([p["restrict"], *fr["sign_bias"], fr["reference_mode"], fr["allow_hp"], *p["lrf"], fr["comp_fixed_ref"], *fr["comp_var_ref"]], np.int32)
        for k in ("lf_mi", "mc_mi"):
            out[f"{k}|{n}"] = np.ascontiguousarray(p[k]).view(np.uint8)
        out[f"ext|{n}"] = np.ascontiguousarray(ext).view(np.uint8)
        idx = np.flatnonzero(p["qcoeff"]).astype(np.uint32)
        out[f"q_idx|{n}"], out[f"q_val|{n}"], out[f"eob_map|{n}"] = idx, p["qcoeff"][idx], p["eob_map"]
        out[f"tile_bytes|{n}"], out[f"all_newmv_bytes|{n}"] = tile, np.array(len(plain), np.int32)
    out["names"] = np.array(names)
    np.savez_compressed(D.GOLD, **out)
    print(D.GOLD, os.path.getsize(D.GOLD), "bytes")


if __name__ == "__main__":
    main()

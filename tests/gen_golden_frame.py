"""Writes tests/golden/frame_reference.npz: the frame parameters of tests/frame_model.py's cases and what the REFERENCE's
eb_vp9_pack_bitstream (VPX/vp9_bitstream.c:1369-1412) makes of them -- the uncompressed header, first_part_size and the compressed
header of every header case (an empty entropy-coder stream behind them), the one-byte show-existing frames, and the whole frames of the
group-11 cases, whose entropy-coder stream is the tile the fixtures modes_reference.npz / modes_inter_reference.npz recorded from the
reference.  The reference runs in tests/c/ref_frame_driver.c, compiled here against the reference's headers into a temporary directory
and linked with the objects `make -C oracle ref` builds; only parameters and recorded bytes are stored.

The driver notes from the reference's own structures which branches of the two header writers each case takes; the generator fails
unless every branch is reached.

    python tests/gen_golden_frame.py            (needs the reference sources and oracle/_ref)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_model as FM           # noqa: E402
import svt_testlib as T            # noqa: E402

REF = os.environ.get("SVT_REFERENCE", "/root/reference")
# enum ucov / enum ccov of the driver
UCOV = ("key", "intra_only", "inter", "hidden", "shown", "resilient_0", "resilient_1", "render_same", "render_differs", "lf_deltas_off", "lf_no_update", "lf_update",
        "lf_changed_pos", "lf_changed_neg", "lf_unchanged", "dq_zero", "dq_neg", "dq_pos", "tile_bit_0", "tile_bit_1", "show_existing")
CCOV = ("intra", "inter", "comp_not_allowed", "comp_single", "comp_compound", "comp_hybrid", "single_refs", "no_single_refs", "comp_refs", "no_comp_refs", "hp_0", "hp_1")


def build_driver(td):
    rs = os.path.join(REF, "Source")
    rl = os.path.join(rs, "Lib")
    obj = os.path.join(T.REF_DIR, "obj")
    exe = os.path.join(td, "ref_frame")
    inc = [os.path.join(T.REF_DIR, "gen"), os.path.join(rs, "API")] + [os.path.join(rl, d) for d in ("VPX", "Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    objs = [os.path.join(obj, n + ".o") for n in ("vp9_tokenize", "vp9_entropy", "vp9_treewriter", "vp9_common_data", "vp9_blockd", "vp9_cost")]
    cmd = ["gcc", "-std=gnu99", "-O2", "-w"] + [f"-I{d}" for d in inc] + ["-no-pie", "-Wl,-z,lazy", "-Wl,--unresolved-symbols=ignore-all", "-o", exe,
                                                                      os.path.join(T.ROOT, "tests", "c", "ref_frame_driver.c")] + objs + ["-lm"]
    subprocess.check_call(cmd)
    return exe


def run_reference(exe, td, cases):
    """cases: [("show", slot) | ("frame", parameters, tile bytes)] -> ([(frame bytes, uncompressed bytes, first_part_size)], coverage names)"""
    req, rsp = os.path.join(td, "req.bin"), os.path.join(td, "rsp.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<2i", 0x4d415246, len(cases)))
        for c in cases:
            if c[0] == "show":
                f.write(struct.pack("<2i", 1, c[1]))
            else:
                f.write(struct.pack(f"<i{FM.N_VALUES}ii", 0, *FM.flat(c[1]), len(c[2])))
                f.write(c[2])
    subprocess.check_call([exe, req, rsp])
    raw = open(rsp, "rb").read()
    out, pos = [], 0
    for _ in cases:
        size = struct.unpack_from("<I", raw, pos)[0]
        frame = raw[pos + 4:pos + 4 + size]
        ub, cb = struct.unpack_from("<2I", raw, pos + 4 + size)
        out.append((frame, ub, cb))
        pos += 12 + size
    u, c = struct.unpack_from("<2I", raw, pos)
    assert pos + 8 == len(raw)
    return out, {n for b, n in enumerate(UCOV) if (u >> b) & 1} | {"c_" + n for b, n in enumerate(CCOV) if (c >> b) & 1}


def main():
    cases = [("frame", p, b"") for _, p in FM.CASES] + [("show", s) for s in FM.SHOW_EXISTING_SLOTS] + [("frame", p, FM.whole_tile(kind, pic)) for _, kind, pic, p in FM.WHOLE]
    names = [n for n, _ in FM.CASES] + [f"show_existing_{s}" for s in FM.SHOW_EXISTING_SLOTS] + [n for n, *_ in FM.WHOLE]
    assert len(set(names)) == len(names)
    with tempfile.TemporaryDirectory() as td:
        got, cov = run_reference(build_driver(td), td, cases)
    missing = (set(UCOV) | {"c_" + n for n in CCOV}) - cov
    assert not missing, f"the reference did not reach: {sorted(missing)}"
    out = {"names": np.array(names)}
    for name, case, (frame, ub, cb) in zip(names, cases, got):
        out[f"frame|{name}"] = np.frombuffer(frame, np.uint8)
        if case[0] == "show":
            assert len(frame) == 1
            continue
        out[f"params|{name}"] = np.array(FM.flat(case[1]), np.int32)
        out[f"lengths|{name}"] = np.array([ub, cb], np.int32)
        assert len(frame) == ub + cb + len(case[2]) and frame[ub + cb:] == case[2]
        print(f"{name}: uncompressed {ub} bytes, compressed {cb} bytes, frame {len(frame)} bytes")
    out["coverage"] = np.array(sorted(cov))
    print("reference reached:", sorted(cov))
    print("longest header:", max(int(out[k].sum()) for k in out if k.startswith("lengths|")), "bytes")
    np.savez_compressed(FM.GOLD, **out)
    print(FM.GOLD, os.path.getsize(FM.GOLD), "bytes")


if __name__ == "__main__":
    main()

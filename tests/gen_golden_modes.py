"""Writes tests/golden/modes_reference.npz: the seeded key-frame pictures of tests/modes_model.py -- grid, coefficients, eob map -- and
what the REFERENCE makes of them: the bytes of the whole tile (write_partition, write_mb_modes_kf and pack_mb_tokens per block between
eb_vp9_start_encode and eb_vp9_stop_encode), the bytes of the mode-info bools alone (the same walk, tokens left out), the four tables it
codes modes with (eb_vp9_kf_y_mode_prob, eb_vp9_kf_uv_mode_prob, eb_vp9_kf_partition_probs, the default skip probabilities) and the
seconds one pass of its tile coding took.  The token records sent to the reference come from svt_hip_tokenize_picture, the host form
tests/golden/tokens_reference.npz pins to the reference.  The reference runs in tests/c/ref_modes_driver.c, compiled here against the
reference's headers into a temporary directory and linked with the objects `make -C oracle ref` builds; only inputs and recorded
results are stored.

    python tests/gen_golden_modes.py            (needs the reference sources and oracle/_ref)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boolcode_model as BM   # noqa: E402
import modes_model as MM      # noqa: E402
import svt_testlib as T       # noqa: E402
import tokenize_model as TM   # noqa: E402

REF = os.environ.get("SVT_REFERENCE", "/root/reference")
TABLES = (("kf_y_mode_prob", (10, 10, 9)), ("kf_uv_mode_prob", (10, 9)), ("kf_partition_probs", (16, 3)), ("skip_probs", (3,)))


def build_driver(td):
    rs = os.path.join(REF, "Source")
    rl = os.path.join(rs, "Lib")
    obj = os.path.join(T.REF_DIR, "obj")
    exe = os.path.join(td, "ref_modes")
    inc = [os.path.join(T.REF_DIR, "gen"), os.path.join(rs, "API")] + [os.path.join(rl, d) for d in ("VPX", "Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    objs = [os.path.join(obj, n + ".o") for n in ("vp9_tokenize", "vp9_entropy", "vp9_treewriter", "vp9_common_data", "vp9_blockd")]
    cmd = ["gcc", "-std=gnu99", "-O2", "-w"] + [f"-I{d}" for d in inc] + ["-no-pie", "-Wl,-z,lazy", "-Wl,--unresolved-symbols=ignore-all", "-o", exe,
                                                                      os.path.join(T.ROOT, "tests", "c", "ref_modes_driver.c")] + objs + ["-lm"]
    subprocess.check_call(cmd)
    return exe


def run_reference(exe, td, pictures):
    """pictures: [(W, H, lf_mi, token records, runs)] -> (tables, [tile bytes], [mode-info bytes], [seconds])"""
    req, rsp = os.path.join(td, "req.bin"), os.path.join(td, "rsp.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<2i", 0x45444f4d, len(pictures)))
        for W, H, lf, tokens, runs in pictures:
            f.write(struct.pack("<3i", W, H, len(tokens)))
            f.write(np.ascontiguousarray(lf[:, :W // 8]).tobytes())
            tok, row, extra = BM.unpack(tokens)
            # the reference holds EXTRABIT as int16
            f.write(np.stack([tok, extra.astype(np.uint16).view(np.int16).astype(np.int64), row], axis=1).astype("<i4").tobytes())
            f.write(np.ascontiguousarray(runs, "<i4").tobytes())
    subprocess.check_call([exe, req, rsp])
    raw = open(rsp, "rb").read()
    tables, pos = {}, 0
    for name, shape in TABLES + (("coef_probs", (1728,)), ("pareto", (255, 8)), ("cat_probs", (6, 14))):
        n = int(np.prod(shape))
        tables[name] = np.frombuffer(raw, np.uint8, n, pos).reshape(shape).copy()
        pos += n
    tiles, modes, secs = [], [], []
    for _ in pictures:
        for dst in (tiles, modes):
            size = struct.unpack_from("<I", raw, pos)[0]
            dst.append(np.frombuffer(raw, np.uint8, size, pos + 4).copy())
            pos += 4 + size
        secs.append(struct.unpack_from("<d", raw, pos)[0])
        pos += 8
    assert pos == len(raw)
    return tables, tiles, modes, secs


def check_coverage(cov, lf_all):
    """every row of kf_partition_probs, every skip context, every (above, left) class pair; every leaf size coded at least once"""
    classes = ("missing", "4x4", "larger")
    assert cov["partition"] == set(range(16)), sorted(set(range(16)) - cov["partition"])
    assert cov["skip"] == {0, 1, 2}, cov["skip"]
    assert cov["pairs"] == {(a, b) for a in classes for b in classes}, cov["pairs"]
    coded = {int(t) for lf in lf_all for t in np.unique(lf["sb_type"][lf["skip"] == 0])}
    skipped = {int(t) for lf in lf_all for t in np.unique(lf["sb_type"][lf["skip"] == 1])}
    assert coded == set(MM.LEAF_TYPES) and skipped, (coded, skipped)


def main():
    made, pictures = [], []
    for name, W, H, kind, seed in MM.PICTURES:
        lf, q, emap = MM.make_picture(W, H, kind, seed)
        tok = TM.host_tokenize_picture(lf, q, emap, W, H, counts=False)
        runs = MM.leaf_runs(lf, tok["tok_off"], emap, W, H)
        assert int(runs[..., 1].sum()) == len(tok["tokens"])        # every token belongs to exactly one leaf
        made.append((name, W, H, lf, q, emap))
        pictures.append((W, H, lf, tok["tokens"], runs))
    with tempfile.TemporaryDirectory() as td:
        tables, tiles, modes, secs = run_reference(build_driver(td), td, pictures)
    # the tables the bool coder's fixture holds are the same reference tables
    for n in ("coef_probs", "pareto", "cat_probs"):
        assert np.array_equal(tables[n], BM.fixture()[n]), n
    out = {n: tables[n] for n, _ in TABLES}
    cov = {}
    for (name, W, H, lf, q, emap), tile, mode, sec in zip(made, tiles, modes, secs):
        recs, leaves = MM.serial_walk(lf, W, H, tables, cov)
        print(f"{name}: {len(leaves)} leaves, {len(recs)} mode-info bools, tile {len(tile)} bytes, mode info alone {len(mode)} bytes, reference {sec * 1e6:.1f} us")
        out[f"size|{name}"] = np.array([W, H], np.int32)
        out[f"lf_mi|{name}"], out[f"qcoeff|{name}"], out[f"eob_map|{name}"] = np.ascontiguousarray(lf).view(np.uint8), q, emap
        out[f"tile_bytes|{name}"], out[f"modes_bytes|{name}"] = tile, mode
    out["names"] = np.array([m[0] for m in made])
    out["seconds"] = np.array(secs, np.float64)
    print({k: sorted(v) for k, v in cov.items()})
    check_coverage(cov, [m[3] for m in made])
    np.savez_compressed(MM.GOLD, **out)
    print(MM.GOLD, os.path.getsize(MM.GOLD), "bytes")


if __name__ == "__main__":
    main()

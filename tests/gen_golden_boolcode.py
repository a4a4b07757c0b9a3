"""Writes tests/golden/boolcode_reference.npz: what the REFERENCE's bool coder makes of the streams the bool-coder tests share -- its
pack_mb_tokens + eb_vp9_stop_encode over the three token streams of tests/golden/tokens_reference.npz (in that fixture's order) and
over the token-level cases, its vpx_write over the raw bool streams of tests/boolcode_model.py -- together with the three tables it
codes tokens with (coef_probs after eb_vp9_default_coef_probs, eb_vp9_pareto8_full, the categories' bit probabilities) and the seconds
one pass of its packing took.  The reference runs in tests/c/ref_boolcode_driver.c, compiled here against the reference's headers
into a temporary directory and linked with the objects `make -C oracle ref` builds; only inputs and recorded results are stored.

    python tests/gen_golden_boolcode.py            (needs the reference sources and oracle/_ref)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boolcode_model as BM   # noqa: E402
import svt_testlib as T       # noqa: E402

REF = os.environ.get("SVT_REFERENCE", "/root/reference")


def build_driver(td):
    rs = os.path.join(REF, "Source")
    rl = os.path.join(rs, "Lib")
    obj = os.path.join(T.REF_DIR, "obj")
    exe = os.path.join(td, "ref_boolcode")
    inc = [os.path.join(T.REF_DIR, "gen"), os.path.join(rs, "API")] + [os.path.join(rl, d) for d in ("VPX", "Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    objs = [os.path.join(obj, n + ".o") for n in ("vp9_tokenize", "vp9_entropy", "vp9_treewriter", "vp9_common_data")]
    cmd = ["gcc", "-std=gnu99", "-O2", "-w"] + [f"-I{d}" for d in inc] + ["-no-pie", "-Wl,-z,lazy", "-Wl,--unresolved-symbols=ignore-all", "-o", exe,
                                                                      os.path.join(T.ROOT, "tests", "c", "ref_boolcode_driver.c")] + objs + ["-lm"]
    subprocess.check_call(cmd)
    return exe


def run_reference(exe, td, streams):
    """streams: [(kind, array)]: kind 0 = uint32 token records, kind 1 = uint16 bool records -> (tables, [bytes], [seconds])"""
    req, rsp = os.path.join(td, "req.bin"), os.path.join(td, "rsp.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<2i", 0x4c4f4f42, len(streams)))
        for kind, a in streams:
            f.write(struct.pack("<2i", kind, len(a)))
            if kind == 0:
                tok, row, extra = BM.unpack(a)
                # the reference holds EXTRABIT as int16
                f.write(np.stack([tok, extra.astype(np.uint16).view(np.int16).astype(np.int64), row], axis=1).astype("<i4").tobytes())
            else:
                f.write(np.asarray(a, "<u2").tobytes())
    subprocess.check_call([exe, req, rsp])
    raw = open(rsp, "rb").read()
    tables = dict(coef_probs=np.frombuffer(raw, np.uint8, 576 * 3, 0).copy(), pareto=np.frombuffer(raw, np.uint8, 255 * 8, 576 * 3).reshape(255, 8).copy(),
                  cat_probs=np.frombuffer(raw, np.uint8, 84, 576 * 3 + 255 * 8).reshape(6, 14).copy())
    pos, out, secs = 576 * 3 + 255 * 8 + 84, [], []
    for _ in streams:
        size = struct.unpack_from("<I", raw, pos)[0]
        out.append(np.frombuffer(raw, np.uint8, size, pos + 4).copy())
        secs.append(struct.unpack_from("<d", raw, pos + 4 + size)[0])
        pos += 12 + size
    assert pos == len(raw)
    return tables, out, secs


def main():
    raw = BM.raw_streams()
    tok_streams = BM.fixture_token_streams()
    cases = BM.token_cases()
    streams = [(0, t) for t in tok_streams] + [(0, cases)] + [(1, a) for a in raw.values()]
    with tempfile.TemporaryDirectory() as td:
        tables, coded, secs = run_reference(build_driver(td), td, streams)
    out = dict(tables)
    n_bools = []
    for k, t in enumerate(tok_streams):
        out[f"token_bytes|{k}"] = coded[k]
        n_bools.append(len(BM.expand(t, None, None, tables)))
        print(f"token stream {k}: {len(t)} records, {n_bools[-1]} bools, {len(coded[k])} bytes, reference {secs[k] * 1e6:.1f} us")
    out["token_records"] = np.array([len(t) for t in tok_streams], np.int32)
    out["token_bools"] = np.array(n_bools, np.int32)
    out["token_seconds"] = np.array(secs[:len(tok_streams)], np.float64)
    out["cases_bytes"] = coded[len(tok_streams)]
    for name, c in zip(raw, coded[len(tok_streams) + 1:]):
        out[f"raw_bytes|{name}"] = c
    np.savez_compressed(BM.GOLD, **out)
    print(BM.GOLD, os.path.getsize(BM.GOLD), "bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/coef_update_reference.npz: token streams (and "old" probability tables) of tests/coef_update_model.py's cases and
what the REFERENCE's write_compressed_header (VPX/vp9_bitstream.c:1292-1367) makes of their counts under TWO_LOOP with
coeff_prob_appx_step 1 -- the compressed header's bytes and cm->fc->coef_probs afterwards -- plus the reference's tables: eb_vp9_prob_cost
and, for all 255 x 255 (newp, oldp) pairs, remap_prob and the bits of prob_diff_update_cost.  The reference runs in
tests/c/ref_coef_update_driver.c, compiled here against the reference's headers into a temporary directory and linked with the objects
`make -C oracle ref` builds; only inputs and recorded results are stored.

The driver notes which TWO_LOOP exits and which arms of encode_term_subexp / encode_uniform the reference takes; the generator fails
unless every one is reached.  Through the model it asserts that no sum of any recorded case reaches 2^31: the reference's 32-bit sums
did not wrap, so equality with the product's 64-bit sums is a fair demand on every case here.

Beside each real-stream case the frame's bytes with and without updates (the all-host chain) are recorded: a record of those small
pictures, not a claim.

    python tests/gen_golden_coef_update.py            (needs the reference sources and oracle/_ref)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boolcode_model as BM        # noqa: E402
import coef_update_model as CM     # noqa: E402
import svt_testlib as T            # noqa: E402

REF = os.environ.get("SVT_REFERENCE", "/root/reference")
COV = ("not_searched", "no_entry", "negative", "sent", "subexp_16", "subexp_32", "subexp_64", "uniform_short", "uniform_long", "newp_above", "newp_below")
KEY, INTER, INTER_SELECT_HP = (0, 0, 0, 0), (1, 0, 0, 0), (1, 2, 1, 1)


def build_driver(td):
    rs = os.path.join(REF, "Source")
    rl = os.path.join(rs, "Lib")
    obj = os.path.join(T.REF_DIR, "obj")
    exe = os.path.join(td, "ref_coef_update")
    inc = [os.path.join(T.REF_DIR, "gen"), os.path.join(rs, "API")] + [os.path.join(rl, d) for d in ("VPX", "Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    objs = [os.path.join(obj, n + ".o") for n in ("vp9_tokenize", "vp9_entropy", "vp9_treewriter", "vp9_common_data", "vp9_blockd", "vp9_cost")]
    cmd = ["gcc", "-std=gnu99", "-O2", "-w"] + [f"-I{d}" for d in inc] + ["-no-pie", "-Wl,-z,lazy", "-Wl,--unresolved-symbols=ignore-all", "-o", exe,
                                                                      os.path.join(T.ROOT, "tests", "c", "ref_coef_update_driver.c")] + objs + ["-lm"]
    subprocess.check_call(cmd)
    return exe


def run_reference(exe, td, cases):
    """cases: [(frame 4-tuple, tx_totals, counts, eob, old)] -> ([dict(bytes, probs, exits, updates, savings)], tables dict, coverage names)"""
    req, rsp = os.path.join(td, "req.bin"), os.path.join(td, "rsp.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<2i", 0x44505543, len(cases)))
        for fr, tot, counts, eob, old in cases:
            f.write(struct.pack("<4i4I", *fr, *tot))
            f.write(np.ascontiguousarray(counts, np.uint32).tobytes())
            f.write(np.ascontiguousarray(eob, np.uint32).tobytes())
            f.write(np.ascontiguousarray(old, np.uint8).tobytes())
    subprocess.check_call([exe, req, rsp])
    raw = open(rsp, "rb").read()
    out, pos = [], 0
    for _ in cases:
        size = struct.unpack_from("<I", raw, pos)[0]
        pos += 4
        d = dict(bytes=np.frombuffer(raw, np.uint8, size, pos).copy())
        pos += size
        d["probs"] = np.frombuffer(raw, np.uint8, 1728, pos).copy()
        pos += 1728
        d["exits"] = np.frombuffer(raw, np.int32, 4, pos).copy()
        d["updates"] = np.frombuffer(raw, np.int32, 4, pos + 16).copy()
        d["savings"] = np.frombuffer(raw, np.int64, 4, pos + 32).copy()
        pos += 64
        out.append(d)
    tabs = dict(prob_cost=np.frombuffer(raw, np.uint16, 256, pos).copy(), remap=np.frombuffer(raw, np.uint8, 255 * 255, pos + 512).copy(),
                update_bits=np.frombuffer(raw, np.uint8, 255 * 255, pos + 512 + 255 * 255).copy())
    pos += 512 + 2 * 255 * 255
    cov = struct.unpack_from("<I", raw, pos)[0]
    assert pos + 4 == len(raw)
    return out, tabs, {n for b, n in enumerate(COV) if (cov >> b) & 1}


def cases():
    """[(name, frame, tokens, old probabilities or None)]"""
    cat = np.concatenate
    out = [("zero_counts", KEY, np.zeros(0, np.uint32), None)]
    for n in (20, 21):      # that many blocks at 4x4 beside a well-filled 8x8
        out.append((f"tx_totals_{n}", INTER, cat([CM.seeded_stream(10 + n, blocks=n, groups=(0, 1, 2, 3), mix="zeros"), CM.seeded_stream(40, 6000, groups=(4, 5, 6, 7))]), None))
    for name, kind, pic, fp in CM.real_pictures():
        fr = KEY if kind == "key" else (1, fp["reference_mode"], fp["allow_comp_inter_inter"], fp["allow_hp"])
        out.append((f"real|{name}", fr, CM.host_stream(kind, pic)["tokens"], None))
    for k, mix in enumerate(("default", "zeros", "large", "ones")):
        out.append((f"seeded_{mix}", (KEY, INTER, INTER_SELECT_HP, INTER)[k], CM.seeded_stream(100 + k, 30000, mix=mix), None))
    out.append(("old_at_the_ends", INTER, CM.seeded_stream(120, 30000), CM.seeded_probs(121, ends=True)))
    out.append(("old_random", KEY, CM.seeded_stream(122, 12000, mix="large"), CM.seeded_probs(123)))
    # 16x16: a few dozen blocks whose statistics move a few entries, for less than the 396 flags cost; 32x32: 21 blocks of one EOB each,
    # no entry worth a search; 4x4 and 8x8 sent beside them
    out.append(("negative_and_none", INTER, cat([CM.seeded_stream(130, 9000, groups=(0, 1, 2, 3, 4, 5, 6, 7)), CM.seeded_stream(131, blocks=40, groups=(8, 9), mix="ones", max_len=4),
                                                 CM.seeded_stream(132, blocks=21, groups=(12,), mix="default", max_len=1)]), None))
    return out


def main():
    cs = cases()
    names = [c[0] for c in cs]
    assert len(set(names)) == len(names)
    default = BM.tables()[0]["coef_probs"].reshape(-1)
    req = []
    for name, fr, tok, old in cs:
        counts, eob = CM.counts_of(tok), CM.eob_branch(tok)
        tot = [int(sum(eob[144 * t + ij * 36 + l] for ij in range(4) for l in range(6))) for t in range(4)]
        req.append((fr, tot, counts, eob, default if old is None else old))
    with tempfile.TemporaryDirectory() as td:
        exe = build_driver(td)
        _, tabs, _ = run_reference(exe, td, [])
        got, tabs2, cov = run_reference(exe, td, req)
    assert all(np.array_equal(tabs[k], tabs2[k]) for k in tabs)
    missing = set(COV) - cov
    assert not missing, f"the reference did not reach: {sorted(missing)}"
    out = {"names": np.array(names), "coverage": np.array(sorted(cov)), **tabs}
    for (name, fr, tok, old), (_, tot, counts, eob, oldp), g in zip(cs, req, got):
        m = CM.decide(counts, eob, oldp, cost=tabs["prob_cost"])
        assert m["peak"] < 2 ** 31, (name, m["peak"])          # the reference's sums did not wrap
        out[f"tokens|{name}"] = tok
        out[f"frame|{name}"] = np.array(fr, np.int32)
        if old is not None:
            out[f"old|{name}"] = old
        for k in ("bytes", "probs", "exits", "updates", "savings"):
            out[f"{k}|{name}"] = g[k]
        print(f"{name}: {len(tok)} tokens, tx_totals {tot}, exits {list(g['exits'])}, updates {list(g['updates'])}, header {len(g['bytes'])} bytes, peak {m['peak']}")
    np.savez_compressed(CM.GOLD, **out)          # (the chain below reads the cost table from the fixture)
    for name, kind, pic, fp in CM.real_pictures():
        a, b = CM.host_frame(kind, pic, fp, update=True), CM.host_frame(kind, pic, fp, update=False)
        out[f"frame_with|{name}"], out[f"frame_without|{name}"] = np.frombuffer(a["frame"], np.uint8), np.frombuffer(b["frame"], np.uint8)
        print(f"{name}: frame {len(b['frame'])} bytes without updates, {len(a['frame'])} with (header {len(b['header'])} -> {len(a['header'])}, tile {len(b['tile'])} -> {len(a['tile'])})")
    print("reference reached:", sorted(cov))
    np.savez_compressed(CM.GOLD, **out)
    print(CM.GOLD, os.path.getsize(CM.GOLD), "bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/tq_edges_reference.npz: what the reference's own forward transforms and quantiser (eb_vp9_residual_kernel ->
eb_vp9_fht*_c / eb_vp9_fdct4x4_c / eb_vp9_fdct32x32_c / eb_vpx_partial_fdct32x32_c -> eb_vp9_quantize_b[_32x32]_c) give for the blocks of
tests/tq_edges_model.py: edge_cases().  Needs oracle/_ref/ref_fwdtq and oracle/_ref/ref_fwdtq_ubsan (`make -C oracle ref`, where the
reference's sources are); the tests that read the fixture need neither.

    python tests/gen_golden_tq_edges.py            write the fixture
    python tests/gen_golden_tq_edges.py --check    recompute and compare with the committed file

Every run: (1) all cases through ref_fwdtq_ubsan, the reference compiled with -fsanitize=signed-integer-overflow,shift
-fno-sanitize-recover=all, per (size, type), printed as the table of DESIGN.md section 5.18 -- every group must exit clean: the proof that
the list lies where the reference's C is defined; (2) the plain build's outputs, which the oracle must already equal.  The fixture holds the
outputs and the case names only: the inputs come from the seeds."""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svt_testlib as T  # noqa: E402
import tq_edges_model as E  # noqa: E402

PLAIN, UBSAN = os.path.join(T.REF_DIR, "ref_fwdtq"), os.path.join(T.REF_DIR, "ref_fwdtq_ubsan")
OUT = os.path.join(T.GOLDEN_DIR, "tq_edges_reference.npz")
KEYS = ("coeff", "qcoeff", "dqcoeff", "eob")


def request(cases):
    body = np.int32(len(cases)).tobytes()
    for c in cases:
        qt = np.concatenate([np.asarray(c["qt"][k], np.int16) for k in ("zbin", "round", "quant", "quant_shift", "dequant")])
        body += np.array([c["tx_size"], c["tx_type"], c["partial32"]], np.int32).tobytes() + qt.tobytes() + c["src"].tobytes() + c["pred"].tobytes()
    return body


def run(exe, cases):
    """-> (exit status, [(coeff, qcoeff, dqcoeff, eob)], stderr)"""
    with tempfile.TemporaryDirectory() as d:
        req, rsp = os.path.join(d, "req"), os.path.join(d, "rsp")
        with open(req, "wb") as f:
            f.write(request(cases))
        p = subprocess.run([exe, req, rsp], stderr=subprocess.PIPE)
        with open(rsp, "rb") as f:
            raw = f.read()
    out, pos = [], 0
    for c in cases:
        nn = T.TX_N[c["tx_size"]] ** 2
        if pos + 6 * nn + 4 > len(raw):
            break
        a = np.frombuffer(raw, np.int16, 3 * nn, pos).reshape(3, nn)
        out.append((a[0].copy(), a[1].copy(), a[2].copy(), int(np.frombuffer(raw, np.int32, 1, pos + 6 * nn)[0])))
        pos += 6 * nn + 4
    return p.returncode, out, p.stderr.decode(errors="replace")


def reference_outputs(cases, exe=PLAIN):
    rc, out, err = run(exe, cases)
    assert rc == 0 and len(out) == len(cases), (exe, rc, err[-400:])
    return out


def domain_table(cases):
    """the sanitized reference per (size, type): 'clean' or where it stopped"""
    rows, clean = [], True
    for ts, tt in E.GROUPS:
        n = T.TX_N[ts]
        for part in ((0, 1) if ts == 3 else (0,)):
            grp = [c for c in cases if (c["tx_size"], c["tx_type"], c["partial32"]) == (ts, tt, part)]
            rc, out, err = run(UBSAN, grp)
            where = sorted({ln.split(": runtime error")[0].split("/")[-1] for ln in err.splitlines() if "runtime error" in ln})
            assert (rc == 0) == (not where), (rc, err[-400:])
            peak = max(int(np.abs(o[0].astype(np.int32)).max()) for o in out) if out else 0
            rows.append((f"{E.TYPE_NAMES[tt]} {n}x{n}{' partial' if part else ''}", len(grp), peak, "clean" if rc == 0 else f"stopped after {len(out)} blocks (" + ", ".join(where) + ")"))
            clean &= rc == 0
    print("| block | cases | largest coefficient | ref_fwdtq_ubsan |")
    print("|---|---|---|---|")
    for r in rows:
        print("| " + " | ".join(str(x) for x in r) + " |")
    return clean


def pack(cases, outs):
    """the fixture's arrays: every output of every case, concatenated in list order"""
    return dict(names=np.array([c["name"] for c in cases]), coeff=np.concatenate([o[0] for o in outs]), qcoeff=np.concatenate([o[1] for o in outs]),
                dqcoeff=np.concatenate([o[2] for o in outs]), eob=np.array([o[3] for o in outs], np.uint16))


def generate(check):
    cases = E.edge_cases()
    print(f"{len(cases)} cases; {E.check_conditions()}")
    assert domain_table(cases), "the sanitized reference stopped: the list leaves the domain in which the reference's C is defined"
    print("ref_fwdtq_ubsan: clean on every case")
    ref = reference_outputs(cases)
    for c, r, o in zip(cases, ref, E.oracle_outputs()):
        for k, a, b in zip(KEYS, r, o):
            assert np.array_equal(a, b), ("the oracle differs from the reference", c["name"], k)
    print("oracle_fwd_txfm + oracle_quantize equal the reference on every case")
    want = pack(cases, ref)
    if check:
        g = np.load(OUT)
        same = all(np.array_equal(g[k], want[k]) for k in want)
        print(f"{OUT}: {'reproduced' if same else 'DIFFERS'}")
        return 0 if same else 1
    np.savez_compressed(OUT, **want)
    print(f"{OUT}: {len(cases)} cases, {want['coeff'].size} coefficients, {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 512 * 1024
    return 0


if __name__ == "__main__":
    if not os.path.exists(PLAIN) or not os.path.exists(UBSAN):
        sys.exit("oracle/_ref/ref_fwdtq and ref_fwdtq_ubsan are needed: make -C oracle ref")
    sys.exit(generate("--check" in sys.argv[1:]))

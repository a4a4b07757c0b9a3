"""Writes tests/golden/recon_edges_reference.npz: what the reference's own inverse transforms (its *_add_c kernels behind the eob dispatch of
VPX/vp9_idct.c) reconstruct from the coefficients of tests/decode_model.py: coeff_edge_cases().  Needs oracle/_ref/ref_invtx and
oracle/_ref/ref_invtx_ubsan (`make -C oracle ref`, where the reference's sources are); the tests that read the fixture need neither.

    python tests/gen_golden_recon_edges.py            write the fixture
    python tests/gen_golden_recon_edges.py --check    recompute and compare with the committed file
    python tests/gen_golden_recon_edges.py --probe    only the domain table

Every run: (1) all cases through ref_invtx_ubsan, the reference compiled with -fsanitize=signed-integer-overflow,shift
-fno-sanitize-recover=all, which must exit clean -- the proof that decode_model.OUTSIDE_DOMAIN_ABOVE drops enough; (2) the three-shape probe
(dense +-A, uniform in [-A, A], one coefficient in eight at +-A; PROBE_BLOCKS random full blocks each) through the same program per (size,
type, amplitude), printed as the table of DESIGN.md section 5.17; (3) the plain build's bytes, which oracle_inv_add must already equal.
The fixture holds the outputs and the case names only: the inputs come from the seeds."""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_model as D  # noqa: E402
import svt_testlib as T  # noqa: E402

PLAIN, UBSAN = os.path.join(T.REF_DIR, "ref_invtx"), os.path.join(T.REF_DIR, "ref_invtx_ubsan")
OUT = os.path.join(T.GOLDEN_DIR, "recon_edges_reference.npz")
PROBE_BLOCKS = 3000
TYPE_NAMES = ("DCT_DCT", "ADST_DCT", "DCT_ADST", "ADST_ADST")


def request(ts, tt, eob, pred, dq):
    """blocks of one size as the driver reads them: pred [k, nn] bytes, dq [k, nn] int16, eob scalar or [k]"""
    nn = pred.shape[1]
    rec = np.zeros(pred.shape[0], dtype=np.dtype([("head", "<i4", (3,)), ("pred", "u1", (nn,)), ("dq", "<i2", (nn,))]))
    rec["head"][:, 0], rec["head"][:, 1], rec["head"][:, 2] = ts, tt, eob
    rec["pred"], rec["dq"] = pred, dq
    return rec.tobytes()


def run(exe, count, body):
    """-> (exit status, output bytes, stderr)"""
    with tempfile.TemporaryDirectory() as d:
        req, rsp = os.path.join(d, "req"), os.path.join(d, "rsp")
        with open(req, "wb") as f:
            f.write(np.int32(count).tobytes() + body)
        p = subprocess.run([exe, req, rsp], stderr=subprocess.PIPE)
        with open(rsp, "rb") as f:
            return p.returncode, f.read(), p.stderr.decode(errors="replace")


def case_requests(cases):
    body = b""
    for c in cases:
        dq, _ = D.case_dqcoeff(c)
        body += request(c["tx_size"], c["tx_type"], c["eob"], c["pred"].reshape(1, -1), dq.reshape(1, -1))
    return body


def reference_bytes(cases, exe=PLAIN):
    rc, out, err = run(exe, len(cases), case_requests(cases))
    assert rc == 0, (exe, rc, err[-400:])
    assert len(out) == sum(c["qcoeff"].size for c in cases)
    return np.frombuffer(out, np.uint8).copy()


def probe():
    """the sanitized reference on random full blocks per (size, type, amplitude): 'clean' or where it stopped"""
    rng = np.random.default_rng(31)
    rows = []
    for ts, tt in D.GROUPS:
        n = T.TX_N[ts]
        nn, k, cells = n * n, PROBE_BLOCKS, []
        for a in D.LADDER:
            sign = lambda: rng.choice((-1, 1), (k, nn))                     # noqa: E731
            lvl = lambda s: np.where(s < 0, -32768, 32767) if a == 32767 else s * a      # noqa: E731
            dq = np.concatenate([lvl(sign()), rng.integers(-a, a + 1, (k, nn)), np.where(rng.random((k, nn)) < 0.125, lvl(sign()), 0)])
            pred = rng.integers(0, 256, (3 * k, nn)).astype(np.uint8)
            rc, _, err = run(UBSAN, 3 * k, request(ts, tt, nn, pred, dq.astype(np.int16)))
            where = sorted({ln.split(": runtime error")[0].split("/")[-1] for ln in err.splitlines() if "runtime error" in ln})
            cells.append("clean" if rc == 0 else "int32 overflow (" + ", ".join(where) + ")")
            assert (rc == 0) == (not where), (rc, err[-400:])
        rows.append((f"{TYPE_NAMES[tt]} {n}x{n}", cells))
    print("| block | " + " | ".join(f"A = {a}" for a in D.LADDER) + " |")
    print("|---|" + "---|" * len(D.LADDER))
    for name, cells in rows:
        print(f"| {name} | " + " | ".join(cells) + " |")
    return rows


def generate(check):
    cases = D.coeff_edge_cases()
    print(f"{len(cases)} cases")
    reference_bytes(cases, UBSAN)                                            # (asserts a clean exit)
    print("ref_invtx_ubsan: clean on every case")
    ref = reference_bytes(cases)
    pos = 0
    for c in cases:
        dq, _ = D.case_dqcoeff(c)
        n = T.TX_N[c["tx_size"]]
        got = c["pred"] if c["eob"] == 0 else T.oracle_inv_add(dq, c["pred"], c["tx_size"], c["tx_type"], c["eob"])
        assert np.array_equal(got.ravel(), ref[pos:pos + n * n]), ("oracle_inv_add differs from the reference", c["name"])
        pos += n * n
    print("oracle_inv_add equals the reference on every case")
    names = np.array([c["name"] for c in cases])
    if check:
        g = np.load(OUT)
        same = np.array_equal(g["names"], names) and np.array_equal(g["recon"], ref)
        print(f"{OUT}: {'reproduced' if same else 'DIFFERS'}")
        return 0 if same else 1
    np.savez_compressed(OUT, names=names, recon=ref)
    print(f"{OUT}: {len(names)} cases, {ref.size} bytes of reconstruction, {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 512 * 1024
    return 0


if __name__ == "__main__":
    if not os.path.exists(PLAIN) or not os.path.exists(UBSAN):
        sys.exit("oracle/_ref/ref_invtx and ref_invtx_ubsan are needed: make -C oracle ref")
    args = sys.argv[1:]
    rc = 0 if "--probe" in args else generate("--check" in args)
    if "--no-probe" not in args:
        probe()
    sys.exit(rc)

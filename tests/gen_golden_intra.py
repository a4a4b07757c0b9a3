"""Writes tests/golden/intra_reference.npz: what the REFERENCE's own functions (oracle/_ref/ref_intra: generate_intra_reference_samples +
intra_prediction + perform_coding_loop + the neighbour-array writer, block by block in the reference's coding order) make of every case of
tests/encdec_model.py's INTRA_GOLDEN_CASES -- per case the prediction, the reconstruction before deblocking, qcoeff, dqcoeff and the eob
map, beside the source planes and the mode-info grid the reference was given.  Only inputs and recorded results are stored.

The generator fails unless the recording reaches what it is there for (tests/test_intra_oracle.py asserts the same of the committed file):
every block size, coefficients of a thousand and more and a full 32x32 block at q 0, small but non-zero coefficients at q 255, TM blocks
that clamp on both sides.  The file is written with fixed time stamps: the same inputs give the same bytes.

    python tests/gen_golden_intra.py            (needs oracle/_ref/ref_intra)
"""
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encdec_model as M           # noqa: E402
import svt_testlib as T            # noqa: E402

LIMIT = 400 * 1000


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def main():
    assert T.have_ref("ref_intra"), "build the reference harness first (make -C oracle ref)"
    names = [c[0] for c in M.INTRA_GOLDEN_CASES]
    assert len(set(names)) == len(names)
    out, gold = {"names": np.array(names)}, {}
    for case in M.INTRA_GOLDEN_CASES:
        src, mi = M.intra_golden_inputs(case)
        g = M.intra_flat(M.ref_intra_picture(src, mi, case[4]))
        g["src"] = np.concatenate([p.ravel() for p in src])
        g["mi"] = np.frombuffer(np.ascontiguousarray(mi).tobytes(), np.uint8)
        gold[case[0]] = g
        for k, a in g.items():
            out[f"{k}|{case[0]}"] = a
    print(M.intra_golden_reach(M.INTRA_GOLDEN_CASES, gold, print))
    write_npz(M.INTRA_GOLDEN, out)
    size = os.path.getsize(M.INTRA_GOLDEN)
    print(M.INTRA_GOLDEN, size, "bytes")
    assert size < LIMIT, size


if __name__ == "__main__":
    main()

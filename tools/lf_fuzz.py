"""Randomised parity sweep of the deblocking kernel against the oracle (GPU): random sizes (multiples of 8, partial SBs), mask /
level / content seeds, sharpness 0..7, blocky / smooth / random-walk content, a random padded stride per plane.
tools/lf_fuzz.py [cases] [seed]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import svt_testlib as T
B = T.B; lib = B.load()
ctx = C.c_void_p(); B.check(lib.svt_hip_ctx_create(C.byref(ctx), 0))
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
rng2 = np.random.default_rng([int(sys.argv[2]) if len(sys.argv) > 2 else 1, 1])   # strides and generator choice: the sizes and seeds above keep their stream


def padded(plane, stride):
    """the plane inside rows of `stride` bytes; the padding holds 0xA5"""
    buf = np.full((plane.shape[0], stride), 0xA5, np.uint8)
    buf[:, :plane.shape[1]] = plane
    return buf


bad = 0
for i in range(n_cases):
    w, h = 8 * int(rng.integers(8, 60)), 8 * int(rng.integers(8, 40))
    seed, sharp = int(rng.integers(1 << 20)), int(rng.integers(0, 8))
    case = T.make_lf_case(seed, w, h, sharp)
    kind = "blocky"
    if rng.integers(0, 3) == 0:   # smooth content: the 8- and 16-wide (flat) filters take part
        kind = "ramp"
        ramp = (np.add.outer(np.arange(h), np.arange(w)) // 6 % 200 + 20).astype(np.uint8)
        case["y"][:] = ramp + rng.integers(0, 2, ramp.shape, dtype=np.uint8)
        case["u"][:] = ramp[::2, ::2]; case["v"][:] = 255 - ramp[::2, ::2]
    if rng2.integers(0, 3) == 0:  # random walks: the 15-tap filter, filter4's clamps, mostly level 63 (svt_testlib.make_lf_extremes_case)
        kind = "extremes"
        case = T.make_lf_extremes_case(seed, w, h, sharp, int(rng2.integers(0, 2)))
    o = T.oracle_lf_frame(case)
    # planes in rows longer than the picture (any multiple of 4; 8-byte and 4-byte copy units both come up)
    ys, cs = w + 4 * int(rng2.integers(0, 17)), w // 2 + 4 * int(rng2.integers(0, 17))
    g = [padded(case["y"], ys), padded(case["u"], cs), padded(case["v"], cs)]
    d = T._yuv_desc(g[0][:, :w], g[1][:, :w // 2], g[2][:, :w // 2])
    lfm = np.ascontiguousarray(case["lfm"])
    B.check(lib.svt_hip_lf_frame(ctx, C.byref(d), lfm.ctypes.data_as(C.c_void_p), lfm.shape[1], C.byref(case["thr"]), case["mi_rows"], case["mi_cols"], 0))
    ok = True
    for n, a, b in zip("yuv", o, g):
        inner, pad = b[:, :a.shape[1]], b[:, a.shape[1]:]
        if not np.array_equal(a, inner):
            ok = False
            print("MISMATCH case", i, (w, h), kind, "sharpness", sharp, "strides", (ys, cs), "plane", n, int(np.sum(a != inner)), "samples, first at",
                  np.argwhere(a != inner)[:6].tolist())
        if not np.all(pad == 0xA5):
            ok = False
            print("PADDING CHANGED case", i, (w, h), kind, "strides", (ys, cs), "plane", n, "first at", (np.argwhere(pad != 0xA5)[:6] + [0, a.shape[1]]).tolist())
    bad += not ok
print("cases", n_cases, "mismatches", bad)
sys.exit(1 if bad else 0)

"""CPU: the MV-reference stage's kernels themselves (csrc/mvrefs.hip compiled as plain C++ against tests/emu/hip/hip_runtime.h,
one thread per lane) against svt_hip_mvrefs_picture: every fixture picture singly, batches of one geometry whose pictures differ in
restrict flag, sign biases and ref_mask, optional outputs left out, the malformed grids, wider grids and a 1080x1080 picture of 289 SBs
-- the window staging, the walk from the window, the record stores and the two-pass status as the device runs them, without a device;
and the 72x40 and 136x136 pictures with the outputs 2 bytes off a 16-byte boundary, each optional output present and absent: the 16-bit
stores.
The stand-alone program is built with AddressSanitizer and UBSan where the compiler has their runtimes."""
import os
import struct
import subprocess
import tempfile

import numpy as np

import mvrefs_model as M
import svt_testlib as T
from test_mvrefs import MALFORMED

B = T.B


def build(td):
    emu, src = os.path.join(T.ROOT, "tests", "emu", "mvrefs"), os.path.join(T.ROOT, "svt-vp9_amd")
    exe = os.path.join(td, "mvrefs_emu")
    cmd = ["g++", "-x", "c++", "-std=c++17", "-O1", "-w", f"-I{os.path.dirname(emu)}", f"-I{os.path.join(src, 'csrc')}", os.path.join(emu, "mvrefs_emu.cpp"),
           "-x", "c", os.path.join(src, "host", "mvrefs_host.c"), "-lpthread", "-o", exe]
    sanitized = subprocess.run(cmd[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] + cmd[1:], capture_output=True).returncode == 0
    if not sanitized:
        subprocess.check_call(cmd)
    return exe, sanitized


def test_kernel_text_on_the_cpu_equals_the_host_form():
    groups = []                 # ((W, H, extra stride, byte offset of the outputs), [(picture, ref_mask, restrict, bias, want_ext, want_cand)])

    def case(p, ref_mask=M.ALL_REFS, restrict=None, bias=None, want_ext=1, want_cand=1):
        return p, ref_mask, p["restrict"] if restrict is None else restrict, p["frame"]["sign_bias"] if bias is None else bias, want_ext, want_cand
    by_size = {}
    for name in M.names():
        p = M.fixture_picture(name)
        by_size.setdefault((p["W"], p["H"]), []).append(case(p))
    for size, cases in by_size.items():                  # every fixture picture; the pictures of one size differ in flag and biases
        groups.append(((*size, 0, 0), cases))
    mix = M.fixture_picture("mix_136x136_b")
    groups.append(((136, 136, 0, 0), [case(mix, 0), case(mix, 2, restrict=1), case(mix, 12, bias=M.ZERO_BIAS), case(mix, want_ext=0), case(mix, want_cand=0),
                                   case(mix, 6, want_ext=0, want_cand=0), case(M.fixture_picture("pert_136x136"), 8)]))
    n_bad = 0
    for size in ((136, 136), (72, 40)):
        bad = [case(p) for _, p, _ in MALFORMED if (p["W"], p["H"]) == size]
        n_bad += sum(1 for _, p, good in MALFORMED if (p["W"], p["H"]) == size and not good)
        for k in range(0, len(bad), 24):                 # (a call takes 32 pictures at most) each batch beside a well-formed fixture picture
            groups.append(((*size, 0, 0), bad[k:k + 24] + [case(M.fixture_picture("mix_136x136_a" if size[0] == 136 else "edge_72x40_a"))]))
    for name in ("edge_72x40_b", "mix_136x136_d", "ceil_8192x64"):      # mi_stride = mi_cols + 9, random bytes behind every row
        p = M.fixture_picture(name)
        groups.append(((p["W"], p["H"], 9, 0), [case(M.with_stride(p, 9, 3))]))
    big = M.big_picture()                                # 289 SBs: two entries per thread of the status kernel and threads with none
    groups.append(((1080, 1080, 0, 0), [case(big), case(big, 2, restrict=1)]))
    for name in ("edge_72x40_b", "mix_136x136_d"):       # the records' own alignment only: the stores in halves, chosen per output
        p = M.fixture_picture(name)
        groups.append(((p["W"], p["H"], 0, 2), [case(p), case(p, want_ext=0), case(p, want_cand=0), case(p, want_ext=0, want_cand=0)]))
    n_pics = sum(len(g[1]) for g in groups)
    with tempfile.TemporaryDirectory() as td:
        exe, sanitized = build(td)
        req = os.path.join(td, "req.bin")
        with open(req, "wb") as f:
            f.write(struct.pack("<i", len(groups)))
            for (W, H, extra, offset), pics in groups:
                f.write(struct.pack("<5i", W, H, W // 8 + extra, len(pics), offset))
                for p, ref_mask, restrict, bias, want_ext, want_cand in pics:
                    assert p["lf_mi"].shape == p["mc_mi"].shape == p["ext"].shape == (H // 8, W // 8 + extra)
                    f.write(bytes([ref_mask, restrict, *bias, want_ext, want_cand]))
                    for k in ("lf_mi", "mc_mi", "ext"):
                        f.write(np.ascontiguousarray(p[k]).tobytes())
        r = subprocess.run([exe, req], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "bad 0" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
        assert r.stdout.count(" ok") == n_pics
        assert r.stdout.count(f"status {0xFFFFFFFF}/{0xFFFFFFFF} {0xFFFFFFFF}/{0xFFFFFFFF}") == n_bad
        print("sanitizers:", sanitized)

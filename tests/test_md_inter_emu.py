"""CPU: the kernels of inter mode labelling themselves (csrc/md_inter.hip compiled as plain C++ against tests/emu/hip/hip_runtime.h, one
thread per lane) against svt_hip_md_inter_modes_picture: the seeded and the constructed pictures, batches of one geometry whose
pictures differ in every parameter, d_cand left out, the malformed grids, wider grids and a picture of 289 SBs -- the two window
stagings, the label pass into the scratch grid, the derivation over it, the record stores and the status pass as the device runs them,
without a device; and one picture with the outputs 2 bytes off a 16-byte boundary, with and without d_cand: the 16-bit stores.  Built twice: plain, and as the same stand-alone program under AddressSanitizer and UBSan with the grids allocated to
exactly their size."""
import os
import struct
import subprocess
import tempfile

import numpy as np

import md_inter_model as D
import mvrefs_model as M
import svt_testlib as T
from test_md_inter import MALFORMED, SEEDED, constructed, seeded

B = T.B
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]


def build(td, flags, name):
    emu, src = os.path.join(T.ROOT, "tests", "emu", "md_inter"), os.path.join(T.ROOT, "svt-vp9_amd")
    exe = os.path.join(td, name)
    cmd = ["g++"] + flags + ["-x", "c++", "-std=c++17", "-O1", "-w", f"-I{os.path.dirname(emu)}", f"-I{os.path.join(src, 'csrc')}",
                             os.path.join(emu, "md_inter_emu.cpp"), "-x", "c", os.path.join(src, "host", "md_inter_host.c"), "-lpthread", "-o", exe]
    return exe if subprocess.run(cmd, capture_output=True).returncode == 0 else None


def params(p, ref_mask=M.ALL_REFS, want_cand=1, **over):
    fr = p["frame"]
    v = dict(list_ref_frame=p["lrf"], ref_frame_sign_bias=fr["sign_bias"], restrict_ref_mvs=p["restrict"], allow_hp=fr["allow_hp"],
             reference_mode=fr["reference_mode"], comp_fixed_ref=fr["comp_fixed_ref"], comp_var_ref=fr["comp_var_ref"])
    v.update(over)
    return bytes([*v["list_ref_frame"], *v["ref_frame_sign_bias"], v["restrict_ref_mvs"], v["allow_hp"], v["reference_mode"], v["comp_fixed_ref"],
                  *v["comp_var_ref"], ref_mask, want_cand, 0, 0])


def test_kernel_text_on_the_cpu_equals_the_host_form():
    groups = []                 # ((W, H, extra stride, byte offset of the outputs), [(picture, its 16 parameter bytes)])
    by_size = {}
    for name, _ in SEEDED:
        p = seeded(name)
        by_size.setdefault((p["W"], p["H"]), []).append((p, params(p)))
    for size, cases in by_size.items():                  # the pictures of one size differ in frame, restrict flag and lists
        groups.append(((*size, 0, 0), cases))
    groups.append(((64, 64, 0, 0), [(p, params(p)) for _, p, _, _ in constructed()]))
    mix = seeded("mix_136x72")
    groups.append(((136, 72, 0, 0), [(mix, params(mix, 0)), (mix, params(mix, 2, restrict_ref_mvs=1)), (mix, params(mix, 12, allow_hp=1)), (mix, params(mix, want_cand=0)),
                                  (mix, params(mix, 6, want_cand=0, ref_frame_sign_bias=(0, 1, 0, 1)))]))
    n_bad = 0
    for size in ((136, 72), (72, 40)):
        bad = [(p, params(p, **over)) for _, p, over in MALFORMED if (p["W"], p["H"]) == size]
        n_bad += len(bad)
        for k in range(0, len(bad), 24):                 # (a call takes 32 pictures at most) each batch beside a well-formed picture
            good = seeded("mix_136x72" if size[0] == 136 else "edge_72x40")
            groups.append(((*size, 0, 0), bad[k:k + 24] + [(good, params(good))]))
    for name in ("edge_72x40", "mix_136x72"):            # mi_stride = mi_cols + 7, random bytes behind every row
        p = seeded(name)
        groups.append(((p["W"], p["H"], 7, 0), [(D.with_stride(p, 7, 3), params(p))]))
    big = D.big_picture()                                # 289 SBs: the status pass's threads with two entries and with none
    groups.append(((1080, 1080, 0, 0), [(big, params(big)), (big, params(big, 2, restrict_ref_mvs=1, allow_hp=1))]))
    groups.append(((136, 72, 0, 2), [(mix, params(mix)), (mix, params(mix, want_cand=0))]))      # the records' own alignment only: the stores in halves
    n_pics = sum(len(g[1]) for g in groups)
    with tempfile.TemporaryDirectory() as td:
        plain, sanitized = build(td, [], "md_inter_emu"), build(td, SANITIZE, "md_inter_emu_san")
        assert plain
        req = os.path.join(td, "req.bin")
        with open(req, "wb") as f:
            f.write(struct.pack("<i", len(groups)))
            for (W, H, extra, offset), pics in groups:
                f.write(struct.pack("<5i", W, H, W // 8 + extra, len(pics), offset))
                for p, par in pics:
                    assert p["lf_mi"].shape == p["mc_mi"].shape == (H // 8, W // 8 + extra) and len(par) == 16
                    f.write(par)
                    for k in ("lf_mi", "mc_mi"):
                        f.write(np.ascontiguousarray(p[k]).tobytes())
        for exe in (plain, sanitized):
            if exe is None:
                continue
            r = subprocess.run([exe, req], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "bad 0" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
            assert r.stdout.count(" ok") == n_pics
            bad4 = " ".join([f"{0xFFFFFFFF}/{0xFFFFFFFF}"] * 4)
            assert r.stdout.count(f"status {bad4}") == n_bad
        print("sanitizers:", sanitized is not None)

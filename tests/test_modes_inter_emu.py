"""CPU: the inter mode-info stage's kernels themselves (csrc/modeinfo_inter.hip compiled as plain C++ against
tests/emu/hip/hip_runtime.h, one thread per lane) against svt_hip_modes_inter_picture on the fixture pictures, singly and
as batches of one geometry whose pictures differ in frame parameters, with full, short and no bool capacity, on the malformed grids, on
the unit with the most bools, on wider grids and on 1080x1080 pictures of 289 SBs -- the count, the scan, the LDS assembly, the dword
stores and the segment slots as the device runs them, without a device."""
import os
import struct
import subprocess
import tempfile

import numpy as np

import modes_inter_model as IM
import svt_testlib as T
from test_modes_inter import MALFORMED, worst_unit_picture

B = T.B


def frame_bytes(fr):
    return bytes([fr["reference_mode"], fr["allow_hp"], fr["comp_fixed_ref"], *fr["comp_var_ref"], *fr["sign_bias"]])


def test_kernel_text_on_the_cpu_equals_the_host_form():
    lib = B.load()
    groups = []                 # ((W, H, extra stride), [(capacity, picture, tok_off, frame)])

    def fixture_case(name, capacity=None):
        p = IM.fixture_picture(name)
        cap = int(lib.svt_hip_modes_inter_bools_capacity(p["W"], p["H"])) if capacity is None else capacity
        return cap, p, IM.host_tokens(name)["tok_off"], p["frame"]
    for size in ((64, 64), (72, 40), (136, 136)):       # every fixture picture; single and SELECT pictures in one call
        groups.append(((*size, 0), [fixture_case(n) for n, W, H, *_ in IM.PICTURES if (W, H) == size]))
    total = IM.host_of("mix_136x136_select")["n_bools"]
    groups.append(((136, 136, 0), [fixture_case("mix_136x136_select", c) for c in (total, total - 1, 0, total // 2)]))
    groups.append(((72, 40, 0), [fixture_case("edge_72x40_b", 3)]))
    for size in ((64, 64), (72, 40)):
        pics = []
        for what, p, fr, good in MALFORMED:
            if (p["W"], p["H"]) == size:
                p = dict(p, lf_mi=p["lf_mi"].copy(), eob_map=np.zeros_like(p["eob_map"]))
                p["lf_mi"]["skip"] = 1
                pics.append((int(lib.svt_hip_modes_inter_bools_capacity(*size)), p, np.full(p["eob_map"].size, 0xFFFFFFFF, np.uint32), fr or p["frame"]))
        for k in range(0, len(pics), 24):                # (a call takes 32 pictures at most) each batch beside a well-formed fixture picture
            groups.append(((*size, 0), pics[k:k + 24] + [fixture_case("sb64_leaf3" if size[0] == 64 else "edge_72x40_a")]))
    worst = worst_unit_picture()
    groups.append(((64, 64, 0), [(int(lib.svt_hip_modes_inter_bools_capacity(64, 64)), worst, np.full(worst["eob_map"].size, 0xFFFFFFFF, np.uint32), worst["frame"]),
                                 fixture_case("sb64_leaf12")]))
    for name in ("edge_72x40_b", "mix_136x136_select"):  # mi_stride = mi_cols + 9, random bytes behind every row
        cap, p, tok_off, fr = fixture_case(name)
        groups.append(((p["W"], p["H"], 9), [(cap, IM.with_stride(p, 9, 3), tok_off, fr)]))
    # 289 SBs: two entries per lane of the SB scan and lanes with none, an odd SB count under the batch's % and /, a last workgroup of the
    # emit kernel with one live wave; with room for every bool and for half of them
    big = []
    for p in IM.big_pictures():
        h = IM.big_host(p["name"])
        big += [(cap, p, h["tok"]["tok_off"], p["frame"]) for cap in (int(lib.svt_hip_modes_inter_bools_capacity(p["W"], p["H"])), h["modes"]["n_bools"] // 2)]
    groups.append(((1080, 1080, 0), big))
    n_pics = sum(len(g[1]) for g in groups)
    n_bad = sum(1 for _, _, _, good in MALFORMED if not good)
    emu, src = os.path.join(T.ROOT, "tests", "emu", "modeinfo_inter"), os.path.join(T.ROOT, "svt-vp9_amd")
    with tempfile.TemporaryDirectory() as td:
        exe, req = os.path.join(td, "modeinfo_inter_emu"), os.path.join(td, "req.bin")
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-w", f"-I{os.path.dirname(emu)}", f"-I{os.path.join(src, 'csrc')}", os.path.join(emu, "modeinfo_inter_emu.cpp"),
                               "-x", "c", os.path.join(src, "host", "modeinfo_inter_host.c"), os.path.join(src, "host", "modeinfo_host.c"), "-lpthread", "-o", exe])
        with open(req, "wb") as f:
            f.write(IM.tables()[1].tobytes())
            f.write(struct.pack("<i", len(groups)))
            for (W, H, extra), pics in groups:
                f.write(struct.pack("<4i", W, H, W // 8 + extra, len(pics)))
                for cap, p, tok_off, fr in pics:
                    assert p["lf_mi"].shape == p["mc_mi"].shape == p["ext"].shape == (H // 8, W // 8 + extra)
                    f.write(struct.pack("<i", cap) + frame_bytes(fr))
                    for k in ("lf_mi", "mc_mi", "ext"):
                        f.write(np.ascontiguousarray(p[k]).tobytes())
                    f.write(np.ascontiguousarray(p["eob_map"], np.uint16).tobytes() + np.ascontiguousarray(tok_off, np.uint32).tobytes())
        r = subprocess.run([exe, req], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "bad 0" in r.stdout and "MISMATCH" not in r.stdout, r.stdout + r.stderr
        assert r.stdout.count(" ok") == n_pics
        assert r.stdout.count(f"bools {0xFFFFFFFF}/{0xFFFFFFFF}") == n_bad

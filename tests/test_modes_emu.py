"""CPU: the mode-info stage's kernels themselves (csrc/modeinfo.hip compiled as plain C++ against tests/emu/hip/hip_runtime.h,
one thread per lane) against svt_hip_modes_kf_picture on the fixture pictures, singly and as batches of one geometry, with full, short and
no bool capacity, on the malformed grids, on the unit with the most bools and on 1080x1080 pictures of 289 SBs -- the count, the scan, the LDS assembly, the dword stores and the segment slots as the
device runs them, without a device."""
import os
import struct
import subprocess
import tempfile

import numpy as np

import modes_model as MM
import svt_testlib as T
from test_modes import edge_crossing_grid, malformed_grids, worst_unit_grid

B = T.B


def test_kernel_text_on_the_cpu_equals_the_host_form():
    lib = B.load()
    groups = []

    def fixture_case(name, capacity=None):
        p, tok = MM.fixture_picture(name), MM.host_tokens(name)
        cap = int(lib.svt_hip_modes_bools_capacity(p["W"], p["H"])) if capacity is None else capacity
        return cap, p["lf_mi"], p["eob_map"], tok["tok_off"]
    for size in ((64, 64), (72, 40), (136, 136)):
        groups.append((size, [fixture_case(n) for n, W, H, _, _ in MM.PICTURES if (W, H) == size]))
    total = MM.host_modes(*fixture_case("sbs_136x136_b")[1:], 136, 136)["n_bools"]
    groups.append(((136, 136), [fixture_case("sbs_136x136_b", total - 1), fixture_case("sbs_136x136_b", 0), fixture_case("sbs_136x136_b", total // 2)]))
    groups.append(((72, 40), [fixture_case("edge_72x40_b", 3)]))
    for (W, H), grids in (((64, 64), [lf for _, lf in malformed_grids()]), ((72, 40), [edge_crossing_grid()])):
        emap = np.zeros(MM.eob_offsets(W, H)[3], np.uint16)
        good = "sb64_leaf3" if W == 64 else "edge_72x40_a"
        groups.append(((W, H), [(int(lib.svt_hip_modes_bools_capacity(W, H)), lf, emap, np.full(emap.size, 0xFFFFFFFF, np.uint32)) for lf in grids] + [fixture_case(good)]))
    # the unit that reaches SVT_MI_UNIT_BOOLS (every unit of the SB at its ceiling but for the partition symbols), beside a fixture picture
    worst = worst_unit_grid()
    worst["skip"] = 1
    emap = np.zeros(MM.eob_offsets(64, 64)[3], np.uint16)
    groups.append(((64, 64), [(int(lib.svt_hip_modes_bools_capacity(64, 64)), worst, emap, np.full(emap.size, 0xFFFFFFFF, np.uint32)), fixture_case("sb64_leaf0")]))
    # 289 SBs: two entries per lane of the SB scan and lanes with none, an odd SB count under the batch's % and /, a last workgroup of the
    # emit kernel with one live wave; with room for every bool and for half of them
    big = []
    for p in MM.big_pictures():
        h = MM.big_host(p["name"])
        big += [(cap, p["lf_mi"], p["eob_map"], h["tok"]["tok_off"]) for cap in (int(lib.svt_hip_modes_bools_capacity(p["W"], p["H"])), h["modes"]["n_bools"] // 2)]
    groups.append(((1080, 1080), big))
    n_pics = sum(len(g[1]) for g in groups)
    emu, src = os.path.join(T.ROOT, "tests", "emu", "modeinfo"), os.path.join(T.ROOT, "svt-vp9_amd")
    with tempfile.TemporaryDirectory() as td:
        exe, req = os.path.join(td, "modeinfo_emu"), os.path.join(td, "req.bin")
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-w", f"-I{os.path.dirname(emu)}", f"-I{os.path.join(src, 'csrc')}", os.path.join(emu, "modeinfo_emu.cpp"),
                               "-x", "c", os.path.join(src, "host", "modeinfo_host.c"), "-lpthread", "-o", exe])
        with open(req, "wb") as f:
            f.write(MM.tables()[1].tobytes())
            f.write(struct.pack("<i", len(groups)))
            for (W, H), pics in groups:
                f.write(struct.pack("<3i", W, H, len(pics)))
                for cap, lf, emap, tok_off in pics:
                    f.write(struct.pack("<i", cap))
                    f.write(np.ascontiguousarray(lf).tobytes() + np.ascontiguousarray(emap, np.uint16).tobytes() + np.ascontiguousarray(tok_off, np.uint32).tobytes())
        r = subprocess.run([exe, req], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "bad 0" in r.stdout and "MISMATCH" not in r.stdout, r.stdout + r.stderr
        assert r.stdout.count(" ok") == n_pics
        assert r.stdout.count(f"bools {0xFFFFFFFF}/{0xFFFFFFFF}") == len(malformed_grids()) + 1

"""CPU: the three-part assembly kernel itself (svt_fr_parts_kernel of csrc/frame.hip compiled as plain C++ against
tests/emu/hip/hip_runtime.h, one thread per lane) against svt_hip_frame_assemble_parts_host: compressed headers of 1, 15, 16, 17, 31, 33 and
300 bytes, tiles of 2, 16 and 4 097, all 16 source and all 16 destination phases of each part, every reason to withhold a picture, arenas
that end inside the header, inside the compressed part and inside the tile.  Built twice: plain, and as the same stand-alone program under
AddressSanitizer and UBSan with every source in an allocation of exactly the 16-byte blocks that hold its bytes."""
import os
import subprocess
import tempfile

import frame_parts_model as PM
import svt_testlib as T
from test_frame_read import sanitizer_runtime_present

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
EMU_WGS = 3                     # workgroups per picture in the emulation: a 4 097-byte tile is 256 vectors, one pass of 3 x 256 lanes with idle lanes


def build(td, flags, name):
    emu, src = os.path.join(T.ROOT, "tests", "emu"), os.path.join(T.ROOT, "svt-vp9_amd")
    exe = os.path.join(td, name)
    cmd = ["g++"] + flags + ["-x", "c++", "-std=c++17", "-O1", "-w", f"-DFR_WGS={EMU_WGS}", f"-I{emu}", f"-I{os.path.join(src, 'csrc')}",
                             os.path.join(emu, "frame", "frame_parts_emu.cpp"), "-x", "c", os.path.join(src, "host", "frame_host.c"),
                             os.path.join(src, "host", "boolcode_host.c"), "-lpthread", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the emulation does not compile with " + " ".join(flags) + "\n" + r.stderr[-3000:]
    return exe


def test_cases_cover_every_size_and_phase_of_each_part():
    cases = PM.emu_cases()
    pics = [p for b, _ in cases for p in b["pics"] if PM.has_packet(p)]
    assert {p["comp"] for p in pics} == set(PM.COMP_SIZES) and {p["tile"] for p in pics} == set(PM.TILE_SIZES)
    comp, tile = set(), set()
    for b, _ in cases:
        c, t = PM.phases(b, 0, 0)       # (the emulation keeps every source at its offset's phase and the arena on a 16-byte boundary)
        comp |= c
        tile |= t
    for part in (comp, tile):
        assert {s for s, _ in part} == set(range(16)) and {d for _, d in part} == set(range(16))
    assert {len(p["trailer"]) for p in pics} == {0, 1, 2, 3, 4} and {p["size_bit"] % 8 for p in pics} == set(range(8))


def test_kernel_text_on_the_cpu_equals_the_host_form():
    with tempfile.TemporaryDirectory() as td:
        # where the host compiler links no sanitizer runtime the program runs plain only; with one, a failure to compile under it is an error
        with_san = sanitizer_runtime_present(td)
        exes = [build(td, [], "frame_parts_emu")] + ([build(td, SANITIZE, "frame_parts_emu_san")] if with_san else [])
        req = os.path.join(td, "batches.bin")
        n = PM.emu_request(req, PM.emu_cases())
        for exe in exes:
            r = subprocess.run([exe, req], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "bad 0" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
            assert r.stdout.count(" ok") == n
        print("sanitizers:", with_san)

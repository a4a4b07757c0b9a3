"""CPU: the frame stage's host half against the reference's eb_vp9_pack_bitstream (tests/golden/frame_reference.npz) -- the two headers of
every case from svt_hip_frame_header_host and from the independent model tests/frame_model.py, the show-existing bytes, whole frames,
refusals, struct sizes, SVT_FRAME_HEADER_MAX over a seeded sweep; the packet layout (svt_hip_frame_assemble_host) against a numpy
concatenation with the overflow and short-arena rules; and the assembly kernel's own text on the CPU (csrc/frame.hip compiled as plain C++
against tests/emu/hip/hip_runtime.h, one thread per lane) against the host form, once more under AddressSanitizer and UBSan as a
stand-alone program where the host compiler links one."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import frame_model as FM
import svt_testlib as T

B = T.B
HEADER_NAMES = [n for n, _ in FM.CASES] + [n for n, *_ in FM.WHOLE]


@pytest.mark.parametrize("name", HEADER_NAMES)
def test_headers_equal_the_reference(name):
    p, frame, ub, cb = FM.fixture_case(name)
    assert p == dict(FM.CASES).get(name, {n: q for n, _, _, q in FM.WHOLE}.get(name)), "the fixture was made from other parameters"
    rc, buf, got_ub, got_cb = FM.host_headers(p)
    assert rc == 0 and (got_ub, got_cb) == (ub, cb)
    assert bytes(buf[:ub + cb]) == frame[:ub + cb] and np.all(buf[ub + cb:] == 0xA5)
    u, c = FM.headers(p)
    assert u + c == frame[:ub + cb] and len(c) == cb
    # first_part_size: the last 16 bits in front of the byte padding, in the reference's bytes
    n_bits = len(FM.uncompressed_bits(p, 0).bits)
    assert (n_bits + 7) // 8 == ub
    assert (int.from_bytes(frame[:ub], "big") >> (8 * ub - n_bits)) & 0xFFFF == cb


@pytest.mark.parametrize("slot", FM.SHOW_EXISTING_SLOTS)
def test_show_existing_bytes_equal_the_reference(slot):
    want = bytes(FM.fixture()[f"frame|show_existing_{slot}"])
    out = (C.c_uint8 * 2)(0xA5, 0xA5)
    assert B.load().svt_hip_frame_show_existing_host(slot, out) == 0
    assert bytes(out) == want + b"\xA5" and FM.show_existing(slot) == want


def test_show_existing_refusals():
    out = (C.c_uint8 * 1)(0xA5)
    for slot in (-1, 8):
        assert B.load().svt_hip_frame_show_existing_host(slot, out) == -1 and out[0] == 0xA5
    assert B.load().svt_hip_frame_show_existing_host(0, None) == -1


def test_fixture_reaches_every_branch_of_both_writers():
    """noted by the driver from the reference's own structures while it wrote the fixture; the generator refuses to write a fixture
    that lacks one"""
    import gen_golden_frame as G
    assert set(FM.fixture()["coverage"]) == set(G.UCOV) | {"c_" + n for n in G.CCOV}


@pytest.mark.parametrize("name", [n for n, *_ in FM.WHOLE])
def test_whole_frames_equal_the_reference(name):
    """header || the fixture's recorded tile || nothing, laid out by the host form of the assembly: eb_vp9_pack_bitstream's frame"""
    _, kind, pic, p = next(w for w in FM.WHOLE if w[0] == name)
    frame = bytes(FM.fixture()[f"frame|{name}"])
    tile = np.frombuffer(FM.whole_tile(kind, pic), np.uint8)
    head = FM.host_header_bytes(p)
    batch = dict(source=tile, pics=[dict(src_off=0, size=len(tile), capacity=len(tile), header=head, trailer=b"")])
    arena, table, guards_ok = assemble_host(batch, len(frame))
    assert guards_ok and arena == frame and table.tolist() == [[0, len(frame)], [len(frame), 0]]


REFUSED = (dict(width=4097), dict(width=0), dict(height=0), dict(width=-1), dict(height=65537), dict(render_width=0), dict(render_height=65537), dict(color_space=7),
           dict(y_dc_delta_q=16), dict(uv_dc_delta_q=-16), dict(uv_ac_delta_q=16), dict(ref_deltas=(0, 64, 0, 0)), dict(mode_deltas=(0, -64)),
           dict(last_ref_deltas=(-64, 0, 0, 0)), dict(last_mode_deltas=(64, 0)), dict(frame_type=2), dict(show_frame=2), dict(error_resilient_mode=2),
           dict(intra_only=2), dict(reset_frame_context=4), dict(refresh_frame_context=2), dict(frame_parallel_decoding_mode=2), dict(frame_context_idx=4),
           dict(ref_dpb_index=(0, 8, 0)), dict(ref_frame_sign_bias=(0, 0, 2, 0)), dict(allow_hp=2), dict(reference_mode=3), dict(allow_comp_inter_inter=2),
           dict(color_space=8), dict(color_range=2), dict(filter_level=64), dict(sharpness_level=8), dict(mode_ref_delta_enabled=2), dict(mode_ref_delta_update=2),
           dict(frame_type=FM.INTER, show_frame=1, intra_only=1))


@pytest.mark.parametrize("change", REFUSED, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_refused_parameters_leave_the_buffer_untouched(change):
    rc, buf, ub, cb = FM.host_headers(FM.inter(**change) if "frame_type" not in change else FM.params(**change))
    assert rc == -1 and np.all(buf == 0xA5) and (ub, cb) == (0x77777777, 0x77777777)


def test_refused_capacity_and_null_pointers():
    p = FM.params()
    need = len(FM.host_header_bytes(p))
    rc, buf, *_ = FM.host_headers(p, capacity=need - 1)
    assert rc == -1 and np.all(buf == 0xA5)
    rc, buf, ub, cb = FM.host_headers(p, capacity=need)
    assert rc == 0 and ub + cb == need and np.all(buf[need:] == 0xA5)
    lib, s, out, n = B.load(), FM.struct(p), np.full(64, 0xA5, np.uint8), C.c_uint32(7)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert lib.svt_hip_frame_header_host(None, ptr, 64, C.byref(n), C.byref(n)) == -1
    assert lib.svt_hip_frame_header_host(C.byref(s), None, 64, C.byref(n), C.byref(n)) == -1
    assert lib.svt_hip_frame_header_host(C.byref(s), ptr, 64, None, C.byref(n)) == -1
    assert lib.svt_hip_frame_header_host(C.byref(s), ptr, 64, C.byref(n), None) == -1
    assert np.all(out == 0xA5) and n.value == 7


def test_struct_sizes_match_header():
    src = ('#include <stdio.h>\n#include "svtvp9_hip.h"\nint main(void){printf("%zu %zu %zu %d %u %d",sizeof(svt_frame_params),sizeof(svt_frame_packet),'
           'sizeof(svt_frame_entry),SVT_FRAME_HEADER_MAX,SVT_FRAME_SIZE_NONE,SVT_FRAME_MAX_PICS);return 0;}')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", f"{T.ROOT}/include", os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(td, "s")]).split()]
    assert got == [64, 88, 8, B.FRAME_HEADER_MAX, B.FRAME_SIZE_NONE, B.FRAME_MAX_PICS]
    assert got[:3] == [C.sizeof(B.FrameParams), C.sizeof(B.FramePacket), B.FRAME_ENTRY_DTYPE.itemsize]


def test_header_max_covers_every_case_and_a_seeded_sweep():
    longest = max(sum(FM.fixture_case(n)[2:]) for n in HEADER_NAMES)
    rng = np.random.default_rng(20240)
    for i in range(2000):
        p = FM.random_params(rng)
        rc, buf, ub, cb = FM.host_headers(p)
        assert rc == 0, p
        longest = max(longest, ub + cb)
        if i % 50 == 0:       # the model agrees on the sweep too (every 50th set: it is the slow side)
            u, c = FM.headers(p)
            assert bytes(buf[:ub + cb]) == u + c, p
    for p in FM.worst_params():
        rc, _, ub, cb = FM.host_headers(p)
        assert rc == 0
        longest = max(longest, ub + cb)
    # the derivation's longest uncompressed header (csrc/frame_core.h): 27 bytes without a padding bit
    assert len(FM.uncompressed_bits(FM.worst_params()[0], 0).bits) == 216
    assert 27 + 3 <= longest <= B.FRAME_HEADER_MAX


# ---------------------------------------------------------------------------------------------------
# assembly: the host form
# ---------------------------------------------------------------------------------------------------
GUARD = 64


def aligned(n, fill):
    """n bytes of `fill` that start on a 16-byte boundary"""
    raw = np.full(n + 16, fill, np.uint8)
    off = -raw.ctypes.data % 16
    return raw[off:off + n]


def assemble_host(batch, capacity, sizes=None):
    """svt_hip_frame_assemble_host over the batch: (arena bytes up to min(total, capacity), table, guards and the rest of the arena intact)"""
    n = len(batch["pics"])
    source = aligned(len(batch["source"]), 0)
    source[:] = batch["source"]
    sizes = FM.sizes_array(batch) if sizes is None else sizes
    buf = aligned(GUARD + capacity + GUARD, 0xA5)
    table = np.full((n + 1 + 4, 2), 0x5A5A5A5A, np.uint32)
    arr = FM.packets(batch, source.ctypes.data, sizes.ctypes.data)
    rc = B.load().svt_hip_frame_assemble_host(n, arr, buf[GUARD:].ctypes.data_as(C.c_void_p), capacity, table.ctypes.data_as(C.c_void_p))
    assert rc == 0
    total = int(table[n, 0])
    used = min(total, capacity)
    ok = bool(np.all(buf[:GUARD] == 0xA5) and np.all(buf[GUARD + capacity:] == 0xA5) and np.all(table[n + 1:] == 0x5A5A5A5A))
    if total <= capacity:
        ok = ok and bool(np.all(buf[GUARD + used:GUARD + capacity] == 0xA5))
    return bytes(buf[GUARD:GUARD + used]), table[:n + 1].copy(), ok


def with_failures(batch):
    """the batch with picture 5 answering SVT_BOOL_SIZE_OVERFLOW and picture 20 a size above its capacity"""
    pics = [dict(p) for p in batch["pics"]]
    pics[5]["size"] = B.BOOL_SIZE_OVERFLOW
    pics[20]["size"] = pics[20]["capacity"] + 1
    return dict(source=batch["source"], pics=pics)


def test_standard_batches_meet_all_256_alignment_pairs():
    have = set().union(*[FM.pairs(b, 0, 0) for b in FM.standard_batches()])
    assert len(have) == 256
    heads = {len(p["header"]) for b in FM.standard_batches() for p in b["pics"]}
    assert {1, B.FRAME_HEADER_MAX} <= heads and {len(p["trailer"]) for b in FM.standard_batches() for p in b["pics"]} == {0, 1, 2, 3, 4}
    assert {p["size"] for b in FM.standard_batches() for p in b["pics"]} == set(FM.TILE_SIZES)


@pytest.mark.parametrize("k", range(9))
def test_assembly_host_form_equals_the_concatenation(k):
    batch = FM.standard_batches()[k]
    want, table = FM.expected(batch)
    got, got_table, ok = assemble_host(batch, len(want) + 40)
    assert ok and got == want and np.array_equal(got_table, table)
    got, got_table, ok = assemble_host(batch, len(want))
    assert ok and got == want and np.array_equal(got_table, table)


def test_assembly_host_form_one_picture():
    batch = FM.make_batch(3, n_pics=1)
    want, table = FM.expected(batch)
    got, got_table, ok = assemble_host(batch, len(want))
    assert ok and got == want and np.array_equal(got_table, table)


def test_assembly_host_form_overflow_rules():
    batch = with_failures(FM.standard_batches()[8])
    want, table = FM.expected(batch)
    assert int(table[32, 1]) == 2 and table[5, 1] == table[20, 1] == B.FRAME_SIZE_NONE and table[6, 0] == table[5, 0]
    got, got_table, ok = assemble_host(batch, len(want))
    assert ok and got == want and np.array_equal(got_table, table)


@pytest.mark.parametrize("short", ("one", "all"))
def test_assembly_host_form_short_arena(short):
    batch = FM.standard_batches()[8]
    want, table = FM.expected(batch)
    cap = len(want) - 1 if short == "one" else 0
    got, got_table, ok = assemble_host(batch, cap)
    assert ok and np.array_equal(got_table, table) and got == want[:cap]      # (the host form cuts every run at the capacity)


def test_assembly_host_form_refusals():
    lib = B.load()
    batch = FM.make_batch(1, n_pics=2)
    src, sizes, arena, table = aligned(len(batch["source"]), 0), FM.sizes_array(batch), np.full(20000, 0xA5, np.uint8), np.full((8, 2), 0x5A5A5A5A, np.uint32)
    ap, tp = arena.ctypes.data_as(C.c_void_p), table.ctypes.data_as(C.c_void_p)

    def call(n=2, arr=None, a=ap, t=tp, **change):
        if arr is None:
            arr = FM.packets(batch, src.ctypes.data, sizes.ctypes.data)
            for k, v in change.items():
                setattr(arr[1], k, v)
        return lib.svt_hip_frame_assemble_host(n, arr, a, len(arena), t)
    assert call() == 0
    arena[:] = 0xA5
    table[:] = 0x5A5A5A5A
    assert call(n=0) == -1 and call(n=33) == -1 and call(a=None) == -1 and call(t=None) == -1
    assert lib.svt_hip_frame_assemble_host(2, None, ap, len(arena), tp) == -1
    assert call(header_len=B.FRAME_HEADER_MAX + 1) == -1 and call(trailer_len=5) == -1 and call(d_tile_size=None) == -1 and call(d_tile=None) == -1
    assert np.all(arena == 0xA5) and np.all(table == 0x5A5A5A5A)


# ---------------------------------------------------------------------------------------------------
# assembly: the kernel's text on the CPU
# ---------------------------------------------------------------------------------------------------
def emu_request(path):
    """the standard batches with room to spare, exactly fitting, with the two failed pictures, one byte short, without an arena, a
    one-picture batch and one long tile; returns the number of batches"""
    std = FM.standard_batches()
    runs = [(b, len(FM.expected(b)[0]) + 40) for b in std] + [(std[0], len(FM.expected(std[0])[0]))]
    failed = with_failures(std[8])
    runs += [(failed, len(FM.expected(failed)[0])), (std[8], len(FM.expected(std[8])[0]) - 1), (std[3], len(FM.expected(std[3])[0]) - 1), (std[8], 0)]
    one = FM.make_batch(3, n_pics=1)
    runs.append((one, len(FM.expected(one)[0])))
    # several passes of the grid-stride loop (the emulation runs EMU_WGS workgroups a picture: 8 KiB a pass), source 5 bytes off a boundary
    rng = np.random.default_rng(99)
    long = dict(source=rng.integers(0, 256, 40100, dtype=np.uint8), pics=[dict(src_off=5, size=40000, capacity=40000, header=b"\x82\x49\x83", trailer=b"\x88")])
    runs.append((long, 40004))
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(runs)))
        for batch, cap in runs:
            f.write(struct.pack("<iIi", len(batch["pics"]), cap, len(batch["source"])))
            f.write(batch["source"].tobytes())
            for p in batch["pics"]:
                f.write(struct.pack("<iIIii", p["src_off"], p["size"], p["capacity"], len(p["header"]), len(p["trailer"])))
                f.write(p["header"].ljust(B.FRAME_HEADER_MAX, b"\0") + p["trailer"].ljust(4, b"\0"))
    return len(runs)


EMU_WGS = 2       # workgroups per picture of the emulated launch: a thread per lane makes a workgroup slow, and the loop takes more passes


def build_emu(td, sanitize):
    emu, src = os.path.join(T.ROOT, "tests", "emu", "frame"), os.path.join(T.ROOT, "svt-vp9_amd")
    exe = os.path.join(td, "frame_emu_san" if sanitize else "frame_emu")
    cmd = ["g++", "-x", "c++", "-std=c++17", "-O1", "-w", f"-DFR_WGS={EMU_WGS}"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) + \
          [f"-I{os.path.dirname(emu)}", f"-I{os.path.join(src, 'csrc')}", os.path.join(emu, "frame_emu.cpp"), "-x", "c", os.path.join(src, "host", "frame_host.c"),
           os.path.join(src, "host", "boolcode_host.c"), "-lpthread", "-o", exe]
    return exe if subprocess.run(cmd, capture_output=True).returncode == 0 else None


def run_emu(exe, req, n):
    r = subprocess.run([exe, req], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bad 0" in r.stdout and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(" ok") == n


def test_kernel_text_on_the_cpu_equals_the_host_form():
    with tempfile.TemporaryDirectory() as td:
        req = os.path.join(td, "batches.bin")
        n = emu_request(req)
        exe = build_emu(td, False)
        assert exe, "the emulation does not compile"
        run_emu(exe, req, n)


def test_kernel_text_on_the_cpu_under_address_and_ub_sanitizers():
    """a stand-alone program: every tile in an allocation that is exactly the 16-byte blocks holding its bytes, so a load from a block
    without a source byte is reported.  Where the host compiler links no sanitizer runtime the program runs plain (the test above)."""
    with tempfile.TemporaryDirectory() as td:
        req = os.path.join(td, "batches.bin")
        n = emu_request(req)
        exe = build_emu(td, True) or build_emu(td, False)
        assert exe
        run_emu(exe, req, n)

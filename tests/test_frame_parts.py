"""CPU: the three-part frame assembly's host side (host/frame_host.c, rules in csrc/frame_core.h): the header-byte rule that fills
first_part_size in, against a plain bit writer; svt_hip_frame_assemble_parts_host against the concatenation and against
svt_hip_frame_assemble_host fed the host-joined header; every condition that withholds a picture at both sides of its bound; the
refusals; svt_hip_frame_header_uncompressed_host against svt_hip_frame_header_coef_host for every header case."""
import ctypes as C

import numpy as np
import pytest

import frame_model as FM
import frame_parts_model as PM
import svt_testlib as T

B = T.B
NONE = B.FRAME_SIZE_NONE


def one_picture(header, size_bit, comp, tile=2, comp_cap=None, tile_cap=None, trailer=b"", live=None):
    """a one-picture batch; live: the bytes the source really holds for the compressed part (a withheld picture's are never read)"""
    rng = np.random.default_rng(comp & 0xFFFF)
    n = comp if live is None else live
    source = rng.integers(0, 256, n + 4200, dtype=np.uint8)
    return dict(source=source, pics=[dict(comp_off=3, comp=comp, comp_cap=comp if comp_cap is None else comp_cap, tile_off=n + 8, tile=tile,
                                          tile_cap=tile if tile_cap is None else tile_cap, header=header, size_bit=size_bit, trailer=trailer)])


@pytest.mark.parametrize("phase", range(8))
def test_header_byte_rule_equals_a_plain_bit_writer(phase):
    """all 8 phases of size_bit: the field spans 2 bytes at phase 0 and 3 otherwise; placeholders of all ones and all zeros show that the
    field is replaced and nothing else is touched"""
    for fill in (0xFF, 0x00):
        for value in (1, 0x00FF, 0x0100, 0xFFFF):
            for first in (0, 1, 24):                    # the field's first byte: at the header's start, inside, and ending at its last bit
                size_bit = 8 * first + phase
                hl = max((size_bit + 16 + 7) // 8, 2) if first != 24 else B.FRAME_UNCOMPRESSED_MAX
                if size_bit + 16 > 8 * hl:
                    continue
                batch = one_picture(bytes([fill]) * hl, size_bit, value)
                rc, arena, table, ok = PM.assemble_host(batch, hl + value + 2 + 8)
                want = PM.patched(batch["pics"][0]["header"], size_bit, value)
                assert rc == 0 and ok and bytes(arena[:hl]) == want, (fill, value, size_bit)
                assert sum(a != b for a, b in zip(want, bytes([fill]) * hl)) <= (2 if phase == 0 else 3)
                assert table.tolist() == [[0, hl + value + 2], [hl + value + 2, 0]]
                assert bytes(arena[:hl + value + 2]) == PM.expected(batch)[0]


@pytest.mark.parametrize("k", range(4))
def test_host_form_equals_the_concatenation(k):
    batch = PM.standard_batches()[k]
    want, want_table = PM.expected(batch)
    for slack in (40, 0):
        rc, arena, table, ok = PM.assemble_host(batch, len(want) + slack)
        assert rc == 0 and ok and bytes(arena[:len(want)]) == want and np.all(arena[len(want):] == 0xA5) and np.array_equal(table, want_table)


def test_host_form_equals_the_two_part_form_fed_the_host_joined_header():
    rng = np.random.default_rng(77)
    batch = PM.make_batch(40)
    for p in batch["pics"]:                             # a joined header must fit svt_frame_packet's 56 bytes
        p["comp"] = int(rng.integers(1, B.FRAME_HEADER_MAX - len(p["header"]) + 1))
        p["comp_cap"] = p["comp"] + 3
    batch["pics"][7]["tile"] = PM.OVERFLOW
    sizes = PM.sizes_array(batch)
    arr = (B.FramePacket * 32)()
    base = batch["source"].ctypes.data
    for i, (q, p) in enumerate(zip(arr, batch["pics"])):
        head = PM.patched(p["header"], p["size_bit"], p["comp"]) + batch["source"][p["comp_off"]:p["comp_off"] + p["comp"]].tobytes()
        q.d_tile, q.d_tile_size, q.tile_capacity, q.header_len, q.trailer_len = base + p["tile_off"], sizes.ctypes.data + 8 * i + 4, p["tile_cap"], len(head), len(p["trailer"])
        C.memmove(q.header, head, len(head))
        C.memmove(q.trailer, p["trailer"], len(p["trailer"]))
    for cap in (70000, 3000, 11):
        rc, arena, table, ok = PM.assemble_host(batch, cap)
        a2, t2 = np.full(cap + 128, 0xA5, np.uint8), np.zeros((33, 2), np.uint32)
        assert B.load().svt_hip_frame_assemble_host(32, arr, a2.ctypes.data + 64, cap, t2.ctypes.data_as(C.c_void_p)) == 0
        assert rc == 0 and ok and np.array_equal(arena, a2[64:64 + cap]) and np.array_equal(table, t2) and np.all(a2[:64] == 0xA5) and np.all(a2[64 + cap:] == 0xA5)
    assert int(table[32, 1]) == 1 and int(table[7, 1]) == NONE


def test_every_condition_that_withholds_a_picture_at_both_sides_of_its_bound():
    h = bytes(range(1, 9))

    def size(**kw):
        batch = one_picture(h, 13, **kw)
        rc, arena, table, ok = PM.assemble_host(batch, 70000)
        assert rc == 0 and ok and (int(table[0, 1]) == NONE) == (not PM.has_packet(batch["pics"][0]))
        if int(table[0, 1]) == NONE:
            assert table.tolist() == [[0, NONE], [0, 1]] and np.all(arena == 0xA5)
        else:
            assert bytes(arena[:int(table[0, 1])]) == PM.expected(batch)[0]
        return int(table[0, 1])
    # the tile: the existing rule
    assert size(comp=5, tile=100, tile_cap=100) == 8 + 5 + 100 and size(comp=5, tile=101, tile_cap=100) == NONE
    assert size(comp=5, tile=PM.OVERFLOW, tile_cap=PM.OVERFLOW, live=5) == NONE and size(comp=5, tile=0, tile_cap=0) == 8 + 5
    # the compressed header: 0, its capacity, 16 bits, the coder's overflow word
    assert size(comp=0, comp_cap=10) == NONE and size(comp=1, comp_cap=10) == 8 + 1 + 2
    assert size(comp=10, comp_cap=10) == 8 + 10 + 2 and size(comp=11, comp_cap=10, live=11) == NONE
    assert size(comp=0xFFFF, comp_cap=0x20000) == 8 + 0xFFFF + 2 and size(comp=0x10000, comp_cap=0x20000) == NONE
    assert size(comp=PM.OVERFLOW, comp_cap=PM.OVERFLOW, live=4) == NONE
    # in a batch: the pictures behind a withheld one start where it would have
    batch = PM.with_failures(PM.standard_batches()[1], PM.REASONS)
    want, want_table = PM.expected(batch)
    rc, arena, table, ok = PM.assemble_host(batch, len(want) + 9)
    assert rc == 0 and ok and bytes(arena[:len(want)]) == want and np.array_equal(table, want_table) and int(table[32, 1]) == len(PM.REASONS)
    assert all(int(table[3 + 4 * k, 1]) == NONE and int(table[4 + 4 * k, 0]) == int(table[3 + 4 * k, 0]) for k in range(len(PM.REASONS)))


def test_short_arenas_end_inside_each_part():
    batch = PM.make_batch(26, n_pics=2)
    want, want_table = PM.expected(batch)
    for cap in PM.short_capacities(batch) + (0,):
        rc, arena, table, ok = PM.assemble_host(batch, cap)
        assert rc == 0 and ok and np.array_equal(table, want_table) and bytes(arena) == want[:cap]


def test_refusals_write_nothing():
    batch = PM.make_batch(1, n_pics=2)
    sizes = PM.sizes_array(batch)
    lib = B.load()

    def call(n=2, arr=0, arena=1, table=1, **change):
        a, t = np.full(9000, 0xA5, np.uint8), np.full(16, 0x5A5A5A5A, np.uint32)
        if arr == 0:
            arr = PM.packets(batch, batch["source"].ctypes.data, sizes.ctypes.data)
            for k, v in change.items():
                setattr(arr[1], k, v)
        rc = lib.svt_hip_frame_assemble_parts_host(n, arr, a.ctypes.data if arena else None, 9000, t.ctypes.data_as(C.c_void_p) if table else None)
        return rc, bool(np.all(a == 0xA5) and np.all(t == 0x5A5A5A5A))
    for kw in (dict(n=0), dict(n=33), dict(arr=None), dict(arena=0), dict(table=0), dict(header_len=B.FRAME_UNCOMPRESSED_MAX + 1), dict(trailer_len=5),
               dict(d_tile_size=None), dict(d_compressed_size=None), dict(d_tile=None), dict(d_compressed=None),
               dict(size_bit=8 * len(batch["pics"][1]["header"]) - 15), dict(header_len=1, size_bit=0)):
        assert call(**kw) == (-1, True), kw
    assert call(size_bit=8 * len(batch["pics"][1]["header"]) - 16) == (0, False)
    assert call() == (0, False)


@pytest.mark.parametrize("name,p", FM.CASES, ids=[c[0] for c in FM.CASES])
def test_uncompressed_header_then_the_patch_equals_the_joined_header(name, p):
    lib, s = B.load(), FM.struct(p)
    pre, suf = (C.c_uint16 * 8)(), (C.c_uint16 * 208)()
    n_pre, n_suf = C.c_uint32(), C.c_uint32()
    assert lib.svt_hip_frame_header_parts_host(C.byref(s), pre, C.byref(n_pre), suf, C.byref(n_suf)) == 0
    bools = np.array(list(pre[:n_pre.value]) + [0 << 8 | 128] * 4 + list(suf[:n_suf.value]), np.uint16)
    joined, ub, cb = np.zeros(400, np.uint8), C.c_uint32(), C.c_uint32()
    assert lib.svt_hip_frame_header_coef_host(C.byref(s), bools.ctypes.data_as(C.c_void_p), len(bools), joined.ctypes.data_as(C.c_void_p), 400, C.byref(ub), C.byref(cb)) == 0
    assert bytes(joined[:ub.value + cb.value]) == FM.host_header_bytes(p)           # (four "no update" bits: the plain header)
    out, n, bit = np.full(40, 0xA5, np.uint8), C.c_uint32(), C.c_uint32()
    assert lib.svt_hip_frame_header_uncompressed_host(C.byref(s), out.ctypes.data_as(C.c_void_p), B.FRAME_UNCOMPRESSED_MAX, C.byref(n), C.byref(bit)) == 0
    assert n.value == ub.value and np.all(out[n.value:] == 0xA5) and bit.value + 16 <= 8 * n.value
    assert bytes(out[:n.value]) == FM.uncompressed(p, 0) == PM.patched(bytes(joined[:ub.value]), bit.value, 0)
    assert PM.patched(bytes(out[:n.value]), bit.value, cb.value) == bytes(joined[:ub.value])
    # and through the assembly: the three parts give the joined header's packet
    comp, tile = joined[ub.value:ub.value + cb.value].copy(), np.arange(5, dtype=np.uint8)
    sizes = np.array([cb.value, 5], np.uint32)
    q = (B.FramePartsPacket * 1)()
    q[0].d_compressed, q[0].d_compressed_size, q[0].compressed_capacity = comp.ctypes.data, sizes.ctypes.data, cb.value
    q[0].d_tile, q[0].d_tile_size, q[0].tile_capacity, q[0].size_bit, q[0].header_len = tile.ctypes.data, sizes.ctypes.data + 4, 5, bit.value, n.value
    C.memmove(q[0].header, out.ctypes.data, n.value)
    arena, table = np.zeros(500, np.uint8), np.zeros((2, 2), np.uint32)
    assert lib.svt_hip_frame_assemble_parts_host(1, q, arena.ctypes.data, 500, table.ctypes.data_as(C.c_void_p)) == 0
    assert bytes(arena[:int(table[1, 0])]) == bytes(joined[:ub.value + cb.value]) + tile.tobytes()
    # refusals of the new header entry
    assert lib.svt_hip_frame_header_uncompressed_host(C.byref(s), out.ctypes.data_as(C.c_void_p), n.value - 1, C.byref(n), C.byref(bit)) == -1
    assert lib.svt_hip_frame_header_uncompressed_host(None, out.ctypes.data_as(C.c_void_p), 40, C.byref(n), C.byref(bit)) == -1

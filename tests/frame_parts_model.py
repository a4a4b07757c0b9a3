"""Python model and shared cases of the three-part frame assembly (svt_hip_frame_parts_batch_device / svt_hip_frame_assemble_parts_host),
written independently of the C text: packets are uncompressed header || compressed header || tile || trailer, the 16 bits of
first_part_size at an arbitrary bit position of the header say the compressed header's size.  The seeded batches the CPU tests, the
emulation and the GPU tests share; their concatenation through a plain bit writer; the descriptors; the host form."""
import ctypes as C
import struct

import numpy as np

import svt_testlib as T

B = T.B
COMP_SIZES = (1, 15, 16, 17, 31, 33, 300)
TILE_SIZES = (2, 16, 4097)
TILE_AT = 512                               # a picture's slot of the source: the compressed bytes from 0 .. 15 on, the tile from TILE_AT + 0 .. 15 on
SLOT = TILE_AT + 4097 + 16 + 31            # (a multiple of 16)
assert SLOT % 16 == 0
OVERFLOW = B.BOOL_SIZE_OVERFLOW


def patched(header, size_bit, value):
    """the header's bytes with the bits [size_bit, size_bit + 16) saying value, MSB first: a plain bit list"""
    bits = [(byte >> (7 - k)) & 1 for byte in header for k in range(8)]
    assert size_bit + 16 <= len(bits) and 0 <= value < 1 << 16
    bits[size_bit:size_bit + 16] = [(value >> (15 - k)) & 1 for k in range(16)]
    return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


def make_batch(seed, n_pics=32):
    """dict(source, pics=[dict(comp_off, comp, comp_cap, tile_off, tile, tile_cap, header, size_bit, trailer)]): picture i's compressed bytes
    start (i + seed) % 16 bytes into its slot of the source and its tile (3 i + seed + 5) % 16 bytes behind TILE_AT; the sizes walk through
    COMP_SIZES x TILE_SIZES; header length, the field's place, its placeholder bits and the trailer are drawn"""
    rng = np.random.default_rng(9100 + seed)
    source = rng.integers(0, 256, n_pics * SLOT + 64, dtype=np.uint8)
    pics = []
    for i in range(n_pics):
        comp, tile = COMP_SIZES[(i + seed) % len(COMP_SIZES)], TILE_SIZES[(i // len(COMP_SIZES) + i + seed) % len(TILE_SIZES)]
        hl = int(rng.integers(2, B.FRAME_UNCOMPRESSED_MAX + 1))
        pics.append(dict(comp_off=i * SLOT + (i + seed) % 16, comp=comp, comp_cap=comp + int(rng.integers(0, 8)),
                         tile_off=i * SLOT + TILE_AT + (3 * i + seed + 5) % 16, tile=tile, tile_cap=tile + int(rng.integers(0, 8)),
                         header=rng.integers(0, 256, hl, dtype=np.uint8).tobytes(), size_bit=int(rng.integers(0, 8 * hl - 16 + 1)),
                         trailer=rng.integers(0, 256, int(rng.integers(0, 5)), dtype=np.uint8).tobytes()))
    return dict(source=source, pics=pics)


def standard_batches():
    return [make_batch(k) for k in range(4)]


def has_packet(p):
    return not (p["tile"] == OVERFLOW or p["tile"] > p["tile_cap"] or p["comp"] == OVERFLOW or p["comp"] == 0 or p["comp"] > p["comp_cap"] or p["comp"] > 0xFFFF)


def with_failures(batch, which):
    """the batch with picture 3 + 4 k withheld for reason which[k]"""
    pics = [dict(p) for p in batch["pics"]]
    for k, why in enumerate(which):
        p = pics[3 + 4 * k]
        if why == "tile_overflow":
            p["tile"] = OVERFLOW
        elif why == "tile_above_capacity":
            p["tile"] = p["tile_cap"] + 1
        elif why == "comp_overflow":
            p["comp"] = OVERFLOW
        elif why == "comp_zero":
            p["comp"] = 0
        elif why == "comp_above_capacity":
            p["comp"] = p["comp_cap"] + 1
        elif why == "comp_above_16_bits":
            p["comp"], p["comp_cap"] = 0x10000, 0x20000
        else:
            raise KeyError(why)
    return dict(source=batch["source"], pics=pics)


REASONS = ("tile_overflow", "tile_above_capacity", "comp_overflow", "comp_zero", "comp_above_capacity", "comp_above_16_bits")


def expected(batch):
    """(the dense arena, the table as (n + 1, 2) uint32) by concatenation"""
    out, table, none = b"", [], 0
    src = batch["source"]
    for p in batch["pics"]:
        if not has_packet(p):
            table.append((len(out), B.FRAME_SIZE_NONE))
            none += 1
            continue
        pkt = (patched(p["header"], p["size_bit"], p["comp"]) + src[p["comp_off"]:p["comp_off"] + p["comp"]].tobytes() +
               src[p["tile_off"]:p["tile_off"] + p["tile"]].tobytes() + p["trailer"])
        table.append((len(out), len(pkt)))
        out += pkt
    table.append((len(out), none))
    return out, np.array(table, np.uint32)


def phases(batch, base_address, arena_address):
    """per part the (source address mod 16, destination address mod 16) of the batch's packets: (compressed, tile)"""
    _, table = expected(batch)
    comp, tile = set(), set()
    for p, (off, size) in zip(batch["pics"], table):
        if size != B.FRAME_SIZE_NONE:
            at = arena_address + int(off) + len(p["header"])
            comp.add(((base_address + p["comp_off"]) % 16, at % 16))
            tile.add(((base_address + p["tile_off"]) % 16, (at + p["comp"]) % 16))
    return comp, tile


def sizes_array(batch):
    """the size words: picture i's compressed size at word 2 i, its tile size at word 2 i + 1"""
    return np.array([v for p in batch["pics"] for v in (p["comp"], p["tile"])], np.uint32)


def packets(batch, source_address, size_address):
    arr = (B.FramePartsPacket * len(batch["pics"]))()
    for i, (q, p) in enumerate(zip(arr, batch["pics"])):
        q.d_compressed, q.d_compressed_size, q.compressed_capacity = source_address + p["comp_off"], size_address + 8 * i, p["comp_cap"]
        q.d_tile, q.d_tile_size, q.tile_capacity = source_address + p["tile_off"], size_address + 8 * i + 4, p["tile_cap"]
        q.size_bit, q.header_len, q.trailer_len = p["size_bit"], len(p["header"]), len(p["trailer"])
        C.memmove(q.header, p["header"], len(p["header"]))
        C.memmove(q.trailer, p["trailer"], len(p["trailer"]))
    return arr


def assemble_host(batch, capacity, guard=64, fill=0xA5, arr=None, n=None):
    """svt_hip_frame_assemble_parts_host: (rc, arena bytes [0, capacity), table (n + 1, 2), guards intact)"""
    n = len(batch["pics"]) if n is None else n
    sizes = sizes_array(batch)
    if arr is None:
        arr = packets(batch, batch["source"].ctypes.data, sizes.ctypes.data)
    arena = np.full(guard + capacity + guard, fill, np.uint8)
    table = np.full(2 * (max(n, 0) + 1) + 8, 0x5A5A5A5A, np.uint32)
    rc = B.load().svt_hip_frame_assemble_parts_host(n, arr, arena.ctypes.data + guard, capacity, table.ctypes.data_as(C.c_void_p))
    ok = bool(np.all(arena[:guard] == fill) and np.all(arena[guard + capacity:] == fill) and np.all(table[2 * (max(n, 0) + 1):] == 0x5A5A5A5A))
    return rc, arena[guard:guard + capacity], table[:2 * (max(n, 0) + 1)].reshape(-1, 2), ok


def short_capacities(batch):
    """arena capacities that end inside the first picture's header, inside its compressed part and inside its tile"""
    p = batch["pics"][0]
    hl = len(p["header"])
    return (hl - 1, hl + max(p["comp"] // 2, 0), hl + p["comp"] + p["tile"] // 2)


def emu_request(path, batches_and_caps):
    """the emulation's input file: int32 n_batches; per batch int32 n_pics, uint32 arena_capacity, int32 source_bytes, the source; per picture
    int32 comp_off, uint32 comp, comp_cap, int32 tile_off, uint32 tile, tile_cap, int32 header_len, size_bit, trailer_len, 27 header bytes,
    4 trailer bytes"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(batches_and_caps)))
        for batch, cap in batches_and_caps:
            f.write(struct.pack("<iIi", len(batch["pics"]), cap, len(batch["source"])))
            f.write(batch["source"].tobytes())
            for p in batch["pics"]:
                f.write(struct.pack("<iIIiIIiii", p["comp_off"], p["comp"], p["comp_cap"], p["tile_off"], p["tile"], p["tile_cap"], len(p["header"]), p["size_bit"],
                                    len(p["trailer"])))
                f.write(p["header"].ljust(B.FRAME_UNCOMPRESSED_MAX, b"\0") + p["trailer"].ljust(4, b"\0"))
    return len(batches_and_caps)


def emu_cases():
    """what the emulation runs: the standard batches with room to spare and exactly full, a batch with every reason to withhold a picture,
    and a one-picture batch of every compressed size under the three short arenas"""
    out = []
    for b in standard_batches():
        total = len(expected(b)[0])
        out += [(b, total + 40), (b, total)]
    out.append((with_failures(standard_batches()[1], REASONS), len(expected(standard_batches()[1])[0])))
    for k in range(len(COMP_SIZES)):
        one = make_batch(20 + k, n_pics=2)
        out += [(one, c) for c in short_capacities(one)]
    return out

"""GPU: the frame stage's assembly kernel (csrc/frame.hip) through the C ABI, exactly: seeded batches of 32 synthetic tiles against a numpy
concatenation over all 256 (source address mod 16, destination address mod 16) pairs, with guards round the arena and behind the table, a
one-picture batch, an arena in pinned host memory; the overflow and short-arena rules; a tile of many passes of the grid-stride loop; the
chain tokeniser -> mode info -> bool coder -> frame enqueued without a host round trip against the reference's whole frames
(tests/golden/frame_reference.npz); refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import boolcode_model as BM
import frame_model as FM
import modes_inter_model as IM
import modes_model as MM
import svt_testlib as T
import test_gpu_modes as GK
import test_gpu_modes_inter as GI
from test_gpu_tokenize import TokBuffers, tokenize_device, upload

B = T.B
pytestmark = pytest.mark.gpu
GUARD = 64
FILL, TABLE_FILL = 0xA5, 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    lib, c = B.load(), C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    B.check(lib.svt_hip_boolcode_set_tables(c, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_set_tables(c, MM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(c, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    yield c
    lib.svt_hip_ctx_destroy(c)


class Arena:
    """capacity bytes with GUARD bytes in front and behind, and a table of n + 1 entries with guard words behind; pinned: the arena
    lives in svt_hip_host_alloc memory"""

    def __init__(self, ctx, n, capacity, pinned=False):
        self.ctx, self.n, self.cap, self.pinned = ctx, n, capacity, pinned
        if pinned:
            self.ptr = C.c_void_p()
            B.check(B.load().svt_hip_host_alloc(ctx, GUARD + capacity + GUARD, C.byref(self.ptr)))
            self.host = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), (GUARD + capacity + GUARD,))
            self.host[:] = FILL
            self.base = self.ptr.value
        else:
            self.bytes = torch.full((GUARD + capacity + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            self.base = self.bytes.data_ptr()
        self.table = torch.full((2 * (n + 1) + 8,), TABLE_FILL, dtype=torch.int32, device="cuda")

    @property
    def address(self):
        return self.base + GUARD

    def result(self):
        """(arena bytes [0, capacity), table (n + 1, 2), front guard, back guard, table guard)"""
        raw = self.host.copy() if self.pinned else self.bytes.cpu().numpy()
        t = self.table.cpu().numpy().view(np.uint32)
        return raw[GUARD:GUARD + self.cap], t[:2 * (self.n + 1)].reshape(-1, 2), raw[:GUARD], raw[GUARD + self.cap:], t[2 * (self.n + 1):]

    def free(self):
        if self.pinned:
            B.load().svt_hip_host_free(self.ctx, self.ptr)


class Launch:
    """a batch uploaded and its outputs allocated: .met = the (source address mod 16, destination address mod 16) pairs of its tiles,
    from the addresses the buffers really have; run() enqueues one svt_hip_frame_batch_device and synchronises"""

    def __init__(self, ctx, batch, capacity, pinned=False):
        self.ctx, self.batch, self.n = ctx, batch, len(batch["pics"])
        self.src = torch.from_numpy(batch["source"]).cuda()
        self.sizes = torch.from_numpy(FM.sizes_array(batch).view(np.int32)).cuda()
        self.arena = Arena(ctx, self.n, capacity, pinned)
        self.met = FM.pairs(batch, self.src.data_ptr(), self.arena.address)
        torch.cuda.synchronize()

    def run(self):
        """(arena bytes, table, guards intact)"""
        try:
            arr = FM.packets(self.batch, self.src.data_ptr(), self.sizes.data_ptr())
            B.check(B.load().svt_hip_frame_batch_device(self.ctx, self.n, arr, self.arena.address, self.arena.cap, self.arena.table.data_ptr()))
            B.check(B.load().svt_hip_ctx_synchronize(self.ctx))
            data, table, front, back, tguard = self.arena.result()
        finally:
            self.arena.free()
        return data, table, bool(np.all(front == FILL) and np.all(back == FILL) and np.all(tguard == TABLE_FILL))


def check_exact(ctx, batch, slack=40, launch=None, **kw):
    want, want_table = FM.expected(batch)
    launch = launch or Launch(ctx, batch, len(want) + slack, **kw)
    data, table, ok = launch.run()
    assert ok and np.array_equal(table, want_table)
    assert bytes(data[:len(want)]) == want and np.all(data[len(want):] == FILL)
    return launch.met


def test_batches_of_32_tiles_meet_every_alignment_pair(ctx):
    """nine batches: a batch has at most 32 pictures and a picture meets one pair, so the 256 pairs need eight; the ninth is drawn freely
    and has empty tiles.  The coverage is computed from the addresses the buffers really have and asserted before the first launch."""
    batches = FM.standard_batches()
    assert {p["size"] for b in batches for p in b["pics"]} == set(FM.TILE_SIZES)
    assert {1, B.FRAME_HEADER_MAX} <= {len(p["header"]) for b in batches for p in b["pics"]}
    assert {len(p["trailer"]) for b in batches for p in b["pics"]} == {0, 1, 2, 3, 4}
    launches = [Launch(ctx, b, len(FM.expected(b)[0]) + 40) for b in batches]
    assert len(set().union(*[x.met for x in launches])) == 256
    for b, x in zip(batches, launches):
        check_exact(ctx, b, launch=x)


def test_one_picture_batch_and_exact_capacity(ctx):
    check_exact(ctx, FM.make_batch(3, n_pics=1), slack=0)
    check_exact(ctx, FM.standard_batches()[2], slack=0)


def test_arena_in_pinned_host_memory(ctx):
    check_exact(ctx, FM.standard_batches()[8], pinned=True)
    check_exact(ctx, FM.standard_batches()[5], pinned=True, slack=0)


def test_overflow_rules(ctx):
    from test_frame import with_failures
    plain = FM.standard_batches()[8]
    batch = with_failures(plain)
    want, want_table = FM.expected(batch)
    assert want_table[5, 1] == want_table[20, 1] == B.FRAME_SIZE_NONE and int(want_table[32, 1]) == 2
    # later offsets: as if the two pictures were not there
    assert int(want_table[6, 0]) == int(want_table[5, 0]) and int(want_table[21, 0]) == int(want_table[20, 0])
    check_exact(ctx, batch)
    # a short arena: the total is still right, nothing is written past the capacity
    want, want_table = FM.expected(plain)
    for cap in (len(want) - 1, 0):
        data, table, ok = Launch(ctx, plain, cap).run()
        assert ok and np.array_equal(table, want_table) and int(table[32, 0]) == len(want) and len(data) == cap


def test_tile_of_many_passes(ctx):
    """about 1 MiB at source misalignment 5 behind a 3-byte header: 16 passes of the grid-stride loop and a tail"""
    wgs, per_pass = C.c_int32(), C.c_int32()
    B.load().svt_hip_frame_geometry(C.byref(wgs), C.byref(per_pass))
    size = (1 << 20) + 7
    assert size > 15 * per_pass.value
    rng = np.random.default_rng(31)
    batch = dict(source=rng.integers(0, 256, size + 64, dtype=np.uint8), pics=[dict(src_off=5, size=size, capacity=size + 100, header=b"\x82\x49\x83", trailer=b"")])
    met = check_exact(ctx, batch)
    assert {m[0] for m in met} == {5}


def frame_batch(ctx, tiles, heads, trailers=None):
    """the arena and the descriptors of one svt_hip_frame_batch_device over the bool coder's streams (test_gpu_modes.Tile)"""
    n = len(tiles)
    arena = Arena(ctx, n, sum(len(h) + t.cap for h, t in zip(heads, tiles)))
    arr = (B.FramePacket * n)()
    for q, t, h, tr in zip(arr, tiles, heads, trailers or [b""] * n):
        q.d_tile, q.d_tile_size, q.tile_capacity, q.header_len, q.trailer_len = t.bytes.data_ptr(), t.size.data_ptr(), t.cap, len(h), len(tr)
        C.memmove(q.header, h, len(h))
        C.memmove(q.trailer, tr, len(tr))
    return arena, arr


def check_frames(arena, names, trailers=None):
    data, table, front, back, tguard = arena.result()
    assert np.all(front == FILL) and np.all(back == FILL) and np.all(tguard == TABLE_FILL)
    at = 0
    for i, name in enumerate(names):
        frame = bytes(FM.fixture()[f"frame|{name}"]) + (trailers[i] if trailers else b"")
        assert table[i].tolist() == [at, len(frame)]
        assert bytes(data[at:at + len(frame)]) == frame, name
        at += len(frame)
    assert table[len(names)].tolist() == [at, 0] and np.all(data[at:] == FILL)


def test_chain_of_key_pictures_without_host_round_trip(ctx):
    """tokeniser -> key-frame mode info -> bool coder -> frame, the two 72x40 key pictures in one batch of every stage; the headers are
    written by the host form before the first launch"""
    cases = [w for w in FM.WHOLE if w[1] == "modes"]
    assert len(cases) >= 2
    pics = [MM.fixture_picture(w[2]) for w in cases]
    W, H = pics[0]["W"], pics[0]["H"]
    heads = [FM.host_header_bytes(w[3]) for w in cases]
    ups = [upload(p["lf_mi"], p["qcoeff"], p["eob_map"]) for p in pics]
    tbs, mbs = [TokBuffers(W, H, counts=False) for _ in pics], [GK.ModesBuffers(W, H) for _ in pics]
    tiles = [GK.Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]
    arena, arr = frame_batch(ctx, tiles, heads)
    torch.cuda.synchronize()
    lib = B.load()
    tokenize_device(ctx, W, H, ups, tbs)
    GK.modes_device(ctx, W, H, [(u[0], u[2], tb.tok_off) for u, tb in zip(ups, tbs)], mbs)
    B.check(lib.svt_hip_boolcode_batch_device(ctx, len(tiles), (B.BoolStream * len(tiles))(*[t.struct for t in tiles])))
    B.check(lib.svt_hip_frame_batch_device(ctx, len(tiles), arr, arena.address, arena.cap, arena.table.data_ptr()))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    check_frames(arena, [w[0] for w in cases])


def test_chain_of_inter_pictures_without_host_round_trip(ctx):
    """tokeniser -> inter mode info -> bool coder -> frame, a SINGLE_REFERENCE and a REFERENCE_MODE_SELECT picture of 72x40 in one batch of
    every stage; the second packet ends in the four show-existing bytes of a packet flagged EB_BUFFERFLAG_SHOW_EXT"""
    cases = [w for w in FM.WHOLE if w[1] == "modes_inter"]
    pics = [IM.fixture_picture(w[2]) for w in cases]
    assert len({p["frame"]["reference_mode"] for p in pics}) == 2
    W, H = pics[0]["W"], pics[0]["H"]
    heads = [FM.host_header_bytes(w[3]) for w in cases]
    trailers = [b"", b"".join(FM.show_existing(s) for s in (0, 3, 7, 3))]
    ups = [upload(p["lf_mi"], p["qcoeff"], p["eob_map"]) for p in pics]
    grids = [GI.upload_grids(p) for p in pics]
    tbs, mbs = [TokBuffers(W, H, counts=False) for _ in pics], [GI.InterBuffers(W, H) for _ in pics]
    tiles = [GK.Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]
    arena, arr = frame_batch(ctx, tiles, heads, trailers)
    torch.cuda.synchronize()
    lib = B.load()
    tokenize_device(ctx, W, H, [(g[0], u[1], u[2]) for g, u in zip(grids, ups)], tbs)
    GI.modes_device(ctx, W, H, [(g, u[2], tb.tok_off, p["frame"]) for g, u, tb, p in zip(grids, ups, tbs, pics)], mbs)
    B.check(lib.svt_hip_boolcode_batch_device(ctx, len(tiles), (B.BoolStream * len(tiles))(*[t.struct for t in tiles])))
    B.check(lib.svt_hip_frame_batch_device(ctx, len(tiles), arr, arena.address, arena.cap, arena.table.data_ptr()))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    check_frames(arena, [w[0] for w in cases], trailers)


def test_entry_point_refusals(ctx):
    lib = B.load()
    batch = FM.make_batch(1, n_pics=2)
    src = torch.from_numpy(batch["source"]).cuda()
    size_t = torch.from_numpy(FM.sizes_array(batch).view(np.int32)).cuda()
    arena = Arena(ctx, 2, 20000)
    torch.cuda.synchronize()

    def call(n=2, arr=0, a=arena.address, t=arena.table.data_ptr(), c=ctx, **change):
        if arr == 0:
            arr = FM.packets(batch, src.data_ptr(), size_t.data_ptr())
            for k, v in change.items():
                setattr(arr[1], k, v)
        return lib.svt_hip_frame_batch_device(c, n, arr, a, arena.cap, t)
    assert call(n=0) == -1 and call(n=33) == -1 and call(c=None) == -1 and call(arr=None) == -1 and call(a=None) == -1 and call(t=None) == -1
    assert call(header_len=B.FRAME_HEADER_MAX + 1) == -1 and call(trailer_len=5) == -1 and call(d_tile_size=None) == -1 and call(d_tile=None) == -1
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    data, table, front, back, tguard = arena.result()
    assert np.all(data == FILL) and np.all(table == TABLE_FILL)      # nothing was launched
    assert call() == 0
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    want, want_table = FM.expected(batch)
    data, table, *_ = arena.result()
    assert bytes(data[:len(want)]) == want and np.array_equal(table, want_table)

"""GPU: the three-part assembly kernel (svt_fr_parts_kernel of csrc/frame.hip) through the C ABI, byte for byte against the host form
(svt_hip_frame_assemble_parts_host): the emulation's cases -- compressed headers of 1 .. 300 bytes, tiles of 2 .. 4 097, all 16 source and
destination phases of each part, short arenas -- with guard bytes round the arena and behind the table; a 32-picture batch with a picture
withheld for each reason; arena and table in pinned host memory; refusals that leave every fill untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_parts_model as PM
import svt_testlib as T
from test_gpu_frame import FILL, GUARD, TABLE_FILL, Arena

B = T.B
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib, c = B.load(), C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


class Launch:
    """a batch uploaded and its outputs allocated; run() enqueues one svt_hip_frame_parts_batch_device and synchronises"""

    def __init__(self, ctx, batch, capacity, pinned=False, pinned_table=False):
        self.ctx, self.batch, self.n = ctx, batch, len(batch["pics"])
        self.src = torch.from_numpy(batch["source"]).cuda()
        self.sizes = torch.from_numpy(PM.sizes_array(batch).view(np.int32)).cuda()
        self.arena = Arena(ctx, self.n, capacity, pinned)
        self.table_ptr, self.table_host = None, None
        if pinned_table:
            self.table_ptr = C.c_void_p()
            B.check(B.load().svt_hip_host_alloc(ctx, 8 * (self.n + 1) + 32, C.byref(self.table_ptr)))
            self.table_host = np.ctypeslib.as_array(C.cast(self.table_ptr, C.POINTER(C.c_uint32)), (2 * (self.n + 1) + 8,))
            self.table_host[:] = TABLE_FILL
        self.met = PM.phases(batch, self.src.data_ptr(), self.arena.address)
        torch.cuda.synchronize()

    def run(self):
        """(arena bytes, table, guards intact)"""
        try:
            arr = PM.packets(self.batch, self.src.data_ptr(), self.sizes.data_ptr())
            table = self.table_ptr.value if self.table_ptr else self.arena.table.data_ptr()
            B.check(B.load().svt_hip_frame_parts_batch_device(self.ctx, self.n, arr, self.arena.address, self.arena.cap, table))
            B.check(B.load().svt_hip_ctx_synchronize(self.ctx))
            data, table, front, back, tguard = self.arena.result()
            if self.table_ptr:
                t = self.table_host.copy()
                table, tguard = t[:2 * (self.n + 1)].reshape(-1, 2), t[2 * (self.n + 1):]
        finally:
            self.arena.free()
            if self.table_ptr:
                B.load().svt_hip_host_free(self.ctx, self.table_ptr)
        return data, table, bool(np.all(front == FILL) and np.all(back == FILL) and np.all(tguard == TABLE_FILL))


def check_against_host(ctx, batch, cap, launch=None, **kw):
    rc, want, want_table, ok = PM.assemble_host(batch, cap, fill=FILL)
    assert rc == 0 and ok
    data, table, intact = (launch or Launch(ctx, batch, cap, **kw)).run()
    assert intact and np.array_equal(table, want_table) and np.array_equal(data, want)


def test_the_emulations_cases_on_the_device_equal_the_host_form(ctx):
    cases = PM.emu_cases()
    launches = [Launch(ctx, b, cap) for b, cap in cases]
    comp, tile = set().union(*[x.met[0] for x in launches]), set().union(*[x.met[1] for x in launches])
    for part in (comp, tile):           # from the addresses the buffers really have
        assert {s for s, _ in part} == set(range(16)) and {d for _, d in part} == set(range(16))
    for (b, cap), x in zip(cases, launches):
        check_against_host(ctx, b, cap, launch=x)
    # and the host form is the concatenation (the CPU suite checks it at length)
    b = PM.standard_batches()[0]
    want, want_table = PM.expected(b)
    data, table, intact = Launch(ctx, b, len(want) + 40).run()
    assert intact and bytes(data[:len(want)]) == want and np.all(data[len(want):] == FILL) and np.array_equal(table, want_table)


def test_32_pictures_with_one_withheld_for_each_reason(ctx):
    batch = PM.with_failures(PM.standard_batches()[2], PM.REASONS)
    want, want_table = PM.expected(batch)
    assert int(want_table[32, 1]) == len(PM.REASONS) and all(int(want_table[3 + 4 * k, 1]) == B.FRAME_SIZE_NONE for k in range(len(PM.REASONS)))
    data, table, intact = Launch(ctx, batch, len(want) + 24).run()
    assert intact and np.array_equal(table, want_table) and bytes(data[:len(want)]) == want and np.all(data[len(want):] == FILL)


def test_arena_and_table_in_pinned_host_memory(ctx):
    b = PM.standard_batches()[3]
    total = len(PM.expected(b)[0])
    check_against_host(ctx, b, total + 40, pinned=True, pinned_table=True)
    check_against_host(ctx, b, total, pinned=True)


def test_refusals_leave_every_fill_untouched(ctx):
    lib = B.load()
    batch = PM.make_batch(1, n_pics=2)
    src = torch.from_numpy(batch["source"]).cuda()
    size_t = torch.from_numpy(PM.sizes_array(batch).view(np.int32)).cuda()
    arena = Arena(ctx, 2, 20000)
    torch.cuda.synchronize()

    def call(n=2, arr=0, a=arena.address, t=arena.table.data_ptr(), c=ctx, **change):
        if arr == 0:
            arr = PM.packets(batch, src.data_ptr(), size_t.data_ptr())
            for k, v in change.items():
                setattr(arr[1], k, v)
        return lib.svt_hip_frame_parts_batch_device(c, n, arr, a, arena.cap, t)
    hl = len(batch["pics"][1]["header"])
    assert call(n=0) == -1 and call(n=33) == -1 and call(c=None) == -1 and call(arr=None) == -1 and call(a=None) == -1 and call(t=None) == -1
    assert call(header_len=B.FRAME_UNCOMPRESSED_MAX + 1) == -1 and call(trailer_len=5) == -1 and call(size_bit=8 * hl - 15) == -1
    assert call(d_tile_size=None) == -1 and call(d_tile=None) == -1 and call(d_compressed_size=None) == -1 and call(d_compressed=None) == -1
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    data, table, front, back, tguard = arena.result()
    assert np.all(data == FILL) and np.all(table == TABLE_FILL)      # nothing was launched
    assert call() == 0
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    want, want_table = PM.expected(batch)
    data, table, front, back, tguard = arena.result()
    assert bytes(data[:len(want)]) == want and np.array_equal(table, want_table) and np.all(front == FILL) and np.all(back == FILL) and np.all(tguard == TABLE_FILL)

"""CPU: the bool coder's rules (csrc/boolcode_core.h in front of the serial writer of host/boolcode_host.c, through
svt_hip_boolcode_host) against an independent Python model (tests/boolcode_model.py: serial writer, the one-integer-sum form, the
kernels' chunked decomposition) and against the reference's own pack_mb_tokens / vpx_write (tests/golden/boolcode_reference.npz,
written by tests/gen_golden_boolcode.py).  Every comparison is byte-exact."""
import ctypes as C

import numpy as np
import pytest

import boolcode_model as BM
import svt_testlib as T

B = T.B
RAW = list(BM.raw_streams())


def test_abi_symbols_and_struct_sizes():
    lib = B.load()
    for s in ("svt_hip_boolcode_set_tables", "svt_hip_boolcode_batch_device", "svt_hip_boolcode", "svt_hip_boolcode_host", "svt_hip_boolcode_capacity",
              "svt_hip_boolcode_bools_capacity", "svt_hip_boolcode_geometry"):
        assert hasattr(lib, s) and s in B.EXPORTS, s
    assert B.BOOL_TABLES_DTYPE.itemsize == 3852 and B.BOOL_SEGMENT_DTYPE.itemsize == 12 and C.sizeof(B.BoolStream) == 64
    k, t = C.c_int32(), C.c_int32()
    lib.svt_hip_boolcode_geometry(C.byref(k), C.byref(t))
    assert k.value >= 8 and k.value % 8 == 0 and t.value >= 1
    # 7 bits a bool at most, the 33 framing bools, the marker byte; 22 bools a token at most
    assert lib.svt_hip_boolcode_bools_capacity(10) == 220 and lib.svt_hip_boolcode_capacity(0) >= (7 * 33 + 7) // 8 + 1
    for a in BM.raw_streams().values():
        assert len(BM.serial_write(a)) <= lib.svt_hip_boolcode_capacity(len(a))


def test_fixture_holds_what_the_tests_need():
    g = BM.fixture()
    assert g["coef_probs"].shape == (1728,) and g["pareto"].shape == (255, 8) and g["cat_probs"].shape == (6, 14)
    probs = g["coef_probs"].reshape(16, 6, 6, 3)       # band 0 has three contexts: its other rows are never addressed and stay 0
    assert probs[:, 0, :3].min() >= 1 and probs[:, 1:].min() >= 1 and not probs[:, 0, 3:].any() and g["pareto"].min() >= 1
    assert [int(np.count_nonzero(r)) for r in g["cat_probs"]] == [1, 2, 3, 4, 5, 14]
    assert list(g["token_records"]) == [11497, 13662, 3850] == [len(t) for t in BM.fixture_token_streams()]
    assert np.all(g["token_seconds"] > 0) and np.all(g["token_bools"] > g["token_records"])
    assert all(f"raw_bytes|{name}" in g for name in RAW)
    marker = [n for n in RAW if n.startswith("random_marker")]
    plain = [n for n in RAW if n.startswith("random_plain")]
    assert len(marker) >= 3 and len(plain) >= 3
    for n in marker:
        assert g[f"raw_bytes|{n}"][-1] == 0 and (g[f"raw_bytes|{n}"][-2] & 0xE0) == 0xC0
    for n in plain:
        st = {}
        BM.serial_write(BM.raw_streams()[n], st)
        assert not st["marker"]


@pytest.mark.parametrize("name", RAW)
def test_raw_stream_host_model_and_reference(name):
    a, want = BM.raw_streams()[name], bytes(BM.fixture()[f"raw_bytes|{name}"])
    got, size, guard = BM.host_code(bools=a, segments=[(0, len(a), 1)])
    assert got == want and size == len(want) and np.all(guard == 0xA5)
    assert BM.serial_write(a) == want
    assert BM.bigint_write(a) == want
    for K, tile in ((8, 2), (16, 4), (256, 256)):
        assert BM.chunked_write(a, K, tile) == want, (K, tile)


def test_straddle_streams_carry_through_long_runs():
    """(on the model) every straddle stream has a carry event; the n = 600 ones flip at least 40 bytes"""
    for name, a in BM.raw_streams().items():
        st = {}
        BM.serial_write(a, st)
        if name.startswith("straddle"):
            assert st["carry_events"] >= 1, name
            if name.startswith("straddle_600"):
                assert st["flipped"] >= 40, (name, st["flipped"])


def test_straddle_padding_shifts_the_stream():
    """(128, 0) bools in front leave range and low end alone: the construction is the same stream, pad bits later"""
    a, cross = BM.straddle_stream(200, 1)
    b, cross_b = BM.straddle_stream(200, 1, pad=37)
    assert b[37:] == a and cross_b == cross + 37 and b[:37] == [BM.rec(0, 128)] * 37
    st = {}
    BM.serial_write(b, st)
    assert st["carry_events"] == 1


@pytest.mark.parametrize("k", range(3))
def test_fixture_token_stream_host_model_and_reference(k):
    t, want = BM.fixture_token_streams()[k], bytes(BM.fixture()[f"token_bytes|{k}"])
    got, size, guard = BM.host_code(tokens=t)
    assert got == want and size == len(want) and np.all(guard == 0xA5)
    bools = BM.expand(t, None, None, BM.tables()[0])
    assert len(bools) == int(BM.fixture()["token_bools"][k])
    assert BM.serial_write(bools) == want and BM.bigint_write(bools) == want


def test_token_cases():
    """every token class with and without the skipped node, the categories' largest offsets (category 6: all 14 bits), both signs"""
    t, tabs = BM.token_cases(), BM.tables()[0]
    tok, row, extra = BM.unpack(t)
    skipped = {int(tok[i]) for i in range(1, len(t)) if tok[i - 1] == 0 and BM.band_of_row(int(row[i])) != 0}
    coded = {int(tok[i]) for i in range(len(t)) if i == 0 or tok[i - 1] != 0}
    assert skipped >= set(range(0, 11)) and coded >= set(range(0, 12))
    assert any(tok[i] == 10 and extra[i] >> 1 == 0x3FFF for i in range(len(t))) and any(extra[i] & 1 for i in range(len(t)))
    want = bytes(BM.fixture()["cases_bytes"])
    assert BM.host_code(tokens=t)[0] == want
    assert BM.serial_write(BM.expand(t, None, None, tabs)) == want
    # record by record: the host's expansion is the model's
    for i in range(len(t)):
        seg = [(i - 1, 2, 0)] if i and tok[i - 1] == 0 else [(i, 1, 0)]
        assert BM.host_code(tokens=t, segments=seg)[0] == BM.serial_write(BM.expand(t, None, seg, tabs)), i


def test_segments_restore_an_order_and_splice_bools():
    t, tabs = BM.fixture_token_streams()[2], BM.tables()[0]
    tok, _, _ = BM.unpack(t)
    ends = [i + 1 for i in range(len(t)) if tok[i] == BM.EOB_TOKEN][:40]     # cuts behind EOB tokens are block boundaries
    cuts = [0] + ends
    blocks = [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    n = ends[-1]
    want = BM.host_code(tokens=t[:n])[0]
    # the same blocks laid out in another order in the buffer, listed in coding order
    perm = np.random.default_rng(4).permutation(len(blocks))
    buf, where, pos = np.zeros(n, np.uint32), {}, 0
    for j in perm:
        a, c = blocks[j]
        buf[pos:pos + c] = t[a:a + c]
        where[j] = pos
        pos += c
    segs = [(where[j], blocks[j][1], 0) for j in range(len(blocks))]
    assert BM.host_code(tokens=buf, segments=segs)[0] == want
    assert BM.serial_write(BM.expand(buf, None, segs, tabs)) == want
    # raw bools between the blocks (an empty segment among them)
    raw = BM.raw_streams()["random_plain_0"]
    mixed = []
    for j, s in enumerate(segs):
        mixed += [s, (3 * j, j % 4, 1)]
    got = BM.host_code(tokens=buf, bools=raw, segments=mixed)[0]
    assert got == BM.serial_write(BM.expand(buf, raw, mixed, tabs)) and got != want


def test_capacity_guard_and_bad_arguments():
    a = BM.raw_streams()["straddle_600_0"]
    want = bytes(BM.fixture()["raw_bytes|straddle_600_0"])
    got, size, guard = BM.host_code(bools=a, segments=[(0, len(a), 1)], capacity=10)
    assert size == len(want) and got == want[:10] and np.all(guard == 0xA5)
    lib, tabs, size = B.load(), BM.tables()[1], C.c_uint32()
    seg = BM.segments_array([(0, len(a) + 1, 1)])
    out = np.zeros(64, np.uint8)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.svt_hip_boolcode_host(p(tabs), None, 0, p(a), len(a), p(seg), 1, p(out), 64, C.byref(size)) != 0          # segment past its buffer
    seg = BM.segments_array([(0, 1, 2)])
    assert lib.svt_hip_boolcode_host(p(tabs), None, 0, p(a), len(a), p(seg), 1, p(out), 64, C.byref(size)) != 0          # unknown kind
    assert lib.svt_hip_boolcode_host(p(tabs), None, 0, None, 0, None, 0, p(out), 64, None) != 0


def test_batch_entry_point_refuses_before_it_touches_a_device():
    """the refusals svt_hip_boolcode_batch_device makes on its arguments alone come before any use of the context"""
    lib = B.load()
    fake_ctx = C.create_string_buffer(1 << 20)      # never dereferenced before the stream checks; all-zero = no tables uploaded
    out, size = np.zeros(256, np.uint8), np.zeros(1, np.uint32)
    a = BM.raw_streams()["len9"]
    seg = BM.segments_array([(0, len(a), 1)])

    def stream(**kw):
        s = B.BoolStream()
        s.d_bools, s.d_segments, s.n_segments, s.max_bools = a.ctypes.data, seg.ctypes.data, 1, 64
        s.d_bytes, s.capacity, s.d_size = out.ctypes.data, 192, size.ctypes.data
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def rc(streams, n=None):
        arr = (B.BoolStream * len(streams))(*streams)
        return lib.svt_hip_boolcode_batch_device(fake_ctx, len(streams) if n is None else n, arr)
    assert rc([stream()] * (B.BOOL_MAX_STREAMS + 1)) != 0 and rc([stream()], 0) != 0 and lib.svt_hip_boolcode_batch_device(None, 1, None) != 0
    assert rc([stream(max_bools=(1 << 32) // 7 + 1 - 33)]) != 0          # 7 * (max_bools + 33) >= 2^32
    assert rc([stream(max_bools=(1 << 32) // 7 - 33), stream(d_size=None)]) != 0
    assert rc([stream(d_bytes=None)]) != 0 and rc([stream(d_segments=None)]) != 0 and rc([stream(d_segments=None, n_segments=0, n_tokens=4)]) != 0
    assert rc([stream()]) != 0 and b"set_tables" in lib.svt_hip_last_error()      # well-formed, but the context has no tables
    assert not out.any() and not size.any()


# ---- past one pass of the device's scans (the host form pinned by the model here; the device is compared with it in test_gpu_boolcode.py)
@pytest.mark.parametrize("n", BM.LONG_RAW)
def test_long_raw_streams_host_and_model(n):
    a = BM.long_raw_stream(n)
    assert len(a) == n
    got, size, guard = BM.host_code(bools=a, segments=[(0, n, 1)])
    assert got == BM.serial_write(a.tolist()) and size == len(got) and np.all(guard == 0xA5)


def test_long_straddle_carries_through_whole_tiles():
    """one carry event whose run of 0xff bytes covers two whole 1024-byte tiles of the device's carry scan"""
    a, (first, end) = BM.long_straddle()
    T_ = BM.CARRY_TILE_BYTES
    j = (first + T_ - 1) // T_
    assert T_ * (j + 2) <= end, (first, end)
    st = {}
    want = BM.serial_write(a.tolist(), st)
    assert st["carry_events"] == 1 and st["runs"] == [(first, end)]
    assert not any(want[first:end]) and want[first - 1] != 0           # the walk turned the whole run to zero bytes
    got, size, guard = BM.host_code(bools=a, segments=[(0, len(a), 1)])
    assert got == want and size == len(want) and np.all(guard == 0xA5)

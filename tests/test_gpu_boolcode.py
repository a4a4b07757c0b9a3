"""GPU: the bool coder (csrc/boolcode.hip) through the C ABI, byte for byte against the host form (svt_hip_boolcode_host) and the
reference's bytes (tests/golden/boolcode_reference.npz): chunk and tile boundaries, carries placed on them, contribution pile-up,
batches with the capacity guard, segment lists, the chain behind encode pass and tokeniser without a host round trip, scratch reuse;
and streams of more than 256 x 1024 items (a second pass of the tile scan) and a carry through whole tiles of the carry scan."""
import ctypes as C

import numpy as np
import pytest
import torch

import boolcode_model as BM
import modes_model as MM
import svt_testlib as T
import tokenize_model as TM
from test_gpu_encdec import dev, flags_of, make_inputs, md_host
from test_gpu_tokenize import KEY, TokBuffers, encode_batch, tokenize_device
import encdec_model as M
import gen_golden_tokens as G

B = T.B
pytestmark = pytest.mark.gpu
GUARD = 0x5A
CARRY_TILE_BYTES = BM.CARRY_TILE_BYTES      # svt_bc_carry_kernel walks the accumulator 256 32-bit words at a time


def geometry():
    k, t = C.c_int32(), C.c_int32()
    B.load().svt_hip_boolcode_geometry(C.byref(k), C.byref(t))
    return k.value, t.value


def new_ctx():
    c = C.c_void_p()
    B.check(B.load().svt_hip_ctx_create(C.byref(c), 0))
    B.check(B.load().svt_hip_boolcode_set_tables(c, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    B.load().svt_hip_ctx_destroy(c)


class Stream:
    """one stream of a batch: host arrays in, device buffers, the descriptor"""

    def __init__(self, tokens=None, bools=None, segments=None, capacity=None, max_bools=None, device_count=False, d_tokens=None):
        lib = B.load()
        self.tokens = np.zeros(0, np.uint32) if tokens is None else np.ascontiguousarray(tokens, np.uint32)
        self.bools = np.zeros(0, np.uint16) if bools is None else np.ascontiguousarray(bools, np.uint16)
        self.segments = segments
        worst = B.BOOL_MAX_PER_TOKEN * len(self.tokens) if segments is None else sum(c * (1 if k else B.BOOL_MAX_PER_TOKEN) for _, c, k in segments)
        self.max_bools = worst if max_bools is None else max_bools
        self.cap = int(lib.svt_hip_boolcode_capacity(self.max_bools)) if capacity is None else capacity
        self.keep = [dev(self.tokens.view(np.int32)) if d_tokens is None else d_tokens, dev(self.bools.view(np.int16)),
                     dev(BM.segments_array(segments).view(np.uint8)) if segments is not None else None,
                     torch.full((self.cap + 64,), GUARD, dtype=torch.uint8, device="cuda"), torch.full((1,), 0x77777777, dtype=torch.int32, device="cuda"),
                     dev(np.array([len(self.tokens)], np.int32)) if device_count else None]
        s = B.BoolStream()
        s.d_tokens, s.d_bools = self.keep[0].data_ptr(), self.keep[1].data_ptr()
        s.d_segments, s.n_segments = (self.keep[2].data_ptr(), len(segments)) if segments is not None else (None, 0)
        s.d_n_tokens, s.n_tokens = (self.keep[5].data_ptr(), 0) if device_count else (None, len(self.tokens))
        s.max_bools, s.capacity, s.d_bytes, s.d_size = self.max_bools, self.cap, self.keep[3].data_ptr(), self.keep[4].data_ptr()
        self.struct = s

    def result(self):
        raw, size = self.keep[3].cpu().numpy(), int(self.keep[4].cpu().numpy().view(np.uint32)[0])
        return bytes(raw[:min(size, self.cap)]), size, raw[self.cap:]

    def want(self):
        return BM.host_code(self.tokens, self.bools, self.segments)[0]


def run(ctx, streams):
    torch.cuda.synchronize()
    arr = (B.BoolStream * len(streams))(*[s.struct for s in streams])
    B.check(B.load().svt_hip_boolcode_batch_device(ctx, len(streams), arr))
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    return [s.result() for s in streams]


def check(ctx, streams, names=None):
    for i, (s, (got, size, guard)) in enumerate(zip(streams, run(ctx, streams))):
        want = s.want()
        assert size == len(want) and got == want and np.all(guard == GUARD), names[i] if names else i


def raw(bools, **kw):
    return Stream(bools=bools, segments=[(0, len(bools), 1)], **kw)


def test_chunk_and_tile_boundaries(ctx):
    """n bools at the chunk size K and the chain tile T * K; and n + 33 symbols (the framing bools count) at the same places"""
    K, Tc = geometry()
    ns = [0, 1, K - 1, K, K + 1, Tc * K - 1, Tc * K, Tc * K + 1, 3 * Tc * K + 7, K - 34, K - 33, K - 32, Tc * K - 34, Tc * K - 33, Tc * K - 32]
    check(ctx, [raw(BM.random_stream(100 + i, n)) for i, n in enumerate(ns)], ns)


def test_raw_fixture_streams_equal_the_reference(ctx):
    names = list(BM.raw_streams())
    streams = [raw(BM.raw_streams()[n]) for n in names]
    for n, (got, size, guard) in zip(names, run(ctx, streams)):
        want = bytes(BM.fixture()[f"raw_bytes|{n}"])
        assert got == want and size == len(want) and np.all(guard == GUARD), n


def test_straddle_streams_placed_on_boundaries(ctx):
    K, _ = geometry()
    streams, names = [], []
    for seed in range(2):
        _, cross = BM.straddle_stream(200, seed)
        for at in (K - 1, 0):           # the crossing bool is symbol 1 + pad + cross: last / first of a chunk
            pad = (at - 1 - cross) % K
            s, c = BM.straddle_stream(200, seed, pad)
            assert (1 + c) % K == at
            streams.append(raw(s)); names.append((seed, at))
    # an n = 600 stream whose run of 0xff bytes lies across a 32-bit word boundary and an accumulator tile boundary
    st = {}
    BM.serial_write(BM.straddle_stream(600, 0)[0], st)
    a, b = st["runs"][0]
    pad = 8 * (CARRY_TILE_BYTES - (a + b) // 2)
    s, _ = BM.straddle_stream(600, 0, pad)
    BM.serial_write(s, st)
    a, b = st["runs"][0]
    assert st["carry_events"] == 1 and a + 4 < CARRY_TILE_BYTES < b - 4 and b - a >= 40
    streams.append(raw(s)); names.append("tile")
    check(ctx, streams, names)


def test_contribution_pile_up(ctx):
    """behind 300 (255, 0) bools, runs of 1-bools that do not move the bit position: up to 127 contributions on one position"""
    head = [BM.rec(0, 255)] * 300
    check(ctx, [raw(head + [BM.rec(1, 1)] * 300), raw(head + [BM.rec(1, 255)] * 300), raw([BM.rec(1, 1)] * 127 + [BM.rec(1, 255)] * 4 + [BM.rec(1, 1)] * 127)])


def test_batch_with_an_empty_stream_a_short_buffer_and_a_short_scratch(ctx):
    lens = (700, 0, 5000, 33, 1800)
    bools = [BM.random_stream(200 + i, n) for i, n in enumerate(lens)]
    full = [BM.host_code(bools=np.array(b, np.uint16), segments=[(0, len(b), 1)])[0] for b in bools]
    streams = [raw(bools[0]), raw(bools[1]), raw(bools[2], capacity=len(full[2]) - 9), raw(bools[3]), raw(bools[4])]
    res = run(ctx, streams)
    for i in (0, 1, 3, 4):
        assert res[i][0] == full[i] and res[i][1] == len(full[i]) and np.all(res[i][2] == GUARD), i
    got, size, guard = res[2]       # the size is reported, the guard bytes behind the buffer are intact
    assert size == len(full[2]) and got == full[2][:-9] and np.all(guard == GUARD) and len(guard) == 64
    # scratch sized for fewer bools than the stream has: not coded, and said so
    streams = [raw(bools[0]), raw(bools[2], max_bools=len(bools[2]) - 1, capacity=4096), raw(bools[4])]
    res = run(ctx, streams)
    assert res[1][1] == B.BOOL_SIZE_OVERFLOW and np.all(res[1][2] == GUARD)
    assert res[0][0] == full[0] and res[2][0] == full[4]


def test_fixture_token_streams_equal_the_reference(ctx):
    toks = BM.fixture_token_streams()
    streams = [Stream(tokens=toks[0]), Stream(tokens=toks[1], device_count=True), Stream(tokens=toks[2]), Stream(tokens=BM.token_cases())]
    want = [bytes(BM.fixture()[f"token_bytes|{k}"]) for k in range(3)] + [bytes(BM.fixture()["cases_bytes"])]
    for k, (got, size, guard) in enumerate(run(ctx, streams)):
        assert got == want[k] and size == len(want[k]) and np.all(guard == GUARD), k


def block_cuts(t):
    """(first, count) of runs of records that end behind an EOB token: block boundaries"""
    tok, _, _ = BM.unpack(t)
    cuts = [0] + [i + 1 for i in range(len(t)) if tok[i] == BM.EOB_TOKEN]
    if cuts[-1] != len(t):
        cuts.append(len(t))
    return [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]


def test_segment_permutations_and_spliced_bools(ctx):
    streams, want = [], []
    for k, t in enumerate(BM.fixture_token_streams()):
        blocks = block_cuts(t)
        perm = np.random.default_rng(k).permutation(len(blocks))
        buf, where, pos = np.zeros(len(t), np.uint32), {}, 0
        for j in perm:
            a, c = blocks[j]
            buf[pos:pos + c] = t[a:a + c]
            where[j] = pos
            pos += c
        segs = [(where[j], blocks[j][1], 0) for j in range(len(blocks))]
        streams.append(Stream(tokens=buf, segments=segs))
        want.append(bytes(BM.fixture()[f"token_bytes|{k}"]))
    bools = BM.raw_streams()["random_plain_0"]
    mixed = []
    for j, s in enumerate(streams[2].segments):
        mixed += [s, ((7 * j) % 150, j % 5, 1)]
    streams.append(Stream(tokens=streams[2].tokens, bools=bools, segments=mixed))
    want.append(streams[-1].want())
    assert want[-1] != want[2]
    for k, (got, size, guard) in enumerate(run(ctx, streams)):
        assert got == want[k] and size == len(want[k]) and np.all(guard == GUARD), k


def enqueue_intra(ctx, W, H, src, lf, q_index, keep):
    """svt_hip_encdec_intra_device on a given grid, enqueued only: (lf_t, q_t, emap_t, work); the device buffers go to `keep`"""
    lib = B.load()
    srcb = dev(np.concatenate([p.ravel() for p in src]))
    nco, n_sb = T.n_sb(W, H) * B.SB_COEFFS, T.n_sb(W, H)
    q_t, dq_t = torch.zeros(nco, dtype=torch.int16, device="cuda"), torch.zeros(nco, dtype=torch.int16, device="cuda")
    rec = M.RefPic(W, H)
    rec_t = dev(rec.buf)
    lf_t = dev(np.ascontiguousarray(lf).view(np.uint8))
    emap_t = torch.full((M.eob_map_offsets(W, H)[3],), 77, dtype=torch.int16, device="cuda")
    lfm_t, nz_t = torch.zeros(n_sb * 160, dtype=torch.uint8, device="cuda"), torch.full((lf.size,), 7, dtype=torch.uint8, device="cuda")
    keep += [srcb, q_t, dq_t, rec_t, lf_t, emap_t, lfm_t, nz_t]
    d = B.YuvPlanes()
    d.y, d.u, d.v = srcb.data_ptr(), srcb.data_ptr() + W * H, srcb.data_ptr() + W * H + (W // 2) * (H // 2)
    d.y_stride, d.uv_stride, d.width, d.height = W, W // 2, W, H
    p = B.EncdecPicture()
    p.d_lf_mi, p.src, p.recon = lf_t.data_ptr(), d, rec.desc(rec_t.data_ptr())
    p.d_qcoeff, p.d_dqcoeff, p.d_eob_map, p.d_lfm, p.d_nz = q_t.data_ptr(), dq_t.data_ptr(), emap_t.data_ptr(), lfm_t.data_ptr(), nz_t.data_ptr()
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, 1, W, H, C.byref(work)))
    torch.cuda.synchronize()
    B.check(lib.svt_hip_encdec_intra_device(ctx, work, C.byref(p), W, H, W // 8, q_index, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
    return lf_t, q_t, emap_t, work


@pytest.mark.parametrize("k", (0, 1, 2))
def test_chain_behind_encode_pass_and_tokeniser(ctx, k):
    """encode pass -> tokeniser -> bool coder on one context, nothing waited for in between, on each of the fixture pictures (inter,
    intra with 4x4 blocks, mixed); the segment list restores the entropy coder's block order from the tokeniser's offsets"""
    lib = B.load()
    W, H, pics = TM.fixture_pictures()
    pic = pics[k]
    kind, seed, q_index, lam = G.PICTURES[k]
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    # the offsets the tokeniser will produce follow from the eob map alone: the host form gives them before anything runs
    host = TM.host_tokenize_picture(pic["lf_mi"], pic["qcoeff"], pic["eob_map"], W, H)
    w4, h4 = W // 4, H // 4
    eoff = (0, w4 * h4, w4 * h4 + (w4 // 2) * (h4 // 2))
    segs = [(int(host["tok_off"][eoff[p] + y4 * (w4 // 2 if p else w4) + x4]), int(n), 0) for p, x4, y4, n in pic["blocks"]]
    assert segs != sorted(segs)        # the entropy coder's order is not the buffer's order
    # every output buffer exists (and torch's fills of them are waited for) before the first launch on the context's stream
    tb = TokBuffers(W, H)
    s = Stream(tokens=np.zeros(1, np.uint32), segments=segs, d_tokens=tb.tokens)
    keep = []
    if kind == "intra":
        frames = T.gen_clip_subpel(W, H, 3, seed)
        lf = M.gen_intra_grid(seed, W, H, sizes=(4, 8, 16, 32), filter_level=level)
        lf_t, q_t, emap_t, work = enqueue_intra(ctx, W, H, (frames[1],) + G._chroma(frames[1], 1), lf, q_index, keep)
    else:
        srcs, refs, me = make_inputs(W, H, 1, seed)
        mc, lf = md_host(me[0], W, H, lam, level)
        if kind == "mixed":
            lf, mc, _ = M.make_mixed(seed, lf, mc, share=0.35, level=level)
        dp, work, keep = encode_batch(ctx, W, H, srcs, refs, [(mc, lf)], q_index, has_intra=int(kind == "mixed"))
        lf_t, q_t, emap_t = dp[0].lf_t, dp[0].q_t, dp[0].emap_t
    try:
        tokenize_device(ctx, W, H, [(lf_t, q_t, emap_t)], [tb])
        arr = (B.BoolStream * 1)(s.struct)
        B.check(lib.svt_hip_boolcode_batch_device(ctx, 1, arr))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
        got_tok = tb.result()
        assert np.array_equal(got_tok["tok_off"], host["tok_off"]) and np.array_equal(got_tok["tokens"], host["tokens"])
        got, size, guard = s.result()
        want = bytes(BM.fixture()[f"token_bytes|{k}"])
        assert got == want and size == len(want) and np.all(guard == GUARD)
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)


def test_entry_point_refusals(ctx):
    lib = B.load()
    ok = raw(BM.random_stream(1, 50))

    def rc(streams, n=None):
        arr = (B.BoolStream * len(streams))(*streams)
        return lib.svt_hip_boolcode_batch_device(ctx, len(streams) if n is None else n, arr)
    assert rc([ok.struct]) == 0
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert rc([ok.struct] * (B.BOOL_MAX_STREAMS + 1)) != 0 and rc([ok.struct], 0) != 0
    for field, value in (("max_bools", (1 << 32) // 7 + 1 - 33), ("d_size", None), ("d_bytes", None)):
        s = raw(BM.random_stream(1, 50)).struct
        setattr(s, field, value)
        assert rc([s]) != 0, field
    # what only the device can see: a segment whose buffer the stream does not have, a segment of an unknown kind
    bad = [raw(BM.random_stream(1, 50)), Stream(tokens=BM.token_cases(), segments=[(0, 5, 0)]), Stream(tokens=BM.token_cases(), segments=[(0, 5, 0), (0, 1, 2)])]
    bad[0].struct.d_bools, bad[1].struct.d_tokens = None, None
    good = raw(BM.random_stream(2, 300))
    res = run(ctx, bad + [good])
    assert [r[1] for r in res[:3]] == [B.BOOL_SIZE_OVERFLOW] * 3 and all(np.all(r[2] == GUARD) for r in res)
    assert res[3][0] == good.want()


def test_context_reuse_longer_shorter_longer(ctx):
    c = new_ctx()
    try:
        for i, n in enumerate((3000, 40000, 500, 90000)):
            check(c, [raw(BM.random_stream(300 + i, n))], [n])
    finally:
        B.load().svt_hip_ctx_destroy(c)


def test_host_pointer_form(ctx):
    t = BM.fixture_token_streams()[2]
    got, size, guard = BM.product_call(B.load().svt_hip_boolcode, tokens=t, ctx=ctx)
    want = bytes(BM.fixture()["token_bytes|2"])
    assert got == want and size == len(want) and np.all(guard == 0xA5)
    a = BM.raw_streams()["straddle_600_1"]
    got, size, guard = BM.product_call(B.load().svt_hip_boolcode, bools=a, segments=[(0, len(a), 1)], capacity=20, ctx=ctx)
    want = bytes(BM.fixture()["raw_bytes|straddle_600_1"])
    assert got == want[:20] and size == len(want) and np.all(guard == 0xA5)


# ---- past one pass of the scans ------------------------------------------------------------------------------------------------
def test_long_raw_streams_in_one_batch(ctx):
    """n bools around 256 tiles of 1024 items, and two passes + 5: the sum the tile scan carries from pass to pass"""
    check(ctx, [raw(BM.long_raw_stream(n)) for n in BM.LONG_RAW], BM.LONG_RAW)


def test_carry_through_whole_tiles_of_the_carry_scan(ctx):
    """one carry through about 3550 bytes of 0xff: tiles of 256 words that generate nothing and only hand the carry on; then the same stream
    moved so that the carry starts in the next tile"""
    a, (first, end) = BM.long_straddle()
    j = (first + CARRY_TILE_BYTES - 1) // CARRY_TILE_BYTES
    assert CARRY_TILE_BYTES * (j + 2) <= end
    tile = end // CARRY_TILE_BYTES
    pad = 8 * ((tile + 1) * CARRY_TILE_BYTES + 100 - end)
    b, (first_b, end_b) = BM.long_straddle(pad)
    assert end_b // CARRY_TILE_BYTES == tile + 1 and end_b - first_b == end - first
    check(ctx, [raw(a), raw(b)], ("straddle", "padded"))


def test_big_picture_tokens_and_segments(ctx):
    """the all-4x4 1080x1080 picture's tokens, bools and segment list (289 x 256 slots, empty ones among them) from host arrays: 821 785 items"""
    h = MM.big_host("big_4x4")
    tok, bools, segs = h["tok"]["tokens"], h["modes"]["bools"], h["segs"]
    assert len(segs) == 289 * 256 and sum(c for _, c, _ in segs) == len(tok) + len(bools) > 3 * 256 * 1024 and sum(1 for s in segs if s[1] == 0) > 20000
    s = Stream(tokens=tok, bools=bools, segments=segs)
    got, size, guard = run(ctx, [s])[0]
    assert size == len(h["tile"]) and got == h["tile"] and np.all(guard == GUARD)

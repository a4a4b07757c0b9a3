"""GPU: the forward coefficient-probability update (csrc/coef_update.hip) through the C ABI, byte for byte against the host form
(svt_hip_coef_update_picture): the count kernel at its pass and grid-stride boundaries, 32 pictures of unlike lengths whose totals only
the device knows, a 32-bit bin, ZERO runs across every band; the decide and join kernels on every case of the reference fixture and
on 32 seeded pictures with unlike "old" tables, guards behind every buffer; the bool coder with coefficient tables per stream; the
chain tokeniser -> stage -> bool coder on one stream; refusals that launch nothing.  The inputs are token streams built directly."""
import ctypes as C

import numpy as np
import pytest
import torch

import boolcode_model as BM
import coef_update_model as CM
import frame_model as FM
import svt_testlib as T
from test_gpu_boolcode import GUARD, Stream, new_ctx

B = T.B
pytestmark = pytest.mark.gpu
DEFAULT = BM.tables()[0]["coef_probs"].reshape(-1)
FILL16, FILL32, FILL8 = 0x5A5A, 0x5A5A5A5A, 0x5A
PAD = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_base = {}


def base_stream(mix="default", n=9000):
    """a seeded stream per token mix, generated once; the tests take slices and tilings of it (a slice may end inside a block: both forms
    scan whatever records they are given)"""
    if mix not in _base:
        _base[mix] = CM.seeded_stream(40 + len(_base), 9000, mix=mix)
    t = _base[mix]
    return t[:n] if n <= len(t) else np.tile(t, n // len(t) + 1)[:n]


def geometry():
    a, b = C.c_int32(), C.c_int32()
    B.load().svt_hip_coef_update_geometry(C.byref(a), C.byref(b))
    return a.value, b.value


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    B.load().svt_hip_ctx_destroy(c)


class Picture:
    """one picture of a batch: host arrays in, every output between guards, the descriptor"""

    def __init__(self, tokens, counts=None, old=None, prefix=(), suffix=(), device_count=False, max_tokens=None):
        self.tokens = np.ascontiguousarray(tokens, np.uint32)
        self.counts = CM.counts_of(self.tokens) if counts is None else np.ascontiguousarray(counts, np.uint32)
        self.old, self.prefix, self.suffix, self.device_count = old, tuple(prefix), tuple(suffix), device_count
        self.max_tokens = len(self.tokens) if max_tokens is None else max_tokens
        self.cap = int(B.load().svt_hip_coef_update_bools_capacity())
        i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device="cuda")      # noqa: E731
        self.keep = dict(tok=dev(self.tokens.view(np.int32)) if len(self.tokens) else None, n_tok=dev(np.array([len(self.tokens)], np.int32)),
                         counts=dev(self.counts.view(np.int32)), old=dev(np.ascontiguousarray(old, np.uint8)) if old is not None else None,
                         eob=i32(576 + PAD, FILL32), probs=torch.full((1728 + PAD,), FILL8, dtype=torch.uint8, device="cuda"),
                         bools=torch.full((self.cap + PAD,), FILL16, dtype=torch.int16, device="cuda"), n=i32(1 + PAD, FILL32), seg=i32(3 + PAD, FILL32),
                         res=i32(18 + PAD, FILL32))
        k = self.keep
        p = B.CuPicture()
        p.d_tokens = k["tok"].data_ptr() if k["tok"] is not None else None
        p.d_n_tokens, p.n_tokens = (k["n_tok"].data_ptr(), 0) if device_count else (None, len(self.tokens))
        p.max_tokens, p.d_counts, p.d_old_probs = self.max_tokens, k["counts"].data_ptr(), k["old"].data_ptr() if old is not None else None
        p.d_eob_branch, p.d_probs, p.d_hdr_bools, p.d_n_hdr_bools = k["eob"].data_ptr(), k["probs"].data_ptr(), k["bools"].data_ptr(), k["n"].data_ptr()
        p.d_segment, p.d_result = k["seg"].data_ptr(), k["res"].data_ptr()
        p.n_prefix, p.n_suffix = len(self.prefix), len(self.suffix)
        for i, v in enumerate(self.prefix):
            p.prefix[i] = v
        for i, v in enumerate(self.suffix):
            p.suffix[i] = v
        self.struct = p

    def result(self):
        k = {n: t.cpu().numpy() for n, t in self.keep.items() if t is not None and n in ("eob", "probs", "bools", "n", "seg", "res")}
        n = int(k["n"].view(np.uint32)[0])
        bools = k["bools"].view(np.uint16)
        untouched = (np.all(k["eob"].view(np.uint32)[576:] == FILL32) and np.all(k["probs"][1728:] == FILL8) and np.all(bools[min(n, self.cap):] == FILL16) and
                     np.all(k["n"].view(np.uint32)[1:] == FILL32) and np.all(k["seg"].view(np.uint32)[3:] == FILL32) and np.all(k["res"].view(np.uint32)[18:] == FILL32))
        return dict(eob=k["eob"].view(np.uint32)[:576], probs=k["probs"][:1728], bools=bools[:min(n, self.cap)], n=n, segment=tuple(int(v) for v in k["seg"].view(np.uint32)[:3]),
                    result=k["res"][:18].view(B.CU_RESULT_DTYPE)[0], untouched=bool(untouched), raw=k)

    def want(self):
        return CM.host_picture(self.tokens, self.counts, old_probs=self.old, prefix=self.prefix, suffix=self.suffix, device_count=self.device_count, max_tokens=self.max_tokens)


def run(ctx, pics):
    torch.cuda.synchronize()
    arr = (B.CuPicture * len(pics))(*[p.struct for p in pics])
    B.check(B.load().svt_hip_coef_update_batch_device(ctx, len(pics), arr))
    B.check(B.load().svt_hip_ctx_synchronize(ctx))
    return [p.result() for p in pics]


def check(ctx, pics, names=None):
    for i, (p, got) in enumerate(zip(pics, run(ctx, pics))):
        what, want = names[i] if names else i, p.want()
        assert got["untouched"], what
        assert np.array_equal(got["eob"], want["eob"]), what
        assert got["n"] == want["n"] and np.array_equal(got["bools"], want["bools"]) and got["segment"] == want["segment"], what
        assert np.array_equal(got["probs"], want["probs"]) and got["result"].tobytes() == want["result"].tobytes(), what


# ---- the count kernel --------------------------------------------------------------------------------------------------------------
def test_stream_lengths_on_the_pass_and_grid_stride_boundaries(ctx):
    per_pass, wgs = geometry()
    ns = [0, 1, per_pass - 1, per_pass, per_pass + 1, per_pass * wgs - 1, per_pass * wgs, per_pass * wgs + 1, 2 * per_pass * wgs + 1]
    long = base_stream("zeros", max(ns))
    check(ctx, [Picture(long[:n], device_count=bool(i & 1)) for i, n in enumerate(ns)], ns)


def test_32_pictures_of_unlike_lengths_with_totals_on_the_device(ctx):
    rng = np.random.default_rng(51)
    lens = [0, 3] + [int(v) for v in rng.integers(5, 9000, 30)]
    base = base_stream()
    pics = [Picture(base[:n] if i & 1 else base_stream("ones")[i:i + n], device_count=True) for i, n in enumerate(lens)]
    check(ctx, pics, lens)
    # a total above max_tokens: the records beyond are not read
    pics = [Picture(base, device_count=True, max_tokens=1000), Picture(base, device_count=False, max_tokens=5000)]
    got = run(ctx, pics)
    assert np.array_equal(got[0]["eob"], CM.eob_branch(base[:1000])) and np.array_equal(got[1]["eob"], CM.eob_branch(base[:5000]))
    assert got[0]["result"]["tokens"] == 1000 and got[1]["result"]["tokens"] == 5000


def test_70000_records_in_one_row_and_zero_runs_across_every_band(ctx):
    row = ((2 * 2 + 1) * 2 + 0) * 36 + 0 * 6 + 1            # 16x16, chroma, intra, band 0, context 1
    one_row = np.full(70000, row << 4 | 3, np.uint32)
    # ZERO runs: in every band but 0 the record behind a ZERO leaves node 0 out; ZERO ZERO ... across all six bands, ended by ONE
    runs = []
    for grp in range(16):
        for band in range(6):
            for ctx6 in range(3 if band == 0 else 6):
                r = (grp * 6 + band) * 6 + ctx6
                runs += [r << 4 | 0, r << 4 | 0, r << 4 | 1, r << 4 | 11 if band else r << 4 | 1]
    runs = np.array(runs * 9, np.uint32)
    got = run(ctx, [Picture(one_row), Picture(runs)])
    assert got[0]["eob"][row] == 70000 and got[0]["eob"].sum() == 70000
    want = CM.eob_branch(runs)
    assert np.array_equal(got[1]["eob"], want) and 0 < want.sum() < len(runs)
    check(ctx, [Picture(one_row), Picture(runs)], ("one row", "zero runs"))


# ---- the decide and join kernels ---------------------------------------------------------------------------------------------------
def test_every_fixture_case_equals_the_host_form_and_the_reference(ctx):
    g = CM.fixture()
    names = [str(n) for n in g["names"]]
    pics = []
    for n in names:
        fr = [int(v) for v in g[f"frame|{n}"]]
        fp = FM.inter(reference_mode=fr[1], allow_comp_inter_inter=fr[2], allow_hp=fr[3]) if fr[0] else FM.params()
        pre, suf = CM.header_parts(fp)
        pics.append(Picture(g[f"tokens|{n}"], old=g.get(f"old|{n}"), prefix=pre, suffix=suf))
    check(ctx, pics, names)
    for n, got in zip(names, run(ctx, pics)):
        assert np.array_equal(got["probs"], g[f"probs|{n}"]), n
        assert BM.host_code(bools=got["bools"], segments=[(0, got["n"], 1)])[0] == bytes(g[f"bytes|{n}"]), n


def test_32_seeded_pictures_with_unlike_old_tables(ctx):
    pics = []
    for i in range(32):
        tok = base_stream(("default", "zeros", "large", "ones")[(i // 4) % 4])[13 * i:][:(700, 4000, 8500, 40)[i % 4]]
        old = None if i % 5 == 0 else CM.seeded_probs(300 + i, ends=bool(i % 3 == 0))
        pics.append(Picture(tok, old=old, prefix=(CM.rec(1, 128),) * (i % (B.CU_PREFIX_MAX + 1)), suffix=(CM.rec(0, 252),) * ((7 * i) % (B.CU_SUFFIX_MAX + 1)),
                            device_count=bool(i & 1)))
    check(ctx, pics)
    got = run(ctx, pics)
    assert any(sum(r["result"]["sent"]) == 4 for r in got) and any(sum(r["result"]["sent"]) == 0 for r in got)
    # counts that are not the stream's own (seeded counts, eob_branch from the stream): the two inputs are independent
    c, _ = CM.seeded_counts(9, 3000, "large")
    check(ctx, [Picture(base_stream("large", 6000), counts=c)])


def test_sums_beyond_32_bits(ctx):
    row = ((1 * 2 + 0) * 2 + 1) * 36 + 1 * 6 + 2
    tok = np.concatenate([np.full(1 << 20, row << 4 | 1, np.uint32), CM.seeded_stream(11, 4000, groups=(4, 5, 6, 7))])
    old = DEFAULT.copy()
    old[3 * row + 1] = 255
    p = Picture(tok, old=old)
    check(ctx, [p])
    assert max(p.want()["result"]["savings"]) >= 2 ** 31


# ---- the bool coder with tables per stream -----------------------------------------------------------------------------------------
def test_bool_coder_with_tables_per_stream(ctx):
    lib = B.load()
    streams, tabs, keep = [], [], []
    for i in range(32):
        streams.append(Stream(tokens=base_stream(("default", "large")[i % 2])[31 * i:][:(300, 2500, 1, 1100)[i % 4]], device_count=bool(i & 1)))
        tabs.append(None if i % 3 == 0 else CM.seeded_probs(600 + i, ends=bool(i & 2)))
        keep.append(dev(tabs[-1]) if tabs[-1] is not None else None)
    ptrs = (C.c_void_p * 32)(*[k.data_ptr() if k is not None else None for k in keep])
    arr = (B.BoolStream * 32)(*[s.struct for s in streams])
    torch.cuda.synchronize()
    B.check(lib.svt_hip_boolcode_batch_tables_device(ctx, 32, arr, ptrs))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    differ = 0
    for i, (s, t) in enumerate(zip(streams, tabs)):
        got, size, guard = s.result()
        want = BM.product_call(lib.svt_hip_boolcode_host, tokens=s.tokens, tabs=CM.tables_with(DEFAULT if t is None else t))[0]
        assert got == want and size == len(want) and np.all(guard == GUARD), i
        differ += want != s.want()
    assert differ >= 16
    # a NULL array is the context's table for every stream; and the old entry's bytes are what they were
    fresh = [Stream(tokens=s.tokens, device_count=s.struct.d_n_tokens is not None) for s in streams[:8]]
    arr = (B.BoolStream * 8)(*[s.struct for s in fresh])
    torch.cuda.synchronize()
    B.check(lib.svt_hip_boolcode_batch_tables_device(ctx, 8, arr, None))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert all(s.result()[0] == s.want() for s in fresh)
    again = [Stream(tokens=s.tokens) for s in streams[:8]]
    arr = (B.BoolStream * 8)(*[s.struct for s in again])
    torch.cuda.synchronize()
    B.check(lib.svt_hip_boolcode_batch_device(ctx, 8, arr))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert all(s.result()[0] == s.want() and np.all(s.result()[2] == GUARD) for s in again)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def test_chain_stage_then_bool_coder_on_one_stream_equals_the_host_chain(ctx):
    """tokens and counts on the device -> the stage -> the bool coder codes the tile under d_probs and the header from d_hdr_bools, nothing
    waited for in between; the bytes are the all-host chain's (tests/coef_update_model.py:host_frame), which the CPU suite reads back"""
    lib = B.load()
    cases = CM.real_pictures()
    pics, tiles, hdrs, want = [], [], [], []
    for name, kind, pic, fp in cases:
        s = CM.host_stream(kind, pic)
        pre, suf = CM.header_parts(fp)
        p = Picture(s["tokens"], counts=s["counts"], prefix=pre, suffix=suf, device_count=True)
        pics.append(p)
        tiles.append(Stream(tokens=s["tokens"], bools=s["bools"], segments=s["segments"]))
        h = Stream(bools=np.zeros(1, np.uint16), segments=[(0, 1, 1)], max_bools=p.cap)
        h.struct.d_bools, h.struct.d_segments = p.keep["bools"].data_ptr(), p.keep["seg"].data_ptr()
        hdrs.append(h)
        want.append(CM.host_frame(kind, pic, fp, update=True))
    n = len(pics)
    torch.cuda.synchronize()
    B.check(lib.svt_hip_coef_update_batch_device(ctx, n, (B.CuPicture * n)(*[p.struct for p in pics])))
    ptrs = (C.c_void_p * (2 * n))(*([p.keep["probs"].data_ptr() for p in pics] + [None] * n))
    B.check(lib.svt_hip_boolcode_batch_tables_device(ctx, 2 * n, (B.BoolStream * (2 * n))(*[s.struct for s in tiles + hdrs]), ptrs))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    for (name, kind, pic, fp), p, t, h, w in zip(cases, pics, tiles, hdrs, want):
        got = p.result()
        assert got["untouched"] and np.array_equal(got["probs"], w["probs"]), name
        tile, size, guard = t.result()
        assert tile == w["tile"] and size == len(w["tile"]) and np.all(guard == GUARD), name
        comp, csize, guard = h.result()
        rc, hdr, ub, cb, _ = CM.header_coef(fp, got["bools"])           # the host header from the device's records
        assert rc == 0 and hdr == w["header"] and comp == hdr[ub:] and csize == cb and np.all(guard == GUARD), name
        assert hdr + tile == w["frame"] == bytes(CM.fixture()[f"frame_with|{name}"]), name


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_every_fill(ctx):
    lib = B.load()
    tok = base_stream(n=3000)

    def rc(p, n=1, c=None):
        arr = (B.CuPicture * max(n, 1))(*([p.struct] * max(n, 1)))
        return lib.svt_hip_coef_update_batch_device(ctx if c is None else c, n, arr)
    p = Picture(tok)
    torch.cuda.synchronize()
    assert rc(p, 0) != 0 and rc(p, B.CU_MAX_PICS + 1) != 0 and lib.svt_hip_coef_update_batch_device(ctx, 1, None) != 0
    assert lib.svt_hip_coef_update_batch_device(None, 1, (B.CuPicture * 1)(p.struct)) != 0
    for field in ("d_counts", "d_eob_branch", "d_probs", "d_hdr_bools", "d_n_hdr_bools", "d_segment", "d_result", "d_tokens"):
        q = Picture(tok)
        setattr(q.struct, field, None)
        assert rc(q) != 0, field
    for field, v in (("n_prefix", B.CU_PREFIX_MAX + 1), ("n_suffix", B.CU_SUFFIX_MAX + 1)):
        setattr(p.struct, field, v)
        assert rc(p) != 0, field
        setattr(p.struct, field, 0)
    bare = C.c_void_p()                       # a context whose tables were never set
    B.check(lib.svt_hip_ctx_create(C.byref(bare), 0))
    try:
        assert rc(p, 1, bare) != 0
        B.check(lib.svt_hip_ctx_synchronize(bare))
    finally:
        lib.svt_hip_ctx_destroy(bare)
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    raw = p.result()["raw"]
    assert all(np.all(raw[k].view(np.uint8) == FILL8) for k in ("eob", "probs", "bools", "n", "seg", "res"))
    check(ctx, [p])


def test_chain_behind_the_real_encode_pass_key_and_inter_pictures(ctx):
    """136 x 72 at q index 40: a key picture through svt_hip_encdec_intra_device and two inter pictures through svt_hip_md_default_batch_device
    and svt_hip_encdec_batch_device; then tokeniser (with counts) -> labelling / mode info -> the stage -> the bool coder under every
    picture's d_probs (tiles) and under none (headers), one stream, nothing waited for.  The packets (host header from the device's records,
    the device's tile) equal the all-host chain over the downloaded grids, and read back to those grids"""
    import encdec_model as EM
    import md_inter_model as D
    import modes_inter_model as IM
    import gen_golden_tokens as GG
    import modes_model as MM
    from test_coef_update import read_back
    from test_gpu_boolcode import enqueue_intra
    from test_gpu_encdec import DevPicture, flags_of, make_inputs
    from test_gpu_md_inter import MdBuffers, md_device
    from test_gpu_modes import ModesBuffers, Tile
    from test_gpu_modes import modes_device as modes_kf_device
    from test_gpu_modes_inter import InterBuffers, modes_device
    from test_gpu_tokenize import KEY, TokBuffers, tokenize_device
    lib = B.load()
    B.check(lib.svt_hip_modes_set_tables(ctx, MM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(ctx, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    W, H, q_index, n = 136, 72, 40, 2
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    fr, lrf = IM.frame(**IM.B_PICTURE), (IM.LAST, IM.ALTREF)
    common = dict(width=W, height=H, base_qindex=q_index, filter_level=level, refresh_frame_context=0, frame_parallel_decoding_mode=1)
    fps = [FM.params(**common)] + [FM.inter(reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1), **common)] * n
    # the inter pictures' inputs
    srcs, refs, me = make_inputs(W, H, n, seed=71)
    pic_bytes, nco = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
    slab_src, slab_pred = torch.zeros(n * pic_bytes, dtype=torch.uint8, device="cuda"), torch.zeros(n * pic_bytes, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(n * nco, dtype=torch.int16, device="cuda"), torch.zeros(n * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    blank = (np.zeros((H // 8, W // 8), B.MC_MODE_INFO_DTYPE), np.zeros((H // 8, W // 8), B.LF_MODE_INFO_DTYPE))
    dp = [DevPicture(W, H, srcs[i], refs_dev, blank[0], blank[1], slab_src, slab_pred, slab_q, slab_dq, i, EM.RefPic(W, H)) for i in range(n)]
    res_t = [dev(m.view(np.uint8)) for m in me]
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
    arr = (B.EncdecPicture * n)(*[d.struct(refs) for d in dp])
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    # every output buffer exists before the first launch
    tbs = [TokBuffers(W, H) for _ in range(n + 1)]
    kb, vbs, mbs = ModesBuffers(W, H), [MdBuffers(W, H, want_cand=False) for _ in dp], [InterBuffers(W, H) for _ in dp]
    tiles = [Tile(W, H, tbs[0], kb)] + [Tile(W, H, tb, mb) for tb, mb in zip(tbs[1:], mbs)]
    stage = []
    for tb, fp in zip(tbs, fps):
        pre, suf = CM.header_parts(fp)
        p = Picture(np.zeros(0, np.uint32), counts=np.zeros(B.TOK_COUNTS, np.uint32), prefix=pre, suffix=suf)
        p.struct.d_tokens, p.struct.d_counts, p.struct.max_tokens = tb.tokens.data_ptr(), tb.counts.data_ptr(), tb.cap
        p.struct.d_n_tokens = tb.sb_off.data_ptr() + 4 * (tb.sb_off.numel() - 1)          # the tokeniser's total: the device alone knows it
        stage.append(p)
    hdrs = []
    for p in stage:
        h = Stream(bools=np.zeros(1, np.uint16), segments=[(0, 1, 1)], max_bools=p.cap)
        h.struct.d_bools, h.struct.d_segments = p.keep["bools"].data_ptr(), p.keep["seg"].data_ptr()
        hdrs.append(h)
    keep = []
    frames = T.gen_clip_subpel(W, H, 3, 72)
    key_lf = EM.gen_intra_grid(72, W, H, sizes=(4, 8, 16, 32), filter_level=level)
    torch.cuda.synchronize()
    try:
        lf_k, q_k, emap_k, work_k = enqueue_intra(ctx, W, H, (frames[1],) + GG._chroma(frames[1], 1), key_lf, q_index, keep)
        B.check(lib.svt_hip_md_default_batch_device(ctx, n, ptrs(res_t), W, H, 300, level, ptrs([d.mc_t for d in dp]), ptrs([d.lf_t for d in dp]), W // 8))
        B.check(lib.svt_hip_encdec_batch_device(ctx, work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), EM.PAD, EM.PAD))
        tokenize_device(ctx, W, H, [(lf_k, q_k, emap_k)] + [(d.lf_t, d.q_t, d.emap_t) for d in dp], tbs)
        modes_kf_device(ctx, W, H, [(lf_k, emap_k, tbs[0].tok_off)], [kb])
        md_device(ctx, W, H, [vb.struct((d.lf_t, d.mc_t), dict(W=W, H=H, frame=fr, restrict=rs, lrf=lrf), ref_mask=0) for vb, d, rs in zip(vbs, dp, (0, 1))])
        modes_device(ctx, W, H, [((d.lf_t, d.mc_t, vb.ext), d.emap_t, tb.tok_off, fr) for d, vb, tb in zip(dp, vbs, tbs[1:])], mbs)
        B.check(lib.svt_hip_coef_update_batch_device(ctx, n + 1, (B.CuPicture * (n + 1))(*[p.struct for p in stage])))
        own = (C.c_void_p * (2 * n + 2))(*([p.keep["probs"].data_ptr() for p in stage] + [None] * (n + 1)))
        B.check(lib.svt_hip_boolcode_batch_tables_device(ctx, 2 * n + 2, (B.BoolStream * (2 * n + 2))(*[s.struct for s in tiles] + [h.struct for h in hdrs]), own))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0 and lib.svt_hip_encdec_work_status(ctx, work_k, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    lib.svt_hip_encdec_work_destroy(ctx, work_k)
    grid = lambda t, dt: t.cpu().numpy().view(dt).reshape(H // 8, W // 8)      # noqa: E731
    pictures = [("key", dict(W=W, H=H, lf_mi=grid(lf_k, B.LF_MODE_INFO_DTYPE), qcoeff=q_k.cpu().numpy(), eob_map=emap_k.cpu().numpy().view(np.uint16)))]
    for d, rs in zip(dp, (0, 1)):
        full = dict(W=W, H=H, frame=fr, restrict=rs, lrf=lrf, lf_mi=grid(d.lf_t, B.LF_MODE_INFO_DTYPE), mc_mi=grid(d.mc_t, B.MC_MODE_INFO_DTYPE), qcoeff=d.q_t.cpu().numpy(),
                    eob_map=d.emap_t.cpu().numpy().view(np.uint16))
        lab = D.host_md_inter(full, ref_mask=0, want_cand=False)
        assert lab["rc"] == 0 and lab["status"][0] != B.MODES_BAD_GRID
        pictures.append(("inter", dict(full, ext=lab["ext_out"])))
    sent = 0
    for (kind, pic), fp, p, t, h in zip(pictures, fps, stage, tiles, hdrs):
        want = CM.host_frame(kind, pic, fp, update=True)
        got = p.result()
        assert got["untouched"] and np.array_equal(got["probs"], want["probs"]) and np.array_equal(got["bools"], want["stage"]["bools"]), kind
        tile, size, guard = t.result()
        assert tile == want["tile"] and size == len(want["tile"]), kind
        rc, hdr, ub, cb, _ = CM.header_coef(fp, got["bools"])
        comp, csize, _ = h.result()
        assert rc == 0 and hdr == want["header"] and comp == hdr[ub:] and csize == cb, kind
        assert hdr + tile == want["frame"] and len(want["frame"]) < len(CM.host_frame(kind, pic, fp, update=False)["frame"]), kind
        _, tabs, back = read_back(hdr + tile, kind, pic)          # the grids, coefficients and eob maps the device coded
        assert back["guards"] and np.array_equal(tabs["coef_probs"][0], got["probs"]) and back["res"]["past_end"] == 0, kind
        assert np.array_equal(back["qcoeff"], pic["qcoeff"]) and np.array_equal(back["eob_map"], pic["eob_map"]), kind
        assert all(np.array_equal(back["lf_mi"][f], pic["lf_mi"][f]) for f in ("sb_type", "tx_size", "skip", "is_inter")), kind
        sent += sum(int(v) for v in got["result"]["sent"])
    assert sent >= 3

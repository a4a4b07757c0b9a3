"""GPU: the entropy pass's coefficient-update mode (svt_hip_entropy_work_set_coef_update, csrc/entropy.hip) through the C ABI, byte for byte
against the host form svt_hip_entropy_picture_coef (which tests/test_entropy_coef_host.py pins to the recorded frames): the fixture
pictures, a mixed key and inter batch in both orders, 32 pictures of 64x64 on grids of 17 and 24 records a row (64 streams: the two
bool-coder calls), the chain behind the real encode pass with every packet read back, a first picture withheld by each budget, one
workspace switched on, off and on under one synchronisation, the stage hook in both modes, counts given and not.  Every output lies
between guard bands."""
import ctypes as C

import numpy as np
import pytest
import torch

import coef_update_model as CM
import entropy_coef_model as EC
import entropy_model as E
import frame_model as FM
import md_inter_model as D
import modes_inter_model as IM
import mvrefs_model as M
import svt_testlib as T
import test_gpu_entropy as GE
import tokenize_model as TM

B = T.B
pytestmark = pytest.mark.gpu
DEFAULT = CM.BM.tables()[0]["coef_probs"].reshape(-1)


@pytest.fixture(scope="module")
def ctx():
    lib, c = B.load(), C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    tb, tm, ti = E.tables()
    B.check(lib.svt_hip_boolcode_set_tables(c, tb.ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_set_tables(c, tm.ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(c, ti.ctypes.data_as(C.c_void_p)))
    yield c
    lib.svt_hip_ctx_destroy(c)


def switch(ctx, work, on):
    B.check(B.load().svt_hip_entropy_work_set_coef_update(ctx, work.ptr, int(on)))


def expected(cases, lim, counts=False):
    return [EC.host_entropy_coef(p, fp, lim, trailer=tr, counts=counts) for p, fp, tr in cases]


def stage_outputs(ctx, work, pic):
    """the probabilities and the stage's record of picture pic, from the workspace's second slab"""
    b = B.EntropyCoefBuffers()
    B.check(B.load().svt_hip_entropy_work_coef_buffers(work.ptr, pic, C.byref(b)))
    # the layout's capacities are the stage's and the bool coder's own answers
    assert b.hdr_bools_capacity == int(B.load().svt_hip_coef_update_bools_capacity()) and b.hdr_capacity == EC.hdr_capacity() <= 0xFFFF
    probs, res = np.zeros(1728, np.uint8), np.zeros(1, B.CU_RESULT_DTYPE)
    B.check(B.load().svt_hip_mem_download(ctx, probs.ctypes.data_as(C.c_void_p), C.c_void_p(b.d_probs), 1728))
    B.check(B.load().svt_hip_mem_download(ctx, res.ctypes.data_as(C.c_void_p), C.c_void_p(b.d_result), res.nbytes))
    return probs, res[0]


def run(ctx, cases, lim=None, stride=None, counts=False, work=None, slack=64, want=None):
    """one call in the mode over [(picture, frame parameters, trailer)], checked against the host form: packets, table, results, the
    probabilities and the stage's record of every picture"""
    W, H = cases[0][0]["W"], cases[0][0]["H"]
    lim = lim or E.limits(W, H, len(cases))
    want = want or expected(cases, lim, counts)
    devs = [GE.DevPic(p, counts) for p, _, _ in cases]
    arr = (B.EntropyPicture * len(cases))(*[GE.struct_of(d, p, fp, tr) for d, (p, fp, tr) in zip(devs, cases)])
    call = GE.Call(ctx, len(cases), sum(len(w["packet"] or b"") for w in want) + slack)
    own = work is None
    work = work or GE.Work(ctx, W, H, lim, stride)
    torch.cuda.synchronize()
    try:
        switch(ctx, work, True)
        B.check(call.enqueue(ctx, work, arr))
        B.check(B.load().svt_hip_ctx_synchronize(ctx))
        res = GE.check_call(call, want)
        for i, w in enumerate(want):
            probs, rec = stage_outputs(ctx, work, i)
            assert np.array_equal(probs, w["probs"]) and rec.tobytes() == w["update"].tobytes(), i
        if counts:
            for d, w in zip(devs, want):
                got, ok = d.counts_result()
                assert ok and np.array_equal(got, w["counts"])
    finally:
        if own:
            work.free()
    return want, res, devs


def fixture_case(k, trailer=b""):
    name, kind, pic, fp, entry = EC.fixture_cases()[k]
    return entry, fp, trailer


def test_fixture_pictures_from_the_device_equal_the_host_form_and_the_recorded_frames(ctx):
    """edge_72x40_select and the key frame in one 72x40 call, the two 136x72 pictures in another"""
    names = [c[0] for c in EC.fixture_cases()]
    by_size = {}
    for k, c in enumerate(EC.fixture_cases()):
        by_size.setdefault((c[4]["W"], c[4]["H"]), []).append(k)
    assert sorted(len(v) for v in by_size.values()) == [2, 2]
    for ks in by_size.values():
        want, res, _ = run(ctx, [fixture_case(k) for k in ks])
        for k, w in zip(ks, want):
            assert w["packet"] == bytes(CM.fixture()[f"frame_with|{names[k]}"]) and sum(int(v) for v in w["update"]["sent"]) >= 1


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_mixed_batch_of_a_key_and_an_inter_picture(ctx, order):
    cases = EC.fixture_cases()
    key = next(k for k, c in enumerate(cases) if c[1] == "key")
    inter = next(k for k, c in enumerate(cases) if c[1] == "inter" and (c[4]["W"], c[4]["H"]) == (cases[key][4]["W"], cases[key][4]["H"]))
    both = [fixture_case(key), fixture_case(inter, GE.SHOW_EXT)]
    want, _, _ = run(ctx, [both[i] for i in order])
    assert all(w["packet"] is not None for w in want) and want[order.index(1)]["packet"].endswith(GE.SHOW_EXT)


def batch_of_32(extra):
    """32 pictures of 64x64, key and inter pictures alternating, on grids `extra` records a row wider than the picture"""
    fr = IM.frame(reference_mode=IM.SELECT, sign_bias=M.ALT_BIAS)
    cases = []
    for i in range(32):
        if i % 2 == 0:
            g = IM.make_picture(64, 64, "random", 900 + i % 6, IM.frame(), 1.0)         # every leaf intra: a key picture's grid
            p, fp = dict(W=64, H=64, lf_mi=g["lf_mi"], mc_mi=None, qcoeff=g["qcoeff"], eob_map=g["eob_map"]), E.key_params(64, 64, base_qindex=40 + i, **EC.NO_REFRESH)
        else:
            p = D.encoder_like(64, 64, 930 + i % 10, fr, i // 2 & 1, (IM.LAST, IM.ALTREF), 0.1 + 0.05 * (i % 5))
            fp = E.inter_params(p, base_qindex=60 + i, **EC.NO_REFRESH)
        p = dict(p, lf_mi=TM.with_stride(p["lf_mi"], extra, i), mc_mi=TM.with_stride(p["mc_mi"], extra, 40 + i) if p["mc_mi"] is not None else None)
        cases.append((p, fp, GE.SHOW_EXT[:i % 5]))
    return cases


@pytest.mark.parametrize("stride", [17, 24])
def test_32_pictures_of_64x64_need_both_bool_coder_calls(ctx, stride):
    """32 tiles and 32 compressed headers are 64 streams, twice what one bool-coder call takes"""
    cases = batch_of_32(stride - 8)
    want, res, _ = run(ctx, cases, stride=stride)
    assert all(w["packet"] is not None for w in want) and len({w["packet"] for w in want}) >= 8
    assert sum(int(r["inter_leaves"]) > 0 for r in res) == 16
    assert any(sum(int(v) for v in w["update"]["sent"]) for w in want)


def three_pictures():
    fr = IM.frame(reference_mode=IM.SELECT, sign_bias=M.ALT_BIAS)
    pics = [D.encoder_like(136, 72, 420 + k, fr, k & 1, (IM.LAST, IM.ALTREF), 0.1 + 0.1 * k) for k in range(3)]
    return [(p, E.inter_params(p, **EC.NO_REFRESH), b"") for p in pics]


@pytest.mark.parametrize("what", ["max_tokens", "max_bools", "max_tile_bytes"])
def test_a_first_picture_withheld_by_a_budget_leaves_the_other_two_exact(ctx, what):
    """the picture that holds the most stands first and its budget is one short: exactly that flag, no packet, the other two packets
    byte-exact and dense.  Under TOKENS_OVER the update stage scans max_tokens records and no more; the header stream is coded and ignored"""
    cases = three_pictures()
    full = expected(cases, E.limits(136, 72, 3))
    assert all(w["packet"] is not None for w in full)
    field = dict(max_tokens=lambda w: w["result"]["tokens"], max_bools=lambda w: w["stream_bools"], max_tile_bytes=lambda w: w["result"]["tile_bytes"])[what]
    flag = dict(max_tokens=B.ENT_TOKENS_OVER, max_bools=B.ENT_STREAM_OVER, max_tile_bytes=B.ENT_TILE_OVER)[what]
    counts = [field(w) for w in full]
    first = int(np.argmax(counts))
    assert sorted(counts)[-1] > sorted(counts)[-2], "one picture holds the most"
    cases = [cases[i] for i in [first] + [i for i in range(3) if i != first]]
    budget = GE.budget_of(full, 3)
    budget[what] -= 1
    want, res, _ = run(ctx, cases, E.limits(136, 72, 3, **budget))
    assert [int(r["flags"]) for r in res] == [flag, 0, 0] and want[0]["packet"] is None and want[1]["packet"] and want[2]["packet"]
    if what == "max_tokens":
        assert int(want[0]["update"]["tokens"]) == budget["max_tokens"]


def test_one_workspace_switched_on_off_on_with_one_synchronisation(ctx):
    """three calls on one workspace into three arenas, the mode on, off and on again, nothing waited for in between; the off call's arena,
    table and results are those of a workspace on which the mode was never enabled"""
    cases = [fixture_case(k) for k, c in enumerate(EC.fixture_cases()) if (c[4]["W"], c[4]["H"]) == (136, 72)]
    assert len(cases) == 2
    lim = E.limits(136, 72, 2)
    on, off = expected(cases, lim), GE.expected(cases, lim)
    assert all(len(a["packet"]) < len(b["packet"]) for a, b in zip(on, off))
    devs = [GE.DevPic(p) for p, _, _ in cases]
    arr = (B.EntropyPicture * 2)(*[GE.struct_of(d, p, fp, tr) for d, (p, fp, tr) in zip(devs, cases)])
    cap = sum(len(w["packet"]) for w in off) + 32
    calls = [GE.Call(ctx, 2, cap) for _ in range(4)]
    work, never = GE.Work(ctx, 136, 72, lim), GE.Work(ctx, 136, 72, lim)
    torch.cuda.synchronize()
    try:
        for call, mode in zip(calls, (True, False, True)):
            switch(ctx, work, mode)
            B.check(call.enqueue(ctx, work, arr))
        B.check(calls[3].enqueue(ctx, never, arr))
        B.check(B.load().svt_hip_ctx_synchronize(ctx))
        for call, want in zip(calls, (on, off, on, off)):
            GE.check_call(call, want)
        a, b = calls[1].result(), calls[3].result()
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
        assert B.load().svt_hip_entropy_work_coef_buffers(never.ptr, 0, C.byref(B.EntropyCoefBuffers())) == -1      # no second slab there
    finally:
        work.free()
        never.free()


def test_stage_hook_order_in_both_modes(ctx):
    seen = []
    hook = B.ENTROPY_STAGE_HOOK(lambda user, stage: seen.append(stage))
    cases = [fixture_case(k) for k, c in enumerate(EC.fixture_cases()) if (c[4]["W"], c[4]["H"]) == (72, 40)]
    lim = E.limits(72, 40, 2)
    work = GE.Work(ctx, 72, 40, lim)
    try:
        B.load().svt_hip_entropy_work_set_stage_hook(work.ptr, hook, None)
        run(ctx, cases, lim, work=work)
        on, seen[:] = list(seen), []
        switch(ctx, work, False)
        GE.run(ctx, cases, lim, work=work)
        off = list(seen)
    finally:
        work.free()
    assert B.ENT_STAGE_COEF_UPDATE == 9 and B.ENT_STAGES_COEF[9] == "coef_update"
    assert on == [0, 1, 2, 3, 9, 4, 5, 6, 7, 8] and off == list(range(9))


def test_counts_given_and_not(ctx):
    """with d_counts NULL the workspace's own counts feed the stage; given, the caller's receive the tokeniser's counts between their guards"""
    cases = [fixture_case(k) for k, c in enumerate(EC.fixture_cases()) if (c[4]["W"], c[4]["H"]) == (136, 72)]
    a, _, _ = run(ctx, cases, counts=False)
    b, _, _ = run(ctx, cases, counts=True)
    assert [w["packet"] for w in a] == [w["packet"] for w in b]


def test_refusals_launch_nothing(ctx):
    lib = B.load()
    cases = [fixture_case(k) for k, c in enumerate(EC.fixture_cases()) if (c[4]["W"], c[4]["H"]) == (72, 40)]
    devs = [GE.DevPic(p, counts=True) for p, _, _ in cases]
    lim = E.limits(72, 40, 2)
    work, call = GE.Work(ctx, 72, 40, lim), GE.Call(ctx, 2, 4096)
    torch.cuda.synchronize()
    try:
        assert lib.svt_hip_entropy_work_set_coef_update(None, work.ptr, 1) == -1 and lib.svt_hip_entropy_work_set_coef_update(ctx, None, 1) == -1
        switch(ctx, work, True)
        for pic in (0, 1):
            structs = [GE.struct_of(d, p, f, tr) for d, (p, f, tr) in zip(devs, cases)]
            structs[pic].frame = FM.struct(dict(cases[pic][1], refresh_frame_context=1))
            assert call.enqueue(ctx, work, (B.EntropyPicture * 2)(*structs)) == -1
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert call.untouched() and all((d.counts.cpu().numpy().view(np.uint32) == GE.CNT_FILL).all() for d in devs)
        switch(ctx, work, False)                                        # the plain pass takes such a picture, as before
        structs = [GE.struct_of(d, p, f, tr) for d, (p, f, tr) in zip(devs, cases)]
        structs[0].frame = FM.struct(dict(cases[0][1], refresh_frame_context=1))
        assert call.enqueue(ctx, work, (B.EntropyPicture * 2)(*structs)) == 0
        B.check(lib.svt_hip_ctx_synchronize(ctx))
    finally:
        work.free()


def test_behind_the_real_encode_pass_key_and_inter_pictures(ctx):
    """136 x 72 at q index 40, the inputs of test_gpu_coef_update's chain test: a key picture through svt_hip_encdec_intra_device and two
    inter pictures through svt_hip_md_default_batch_device and svt_hip_encdec_batch_device, then ONE svt_hip_entropy_batch_device in the
    mode over the three, nothing waited for.  The packets equal the host form over the downloaded grids, send at least three transform
    sizes, are smaller than the plain pass's, and read back to the grids, coefficients, eob maps and the updated tables"""
    import encdec_model as EM
    import gen_golden_tokens as GG
    from test_gpu_boolcode import enqueue_intra
    from test_gpu_encdec import DevPicture, dev, flags_of, make_inputs
    from test_gpu_tokenize import KEY
    lib = B.load()
    W, H, q_index, n = 136, 72, 40, 2
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    fr, lrf = IM.frame(**IM.B_PICTURE), (IM.LAST, IM.ALTREF)
    common = dict(width=W, height=H, base_qindex=q_index, filter_level=level, refresh_frame_context=0, frame_parallel_decoding_mode=1)
    fps = [FM.params(**common)] + [FM.inter(reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1), **common)] * n
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
    encdec_work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(encdec_work)))
    lim = E.limits(W, H, n + 1)
    work, call = GE.Work(ctx, W, H, lim), GE.Call(ctx, n + 1, (n + 1) * 60000)
    switch(ctx, work, True)
    keep = []
    frames = T.gen_clip_subpel(W, H, 3, 72)
    key_lf = EM.gen_intra_grid(72, W, H, sizes=(4, 8, 16, 32), filter_level=level)
    metas = [dict(W=W, H=H, frame=fr, restrict=rs, lrf=lrf) for rs in (0, 1)]
    torch.cuda.synchronize()
    try:
        lf_k, q_k, emap_k, work_k = enqueue_intra(ctx, W, H, (frames[1],) + GG._chroma(frames[1], 1), key_lf, q_index, keep)
        B.check(lib.svt_hip_md_default_batch_device(ctx, n, ptrs(res_t), W, H, 300, level, ptrs([d.mc_t for d in dp]), ptrs([d.lf_t for d in dp]), W // 8))
        B.check(lib.svt_hip_encdec_batch_device(ctx, encdec_work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), EM.PAD, EM.PAD))
        ent = [E.fill_struct(B.EntropyPicture(), (lf_k.data_ptr(), None, q_k.data_ptr(), emap_k.data_ptr()), fps[0])]
        ent += [E.fill_struct(B.EntropyPicture(), (d.lf_t.data_ptr(), d.mc_t.data_ptr(), d.q_t.data_ptr(), d.emap_t.data_ptr()), fp, lrf, m["restrict"])
                for d, m, fp in zip(dp, metas, fps[1:])]
        B.check(call.enqueue(ctx, work, (B.EntropyPicture * (n + 1))(*ent)))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, encdec_work, None) == 0 and lib.svt_hip_encdec_work_status(ctx, work_k, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, encdec_work)
        work.free()
    lib.svt_hip_encdec_work_destroy(ctx, work_k)
    grid = lambda t, dt: t.cpu().numpy().view(dt).reshape(H // 8, W // 8)      # noqa: E731
    held = [dict(W=W, H=H, lf_mi=grid(lf_k, B.LF_MODE_INFO_DTYPE), mc_mi=None, qcoeff=q_k.cpu().numpy(), eob_map=emap_k.cpu().numpy().view(np.uint16))]
    held += [dict(m, lf_mi=grid(d.lf_t, B.LF_MODE_INFO_DTYPE), mc_mi=grid(d.mc_t, B.MC_MODE_INFO_DTYPE), qcoeff=d.q_t.cpu().numpy(), eob_map=d.emap_t.cpu().numpy().view(np.uint16))
             for d, m in zip(dp, metas)]
    want = expected([(p, fp, b"") for p, fp in zip(held, fps)], lim)
    GE.check_call(call, want)
    sent = 0
    for p, fp, w in zip(held, fps, want):
        assert w["packet"] is not None and len(w["packet"]) < len(E.host_entropy(p, fp, lim)["packet"])
        rc, info, back, table, untouched = EC.read_frame_coef(w["packet"], W, H, restrict=p.get("restrict", 0), lrf=lrf)
        assert rc == 0 and untouched and back["guards"] and back["res"]["past_end"] == 0, lib.svt_hip_last_error()
        assert np.array_equal(table, w["probs"]) and np.array_equal(back["qcoeff"], p["qcoeff"]) and np.array_equal(back["eob_map"], p["eob_map"])
        assert all(np.array_equal(back["lf_mi"][f], p["lf_mi"][f]) for f in ("sb_type", "tx_size", "skip", "is_inter"))
        if p["mc_mi"] is not None:
            assert back["mc_mi"].tobytes() == p["mc_mi"].tobytes()
        sent += sum(int(v) for v in w["update"]["sent"])
    assert sent >= 3

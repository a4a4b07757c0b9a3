"""GPU: the open-loop intra search (svt_hip_intra_search_device) against the oracle's predictors on the source, the device grid builder
(svt_hip_md_intra_search_device) against its host form, the intra encode pass on a searched grid against the oracle chain, the searched
grid's quality on a picture only V / H predict, and the opt-in of the encoder library (SVT_HIP_INTRA_DECISION=search)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import encdec_model as M
import intra_search_model as S
import svt_testlib as T
from test_gpu_encdec import dev, flags_of
from test_gpu_intra import KEY, run_intra

B = T.B
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


def picture(W, H, seed):
    """gen_yuv's luma with textured chroma planes (gen_yuv's Cr is flat)"""
    y, u, _ = T.gen_yuv(W, H, seed)
    v = (255 - y[1::2, ::2] // 2).astype(np.uint8)
    return y, u, v


def device_search(ctx, src, stride_pad=0):
    """records of svt_hip_intra_search_device for the tight (or, with stride_pad, wider) source planes"""
    lib = B.load()
    H, W = src[0].shape
    ys, cs = W + stride_pad, W // 2 + stride_pad // 2
    y = np.zeros((H, ys), np.uint8); y[:, :W] = src[0]
    u = np.zeros((H // 2, cs), np.uint8); u[:, :W // 2] = src[1]
    v = np.zeros((H // 2, cs), np.uint8); v[:, :W // 2] = src[2]
    buf = dev(np.concatenate([y.ravel(), u.ravel(), v.ravel()]))
    d = B.YuvPlanes()
    base = buf.data_ptr()
    d.y, d.u, d.v, d.y_stride, d.uv_stride, d.width, d.height = base, base + y.size, base + y.size + u.size, ys, cs, W, H
    n_sb = T.n_sb(W, H)
    out = torch.full((n_sb * B.OIS_PER_SB * 12,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    B.check(lib.svt_hip_intra_search_device(ctx, C.byref(d), W, H, C.c_void_p(out.data_ptr())))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    return out, out.cpu().numpy().view(B.OIS_BLOCK_DTYPE).reshape(n_sb, B.OIS_PER_SB)


def device_grid(ctx, d_ois, W, H, lam, level, mi_stride=None):
    lib = B.load()
    mi_stride = mi_stride or W // 8
    lf_t = torch.full(((H // 8) * mi_stride * 8,), 0x33, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    B.check(lib.svt_hip_md_intra_search_device(ctx, C.c_void_p(d_ois.data_ptr()), W, H, C.c_uint32(lam), level, C.c_void_p(lf_t.data_ptr()), mi_stride))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    return lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, mi_stride)


def edge_sbs(W, H, n_random, seed):
    sb_cols, sb_rows = (W + 63) // 64, (H + 63) // 64
    edge = [sb for sb in range(sb_cols * sb_rows) if sb % sb_cols in (0, sb_cols - 1) or sb // sb_cols in (0, sb_rows - 1)]
    inner = sorted(set(range(sb_cols * sb_rows)) - set(edge))
    pick = np.random.default_rng(seed).choice(inner, size=min(n_random, len(inner)), replace=False).tolist()
    return sorted(edge + pick)


@pytest.mark.parametrize("W,H,seed,sampled,stride_pad", [(640, 360, 1, False, 0), (640, 360, 5, False, 64), (1288, 728, 2, False, 0),
                                                         (1920, 1080, 3, True, 0), (3840, 2160, 4, True, 0)])
def test_search_records_equal_the_oracle_model(ctx, W, H, seed, sampled, stride_pad):
    src = picture(W, H, seed)
    _, got = device_search(ctx, src, stride_pad)
    sbs = edge_sbs(W, H, 64, seed) if sampled else list(range(T.n_sb(W, H)))
    want = S.oracle_ois(src, sbs)
    for sb in sbs:
        assert got[sb].tobytes() == want[sb].tobytes(), (sb, np.nonzero(got[sb] != want[sb])[0][:8].tolist())
    inside = S.inside_mask(W, H)[sbs]
    assert (got[sbs]["sad"][~inside] == S.NONE).all() and (got[sbs]["sad"][inside] != S.NONE).all()
    modes = got[sbs]["mode"][inside]
    assert len(np.unique(modes)) >= 5                                       # several predictors win


@pytest.mark.parametrize("W,H,seed", [(640, 360, 1), (1288, 728, 2), (1920, 1080, 3), (3840, 2160, 4)])
def test_device_grid_equals_the_host_form(ctx, W, H, seed):
    lib = B.load()
    d_ois, ois = device_search(ctx, picture(W, H, seed))
    for q in (60, 200):
        ac = lib.svt_hip_vp9_ac_step(q)
        lam, level = 4 * ac, lib.svt_hip_lf_level_from_q(ac, 1)
        stride = W // 8 + (3 if q == 200 else 0)
        got = device_grid(ctx, d_ois, W, H, lam, level, stride)
        want = S.host_grid(ois, W, H, lam, level, stride)
        assert got[:, :W // 8].tobytes() == want[:, :W // 8].tobytes()
        assert (got[:, W // 8:].view(np.uint8) == 0x33).all()                # nothing written beyond the picture's units
        assert len(np.unique(got["sb_type"][:, :W // 8])) >= 3


@pytest.mark.parametrize("q", [60, 160])
def test_intra_pass_on_the_searched_grid_equals_the_oracle_chain(ctx, q):
    lib = B.load()
    W, H = 1920, 1080
    src = T.gen_yuv(W, H, 21)
    d_ois, ois = device_search(ctx, src)
    ac = lib.svt_hip_vp9_ac_step(q)
    level = lib.svt_hip_lf_level_from_q(ac, 1)
    mi = device_grid(ctx, d_ois, W, H, 4 * ac, level)
    assert mi.tobytes() == S.host_grid(ois, W, H, 4 * ac, level).tobytes()
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    g = run_intra(ctx, src, mi, q, flags, thr, M.RefPic(W, H), want_pred=False)
    assert g["rc"] == 0
    o = M.oracle_intra_chain(src, mi, q, flags, thr, recon_init=M.RefPic(W, H))
    assert np.array_equal(g["q"], o["qcoeff"]) and np.array_equal(g["emap"], o["eob_map"])
    assert np.array_equal(g["lf"]["skip"], o["lf_mi"]["skip"])
    assert np.array_equal(g["rec"], o["rec"].buf), int(np.sum(g["rec"] != o["rec"].buf))


def stripes_picture(W, H, seed):
    """left half: vertical stripes, right half: horizontal stripes (1 or 2 samples wide, random values), a linear gradient band of 16 rows
    at the bottom: only V (left) or H (right) predicts a stripe block exactly (TM too, but it ties and loses on the mode index)"""
    rng = np.random.default_rng(seed)

    def stripes(n):
        out = []
        while len(out) < n:
            out += [int(rng.integers(0, 256))] * int(rng.integers(1, 3))
        return np.array(out[:n], np.uint8)
    band = H - 16
    y = np.zeros((H, W), np.uint8)
    y[:band, :W // 2] = stripes(W // 2)[None, :]
    y[:band, W // 2:] = stripes(band)[:, None]
    xs, ys = np.meshgrid(np.arange(W), np.arange(band, H))
    y[band:] = ((xs * 200) // W + (ys - band)).astype(np.uint8)
    u = np.full((H // 2, W // 2), 110, np.uint8)
    v = (np.arange(W // 2)[None, :] // 3 + 60 + np.zeros((H // 2, 1), int)).astype(np.uint8)
    return (y, u, v), band


def luma_psnr(rec_buf, src):
    y = M.RefPic(src[0].shape[1], src[0].shape[0]).interior(rec_buf)[0].astype(np.float64)
    mse = np.mean((y - src[0]) ** 2)
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-9))


def coded_luma_blocks(lf):
    """(x0, y0, n, mode) of every luma block of an intra grid"""
    out = []
    for ur, uc in zip(*np.nonzero(np.ones(lf.shape, bool))):
        m = lf[ur, uc]
        st = int(m["sb_type"])
        n8 = {0: 1, 3: 1, 6: 2, 9: 4}[st]
        if ur % n8 or uc % n8:
            continue
        if st == 0:
            md = int(m["pad"][1]) | int(m["pad"][0]) << 8
            out += [(uc * 8 + 4 * (k & 1), ur * 8 + 4 * (k >> 1), 4, (md >> (4 * k)) & 15) for k in range(4)]
        else:
            out.append((uc * 8, ur * 8, 8 * n8, int(m["pad"][1])))
    return out


def test_searched_grid_finds_the_stripes_and_beats_the_dc_stand_in(ctx):
    lib = B.load()
    W, H, q = 640, 360, 120
    src, band = stripes_picture(W, H, 9)
    ac = lib.svt_hip_vp9_ac_step(q)
    level = lib.svt_hip_lf_level_from_q(ac, 1)
    d_ois, ois = device_search(ctx, src)
    mi = device_grid(ctx, d_ois, W, H, 4 * ac, level)
    n_v = n_h = 0
    for x0, y0, n, mode in coded_luma_blocks(mi):
        if y0 + n <= band and x0 + n <= W // 2 and y0 > 0:
            assert mode == 1, (x0, y0, n, mode)                                 # V
            n_v += 1
        if y0 + n <= band and x0 > W // 2:
            assert mode == 2, (x0, y0, n, mode)                                 # H
            n_h += 1
    assert n_v > 20 and n_h > 20
    assert len(np.unique(mi["pad"][..., 1])) > 1
    flags, thr = flags_of(**KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    dc = np.zeros_like(mi)
    r, c = np.meshgrid(np.arange(H // 8), np.arange(W // 8), indexing="ij")
    fit = ((r & ~1) + 2 <= H // 8) & ((c & ~1) + 2 <= W // 8)
    dc["sb_type"], dc["tx_size"], dc["filter_level"] = np.where(fit, 6, 3), np.where(fit, 2, 1), level
    gs = run_intra(ctx, src, mi, q, flags, thr, M.RefPic(W, H), want_pred=False)
    gd = run_intra(ctx, src, dc, q, flags, thr, M.RefPic(W, H), want_pred=False)
    assert gs["rc"] == 0 and gd["rc"] == 0
    # (both reconstructions are deterministic: 45.79 against 43.85 dB.  At this q index the quantiser, not the predictor, bounds the
    # distortion of a vertically constant pattern: a V chain inherits the error of the first block row it copies from)
    p_s, p_d = luma_psnr(gs["rec"], src), luma_psnr(gd["rec"], src)
    assert p_s >= p_d + 1.5, (p_s, p_d)


# ---- through the public API ----
import test_enc_shim_encdec as E  # noqa: E402  (its helpers: run_clip, structure, chroma, stand_in)


def key_grid(src, W, H, q_index, level):
    """the grid the library's searched stand-in gives a key frame: the search model's records -> the host form"""
    lam = 4 * B.load().svt_hip_vp9_ac_step(q_index)
    return S.host_grid(S.oracle_ois(src), W, H, lam, level)


def oracle_clip_searched(frames, W, H, N, enc_mode, tune, qp, recon_file, intra_period):
    """E.oracle_clip with the searched grid in place of the 16x16 DC stand-in on the intra pictures"""
    lib = B.load()
    q_index = lib.svt_hip_vp9_qindex_from_qp(qp)
    ac = lib.svt_hip_vp9_ac_step(q_index)
    level_key = lib.svt_hip_lf_level_from_q(ac, 1)
    thr = B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    pics = [T.PaPic(f) for f in frames]
    minigop = 16 if tune != 0 else 8
    recs, outs = {}, {}
    for (k, layer, lv, nl, r0, r1, used) in E.structure(N, minigop, intra_period):
        src = (frames[k],) + E.chroma(frames[k], k)
        if nl == 0:
            lf = key_grid(src, W, H, q_index, level_key)
            c, fl = B.EncdecFlagsConfig(enc_mode=enc_mode, tune=tune, temporal_layer_index=0, is_used_as_reference=1, recon_file=recon_file, loop_filter=1), B.EncdecFlags()
            assert lib.svt_hip_encdec_flags_derive(C.byref(c), C.byref(fl)) == 0
            o = M.oracle_intra_chain(src, lf, q_index, fl, thr)
            recs[k] = o["rec"]
            outs[k] = dict(intra=True, o=o, grid=lf)
            continue
        p = B.me_params_derive(pic_width=W, pic_height=H, enc_mode=enc_mode, tune=tune, frame_rate=60, num_ref_lists=nl, temporal_layer_index=layer,
                               hierarchical_levels=lv, is_used_as_reference=used, same_ref_poc=int(nl == 2 and r0 == r1))
        me, _ = T.oracle_me_picture_mt(pics[k], pics[r0], pics[r1] if nl == 2 else None, p)
        q_pic = lib.svt_hip_vp9_layer_qindex(qp, tune, lv, layer, 0)
        ac_pic = lib.svt_hip_vp9_ac_step(q_pic)
        level_pic = lib.svt_hip_lf_level_from_q(ac_pic, 0)
        mc, lf = E.stand_in(me, W, H, 4 * ac_pic, level_pic)
        c, fl = B.EncdecFlagsConfig(enc_mode=enc_mode, tune=tune, temporal_layer_index=layer, is_used_as_reference=used, recon_file=recon_file, loop_filter=1), B.EncdecFlags()
        assert lib.svt_hip_encdec_flags_derive(C.byref(c), C.byref(fl)) == 0
        o = M.oracle_encdec_picture(src, [recs[r0], recs[r1 if nl == 2 else r0]], mc, lf, q_pic, fl, thr, use_subpel=int(p.fractional_search_model != 2))
        recs[k] = o["rec"]
        outs[k] = dict(intra=False, o=o, mc=mc)
    return recs, outs


def test_public_api_search_opt_in_equals_the_oracle_chain():
    W, H, N, enc_mode, tune, qp, intra_period = 640, 360, 22, 8, 1, 40, 19
    env = {"SVT_HIP_INTRA_DECISION": "search"}
    frames, recon, order, flags_seen, packets, infos, refpics, _ = E.run_clip(W, H, N, enc_mode, tune, qp, 1, intra_period, False, env=env)
    base = E.run_clip(W, H, N, enc_mode, tune, qp, 1, intra_period, False, frames=frames)
    recs, outs = oracle_clip_searched(frames, W, H, N, enc_mode, tune, qp, 1, intra_period)
    assert sorted(order) == list(range(N)) and len(packets) == N and packets[-1][1] & 1 and flags_seen[-1] == 1
    for k in range(N):
        y, u, v = recs[k].interior()
        assert np.array_equal(recon[k], np.concatenate([y.ravel(), u.ravel(), v.ravel()])), (k, outs[k]["intra"])
    n_key = 0
    for k, d in infos.items():
        i = d["info"]
        if outs[k]["intra"]:
            n_key += 1
            assert i.is_intra and i.decision_source == 2 and base[5][k]["info"].decision_source == 0
            grid = d["lf"].copy()
            grid["skip"] = 0
            assert grid.tobytes() == outs[k]["grid"].tobytes(), k                # the host form of the search model
            assert d["lf"].tobytes() == outs[k]["o"]["lf_mi"].tobytes() and np.array_equal(d["q"], outs[k]["o"]["qcoeff"]), k
        else:
            assert i.decision_source == base[5][k]["info"].decision_source, k
    assert n_key >= 1
    # the inter pictures predict from the searched key frames: they differ from the run with the DC stand-in
    assert sum(not np.array_equal(recon[k], base[1][k]) for k in range(1, N) if not outs[k]["intra"]) >= 5


def test_public_api_rejects_an_unknown_intra_decision():
    lib = E.shim()
    cfg, h = E.Cfg(), C.c_void_p()
    assert lib.eb_vp9_svt_init_handle(C.byref(h), None, C.byref(cfg)) == 0
    cfg.source_width, cfg.source_height, cfg.enc_mode, cfg.tune, cfg.frame_rate, cfg.intra_period, cfg.qp = 256, 192, 8, 1, 60 << 16, 19, 40
    assert lib.eb_vp9_svt_enc_set_parameter(h, C.byref(cfg)) == 0
    saved = os.environ.get("SVT_HIP_INTRA_DECISION")
    os.environ["SVT_HIP_INTRA_DECISION"] = "bogus"
    try:
        assert lib.eb_vp9_init_encoder(h) & 0xffffffff == 0x80001005                # EB_ErrorBadParameter
    finally:
        if saved is None:
            os.environ.pop("SVT_HIP_INTRA_DECISION", None)
        else:
            os.environ["SVT_HIP_INTRA_DECISION"] = saved
    assert lib.eb_vp9_deinit_handle(h) == 0

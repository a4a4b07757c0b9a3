"""GPU: intra blocks in the decode pass.  svt_hip_decode_intra_device (csrc/intra_recon_kernel.hip: the wavefront kernel driven by coefficients)
rebuilds from a key frame's grid, coefficients and eob map the very prediction, reconstruction (padding included), skip flags and loop-filter
masks svt_hip_encdec_intra_device left; svt_hip_decode_mixed_batch_device does the same for inter pictures that hold intra leaves; and a key
frame's packet, read by svt_hip_frame_read_host, goes the whole way back to the encode pass's planes.  The yardstick is always the existing
encode pass (pinned to the oracle chain and to the recorded reference by tests/test_gpu_intra.py, test_gpu_intra_edges.py and
test_gpu_encdec.py), never the new code.  All comparisons exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import boolcode_model as BM
import decode_model as D
import encdec_model as M
import frame_model as FM
import modes_inter_model as IM
import modes_model as MM
import svt_testlib as T
import test_gpu_intra as TI
from test_gpu_encdec import DevPicture, dev, flags_of, make_inputs, masks_equal, md_host
from test_gpu_frame import frame_batch
from test_gpu_md_inter import MdBuffers, md_device
from test_gpu_modes import ModesBuffers, Tile, modes_device
from test_gpu_modes_inter import InterBuffers
from test_gpu_modes_inter import modes_device as inter_modes_device
from test_gpu_tokenize import TokBuffers, tokenize_device
from test_tile_read_inter import read_frame
from tokenize_model import _zorder

B = T.B
pytestmark = pytest.mark.gpu
KEY = TI.KEY                                                                                                     # every encode-pass flag on
NO_LF = dict(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=0, loop_filter=0)   # padded, not deblocked
NO_PAD = dict(enc_mode=8, tune=1, temporal_layer_index=4, is_used_as_reference=0, recon_file=1, loop_filter=1)  # deblocked, not padded
JUNK = 0x5A5A5A5A
GOLD = {c[0]: c for c in M.INTRA_GOLDEN_CASES}
ALL = (4, 8, 16, 32)


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    B.check(lib.svt_hip_boolcode_set_tables(c, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_set_tables(c, MM.tables()[1].ctypes.data_as(C.c_void_p)))
    yield c
    lib.svt_hip_ctx_destroy(c)


def thresholds():
    thr = B.LfThresh()
    B.load().svt_hip_lf_thresh_init(C.byref(thr), 0)
    return thr


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases: (id, kind, ...) -> source planes, grid, q index, encode-pass flags.  Host only: the coverage test reads them through the oracle.
# ---------------------------------------------------------------------------------------------------------------------------------------
def gen(name, W, H, seed, q, sizes, modes=tuple(range(10)), mi_stride=None, cfg=KEY):
    return (name, "gen", W, H, seed, q, sizes, modes, mi_stride, tuple(sorted(cfg.items())))


FIXTURE_SPECS = [(n, "fixture") for n in GOLD]
SINGLE_MODE_SPECS = ([gen(f"mode{m}_4x4", 96, 72, 80 + m, 100, (4,), (m,)) for m in range(10)] +
                     [gen(f"mode{m}_{s}", 192, 136, 70 + m, 110, (8, s) if s > 8 else (8,), (m,)) for s in (8, 16, 32) for m in range(10)])
MIXED_SIZE_SPECS = [gen("all_320x192_q40", 320, 192, 33, 40, ALL), gen("all_320x192_q200", 320, 192, 3, 200, ALL), gen("all_704x392_q160", 704, 392, 34, 160, ALL),
                    gen("stride40_200x136", 200, 136, 9, 180, ALL, mi_stride=40), gen("no_lf_200x136", 200, 136, 10, 180, ALL, cfg=NO_LF),
                    gen("no_pad_200x136", 200, 136, 12, 180, ALL, cfg=NO_PAD)]
# smooth content (a ramp plus noise of amplitude `amp`): the large blocks with FEW coefficients the noisy pictures above do not hold
SOFT_SPECS = [("soft_amp2_q60", "soft", 192, 136, 21, 60, 2), ("soft_amp24_q180", "soft", 192, 136, 21, 180, 24)]
SPECS = FIXTURE_SPECS + SINGLE_MODE_SPECS + MIXED_SIZE_SPECS + SOFT_SPECS
BY_NAME = {s[0]: s for s in SPECS}


@functools.lru_cache(maxsize=None)
def inputs_of(name):
    """(src, mi, W, H, q index, flags configuration) of a case; built once, not written to"""
    spec = BY_NAME[name]
    if spec[1] == "fixture":
        _, W, H, seed, q, kind = GOLD[name]
        src, mi = M.intra_golden_inputs(GOLD[name])
        return src, mi, W, H, q, KEY
    lib = B.load()
    if spec[1] == "soft":
        _, _, W, H, seed, q, amp = spec
        yy, xx = np.mgrid[0:H, 0:W]
        y = (90 + (xx + 2 * yy) // 6 + np.random.default_rng(2000 + seed).integers(0, amp + 1, (H, W))).clip(0, 255).astype(np.uint8)
        mi = M.gen_intra_grid(seed, W, H, sizes=ALL, filter_level=lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q), 1))
        return (y, y[::2, ::2].copy(), (255 - y[1::2, ::2]).astype(np.uint8)), mi, W, H, q, KEY
    _, _, W, H, seed, q, sizes, modes, mi_stride, cfg = spec
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q), 1)
    mi = M.gen_intra_grid(seed, W, H, sizes=sizes, modes=modes, filter_level=level, mi_stride=mi_stride)
    if mi_stride:
        mi["sb_type"][:, W // 8:] = 0
    return T.gen_yuv(W, H, seed), mi, W, H, q, dict(cfg)


def block_table(mi, W, H):
    """(plane, x0, y0, n, tx_type, eob map index, coefficient offset) of every transform block an intra grid codes"""
    e, sb_cols, out = M.eob_map_offsets(W, H), (W + 63) // 64, []
    for plane, x0, y0, n, mode in M.intra_blocks(mi, W, H):
        pw4, sh, mask = (W // 2 if plane else W) // 4, 5 if plane else 6, 31 if plane else 63
        sb = (y0 >> sh) * sb_cols + (x0 >> sh)
        off = sb * B.SB_COEFFS + (0, 4096, 5120)[plane] + _zorder((x0 & mask) >> 2, (y0 & mask) >> 2) * 16
        out.append((plane, x0, y0, n, M.INTRA_TX_TYPE[mode] if plane == 0 and n < 32 else 0, e[plane] + (y0 >> 2) * pw4 + (x0 >> 2), off))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# encode (the yardstick) and decode
# ---------------------------------------------------------------------------------------------------------------------------------------
_encoded = {}


def encoded(ctx, name):
    """svt_hip_encdec_intra_device on a case, once: its outputs on the host, left unchanged"""
    if name not in _encoded:
        src, mi, W, H, q, cfg = inputs_of(name)
        rec_init = M.RefPic(W, H)
        rec_init.buf[:] = np.random.default_rng(len(name)).integers(0, 256, rec_init.buf.size, dtype=np.uint8)
        g = TI.run_intra(ctx, src, mi, q, flags_of(**cfg), thresholds(), rec_init)
        assert g["rc"] == 0
        _encoded[name] = g
    return _encoded[name]


def run_decode(ctx, W, H, mi, q, emap, q_index, thr, no_pad=0, want_pred=True, seed=5, workers=0):
    """svt_hip_decode_intra_device on fresh buffers whose outputs start as junk; everything back on the host"""
    lib = B.load()
    mi = np.ascontiguousarray(mi)
    lf_t, q_t, emap_t = dev(mi.view(np.uint8)), dev(np.ascontiguousarray(q)), dev(np.ascontiguousarray(emap).view(np.int16))
    predb = torch.full((W * H * 3 // 2,), 0x3C, dtype=torch.uint8, device="cuda")
    rec = M.RefPic(W, H)
    rec.buf[:] = np.random.default_rng(1000 + seed).integers(0, 256, rec.buf.size, dtype=np.uint8)      # a recycled buffer holds junk
    rec_t = dev(rec.buf)
    lfm_t = torch.full((T.n_sb(W, H) * 160,), 0x77, dtype=torch.uint8, device="cuda")
    nz_t = torch.full((mi.size,), 7, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), JUNK, dtype=torch.int32, device="cuda")
    p = B.EncdecPicture()
    p.d_lf_mi = lf_t.data_ptr()
    if want_pred:
        base = predb.data_ptr()
        p.pred.y, p.pred.u, p.pred.v = base, base + W * H, base + W * H + (W // 2) * (H // 2)
        p.pred.y_stride, p.pred.uv_stride, p.pred.width, p.pred.height = W, W // 2, W, H
    p.recon = rec.desc(rec_t.data_ptr())
    p.d_qcoeff, p.d_eob_map, p.d_lfm, p.d_nz, p.no_pad = q_t.data_ptr(), emap_t.data_ptr(), lfm_t.data_ptr(), nz_t.data_ptr(), no_pad      # src, d_dqcoeff, d_mc_mi: NULL
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, 1, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        if workers:
            B.check(lib.svt_hip_ctx_set_intra_workgroups(ctx, workers))
        B.check(lib.svt_hip_decode_intra_device(ctx, work, C.byref(p), W, H, mi.shape[1], q_index, C.byref(thr) if thr is not None else None, M.PAD, M.PAD,
                                                C.c_void_p(status.data_ptr())))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        rc = lib.svt_hip_encdec_work_status(ctx, work, None)
    finally:
        B.check(lib.svt_hip_ctx_set_intra_workgroups(ctx, 0))
        lib.svt_hip_encdec_work_destroy(ctx, work)
    return dict(rc=rc, status=status.cpu().numpy().view(np.uint32), pred=predb.cpu().numpy(), rec=rec_t.cpu().numpy(), rec_init=rec.buf, refpic=rec, q=q_t.cpu().numpy(),
                emap=emap_t.cpu().numpy().view(np.uint16), lfm=lfm_t.cpu().numpy(), lf=lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(mi.shape),
                nz=nz_t.cpu().numpy())


def same_picture(rec, d_rec, d_init, g_rec, padded):
    """the reconstruction equals the encode pass's: padded -- every plane with its padding, the buffer's tail untouched; not padded -- the
    interiors, and every byte outside them as the decode pass found it"""
    if padded:
        for name, a, b in zip("yuv", rec.planes(d_rec), rec.planes(g_rec)):
            assert a.tobytes() == b.tobytes(), ("reconstruction plane with its padding", name, int(np.count_nonzero(a != b)))
        end = rec.v_base + rec.cpw * rec.cph
        assert np.array_equal(d_rec[end:], d_init[end:]), "buffer tail"
        return
    for name, a, b in zip("yuv", rec.interior(d_rec), rec.interior(g_rec)):
        assert np.array_equal(a, b), ("reconstruction", name, int(np.count_nonzero(a != b)))
    outside = np.ones(d_rec.size, bool)
    for plane in rec.interior(outside):
        plane[:] = False
    assert np.array_equal(d_rec[outside], d_init[outside]), "bytes outside the planes' interiors"


def decode_equals_encode(ctx, name, skip_as_coded=True, want_pred=True, workers=0, g=None, grid=None, q=None, emap=None):
    """the case's grid (skip flags as coded, or all 0), qcoeff and eob map through the decode pass: every output equals the encode pass's"""
    _, mi_in, W, H, q_index, cfg = inputs_of(name)
    g = encoded(ctx, name) if g is None else g
    flags = flags_of(**cfg)
    lf = np.array(g["lf"] if grid is None else grid)
    if not skip_as_coded:
        lf["skip"][:, :W // 8] = 0
    q, emap = g["q"] if q is None else q, g["emap"] if emap is None else emap
    d = run_decode(ctx, W, H, lf, q, emap, q_index, thresholds() if flags.apply_loop_filter else None, no_pad=0 if flags.pad_reference else 1, want_pred=want_pred,
                   seed=len(name), workers=workers)
    assert d["rc"] == 0, "svt_hip_encdec_work_status"
    assert d["status"][0] == 0 and (d["status"][1:] == JUNK).all(), d["status"]
    assert np.array_equal(d["pred"], g["pred"]) if want_pred else (d["pred"] == 0x3C).all(), "prediction"
    same_picture(d["refpic"], d["rec"], d["rec_init"], g["rec"], bool(flags.pad_reference))
    assert np.array_equal(d["lf"]["skip"][:, :W // 8], g["lf"]["skip"][:, :W // 8]), "skip flags"
    for f in ("sb_type", "tx_size", "is_inter", "filter_level", "pad"):
        assert np.array_equal(d["lf"][f], lf[f]), f
    assert d["lf"][:, W // 8:].tobytes() == lf[:, W // 8:].tobytes()                                  # (a wider grid: nothing written beyond the picture's units)
    if flags.apply_loop_filter:
        assert masks_equal(d["lfm"].view(B.LF_MASK_DTYPE), g["lfm"].view(B.LF_MASK_DTYPE)), "loop-filter masks"
    else:
        assert (d["lfm"] == 0x77).all()
    assert np.array_equal(d["q"], q) and np.array_equal(d["emap"], emap), "the inputs stay"
    return d


# ---------------------------------------------------------------------------------------------------------------------------------------
# the first thing to run on a device: one cell
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_cell_picture(ctx):
    """16x16: one cell per plane, three tickets, nothing to wait for"""
    decode_equals_encode(ctx, "thin_16x16")


@pytest.mark.parametrize("skip_as_coded", [True, False])
@pytest.mark.parametrize("name", [s[0] for s in FIXTURE_SPECS])
def test_fixture_pictures(ctx, name, skip_as_coded):
    """every case of tests/golden/intra_reference.npz as a key frame: thin pictures (cell grids 1x1 .. 7x2), q 0 / 1 / 254 / 255 on synthetic contents"""
    decode_equals_encode(ctx, name, skip_as_coded)


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("name", [n for n in GOLD if n.startswith("thin_")])
def test_thin_pictures_on_few_workers(ctx, name, n):
    decode_equals_encode(ctx, name, workers=n)


@pytest.mark.parametrize("skip_as_coded", [True, False])
@pytest.mark.parametrize("name", [s[0] for s in SINGLE_MODE_SPECS])
def test_single_mode(ctx, name, skip_as_coded):
    decode_equals_encode(ctx, name, skip_as_coded)


@pytest.mark.parametrize("skip_as_coded", [True, False])
@pytest.mark.parametrize("name", [s[0] for s in MIXED_SIZE_SPECS + SOFT_SPECS])
def test_mixed_block_sizes(ctx, name, skip_as_coded):
    """4x4 .. 32x32 in one picture at three q indexes; a grid wider than the picture; thr NULL (not deblocked); no_pad (not padded)"""
    decode_equals_encode(ctx, name, skip_as_coded)


@pytest.mark.parametrize("n", [1, 3, 16, 100000])
def test_worker_cap_does_not_change_the_result(ctx, n):
    decode_equals_encode(ctx, "all_320x192_q200", workers=n)


def test_prediction_planes_may_be_null(ctx):
    decode_equals_encode(ctx, "all_320x192_q40", want_pred=False)


# the shortcut classes of rc_block_body among DCT_DCT blocks: (lowest eob, highest eob) per transform size
CLASSES = {4: ((1, 1), (2, 16)), 8: ((1, 1), (2, 12), (13, 64)), 16: ((1, 1), (2, 10), (11, 38), (39, 256)), 32: ((1, 1), (2, 34), (35, 135), (136, 1024))}


def test_every_shortcut_class_occurs_among_the_cases(ctx):
    """a condition on the INPUTS, taken from the eob maps the decode runs above really consume (the encode pass's, cached by `encoded`; the
    seeds and q indexes were picked on the CPU with encdec_model.oracle_intra_picture, to which the encode pass is pinned): over the union of
    the cases, the DCT_DCT blocks of each size hold every eob class the inverse transform distinguishes, and every size below 32 has an ADST
    block with coefficients.  (The exact thresholds are pinned for the shared body by tests/test_gpu_decode.py.)"""
    seen, adst = set(), set()
    for name in BY_NAME:
        src, mi, W, H, q, cfg = inputs_of(name)
        emap = encoded(ctx, name)["emap"]
        for plane, x0, y0, n, tt, ei, off in block_table(mi[:, :W // 8], W, H):
            e = int(emap[ei])
            if e and tt:
                adst.add(n)
            if e and not tt:
                seen |= {(n, k) for k, (lo, hi) in enumerate(CLASSES[n]) if lo <= e <= hi}
    missing = [(n, c) for n, cl in CLASSES.items() for k, c in enumerate(cl) if (n, k) not in seen]
    assert not missing, missing
    assert adst >= {4, 8, 16}, adst


# ---------------------------------------------------------------------------------------------------------------------------------------
# overflow
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_overflow_count_of_a_constructed_key_frame(ctx):
    """q index 255, coefficients of +-32767 among small ones at the blocks given a non-zero eob (every second block; the others hold
    coefficients too, which are not read): status[0] is numpy's count (tests/decode_model.py: dequantise), on 1 and on 16 workers the same planes"""
    W, H, q_index = 64, 40, 255
    rng = np.random.default_rng(91)
    mi = M.gen_intra_grid(7, W, H, sizes=ALL)
    table = block_table(mi, W, H)
    assert {b[3] for b in table} == {4, 8, 16, 32}
    q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
    emap = np.zeros(M.eob_map_offsets(W, H)[3], np.uint16)
    coded = np.zeros(len(table), dtype=[("tx_size", np.uint8), ("coeff_off", np.uint32), ("qtab", np.uint8)])
    n_coded = 0
    for k, (plane, x0, y0, n, tt, ei, off) in enumerate(table):
        c = rng.integers(-40, 41, n * n)
        big = rng.random(n * n) < 0.3
        c[big] = rng.choice((-32767, 32767), int(big.sum()))
        q[off:off + n * n] = c
        if k % 2 == 0:
            emap[ei] = n * n
            coded[n_coded] = ({4: 0, 8: 1, 16: 2, 32: 3}[n], off, 1 if plane else 0)
            n_coded += 1
    want = D.dequantise(q, coded[:n_coded], D.qindex_tables(q_index))[1]
    assert want > 500                                                       # (the input is what it was built to be: plenty of overflowing products)
    a = run_decode(ctx, W, H, mi, q, emap, q_index, thresholds(), workers=1)
    b = run_decode(ctx, W, H, mi, q, emap, q_index, thresholds(), workers=16)
    for d in (a, b):
        assert d["rc"] == 0 and int(d["status"][0]) == want and (d["status"][1:] == JUNK).all(), (d["status"], want)
    assert np.array_equal(a["rec"], b["rec"]) and np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["lf"], b["lf"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# inter pictures with intra leaves
# ---------------------------------------------------------------------------------------------------------------------------------------
MIXED = [(256, 192, 2, 160, dict(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=0, loop_filter=1)),
         (200, 136, 3, 120, dict(enc_mode=8, tune=1, temporal_layer_index=2, is_used_as_reference=1, recon_file=0, loop_filter=1)),   # reconstructed, not deblocked
         (136, 72, 2, 200, dict(enc_mode=8, tune=1, temporal_layer_index=4, is_used_as_reference=0, recon_file=1, loop_filter=1))]    # deblocked, not padded
_mixed = {}


def mixed_encoded(ctx, k, pure=()):
    """configuration k of test_gpu_encdec.py::test_intra_blocks_inside_inter_pictures through svt_hip_encdec_batch_device with has_intra = 1
    (pictures listed in `pure` keep their inter-only grid); once, downloaded, left unchanged"""
    if (k, pure) in _mixed:
        return _mixed[k, pure]
    lib = B.load()
    W, H, n, q_index, cfg = MIXED[k]
    srcs, refs, me = make_inputs(W, H, n, seed=W + n + 1)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    grids, n_intra = [], 0
    for i, m in enumerate(me):
        mc, lf = md_host(m, W, H, 300, level)
        if i not in pure:
            lf, mc, cnt = M.make_mixed(50 + i, lf, mc, share=0.3, level=level)
            n_intra += cnt
        grids.append((mc, lf))
    assert n_intra > 10
    flags, thr = flags_of(**cfg), thresholds()
    assert flags.do_recon
    rng = np.random.default_rng(6)
    pic, nco = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
    slab_src, slab_pred = torch.zeros(n * pic, dtype=torch.uint8, device="cuda"), torch.zeros(n * pic, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(n * nco, dtype=torch.int16, device="cuda"), torch.zeros(n * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    rec_inits = [M.RefPic(W, H) for _ in range(n)]
    for r in rec_inits:
        r.buf[:] = rng.integers(0, 256, r.buf.size, dtype=np.uint8)
    dp = [DevPicture(W, H, srcs[i], refs_dev, grids[i][0], grids[i][1], slab_src, slab_pred, slab_q, slab_dq, i, rec_inits[i]) for i in range(n)]
    arr = (B.EncdecPicture * n)(*[d.struct(refs, has_intra=1) for d in dp])
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_encdec_batch_device(ctx, work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
        cnt = (C.c_int32 * 8)()
        B.check(lib.svt_hip_encdec_work_status(ctx, work, cnt))
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    pics = [dict(lf=d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8), mc=d.mc_t.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8),
                 q=d.q_t.cpu().numpy(), emap=d.emap_t.cpu().numpy().view(np.uint16), pred=d.pred_t.cpu().numpy(), rec=d.rec_t.cpu().numpy(),
                 lfm=d.lfm_t.cpu().numpy().view(B.LF_MASK_DTYPE), has_intra=int(i not in pure)) for i, d in enumerate(dp)]
    _mixed[k, pure] = dict(W=W, H=H, q_index=q_index, flags=flags, thr=thr, refs=refs, refs_dev=refs_dev, pics=pics, counts=list(cnt))
    return _mixed[k, pure]


class MixedBuffers:
    """fresh device buffers of a batch for the decode pass, filled with the encode pass's grids, coefficients and eob maps; outputs start as junk"""

    def __init__(self, enc, skip_as_coded=True):
        W, H = enc["W"], enc["H"]
        pic, nco, n = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS, len(enc["pics"])
        self.W, self.H = W, H
        self.slab_pred = torch.full((n * pic,), 0x3C, dtype=torch.uint8, device="cuda")
        self.slab_q = torch.zeros(n * nco, dtype=torch.int16, device="cuda")
        rng = np.random.default_rng(9)
        self.items = []
        for i, p in enumerate(enc["pics"]):
            lf = p["lf"].copy()
            if not skip_as_coded:
                lf["skip"] = 0
            self.slab_q[i * nco:(i + 1) * nco].copy_(torch.from_numpy(p["q"]))
            rec = M.RefPic(W, H)
            rec.buf[:] = rng.integers(0, 256, rec.buf.size, dtype=np.uint8)
            self.items.append(dict(lf_in=lf, lf_t=dev(lf.view(np.uint8)), mc_t=dev(p["mc"].view(np.uint8)), emap_t=dev(p["emap"].view(np.int16)), rec=rec, rec_t=dev(rec.buf),
                                   rec_init=rec.buf.copy(), lfm_t=torch.full((T.n_sb(W, H) * 160,), 0x77, dtype=torch.uint8, device="cuda"),
                                   nz_t=torch.full((lf.size,), 7, dtype=torch.uint8, device="cuda"), pred_t=self.slab_pred[i * pic:(i + 1) * pic],
                                   q_t=self.slab_q[i * nco:(i + 1) * nco]))
        self.status = torch.full((4,), JUNK, dtype=torch.int32, device="cuda")

    def structs(self, enc, has_intra=None):
        W, H, out = self.W, self.H, []
        for i, it in enumerate(self.items):
            p = B.EncdecPicture()
            p.d_mc_mi, p.d_lf_mi = it["mc_t"].data_ptr(), it["lf_t"].data_ptr()
            base = it["pred_t"].data_ptr()
            p.pred.y, p.pred.u, p.pred.v = base, base + W * H, base + W * H + (W // 2) * (H // 2)
            p.pred.y_stride, p.pred.uv_stride, p.pred.width, p.pred.height = W, W // 2, W, H
            p.recon = it["rec"].desc(it["rec_t"].data_ptr())
            for l in range(2):
                p.ref[l] = enc["refs"][l].desc(enc["refs_dev"][l].data_ptr())
            p.d_qcoeff, p.d_eob_map = it["q_t"].data_ptr(), it["emap_t"].data_ptr()
            p.d_lfm, p.d_nz, p.use_subpel = it["lfm_t"].data_ptr(), it["nz_t"].data_ptr(), 1
            p.has_intra = enc["pics"][i]["has_intra"] if has_intra is None else has_intra[i]
            p.no_pad = 0 if enc["flags"].pad_reference else 1
            out.append(p)
        return (B.EncdecPicture * len(out))(*out)


def mixed_decode(ctx, enc, bufs, arr):
    lib = B.load()
    n, W, H = len(enc["pics"]), enc["W"], enc["H"]
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_decode_mixed_batch_device(ctx, work, n, arr, W, H, W // 8, enc["q_index"], C.byref(enc["thr"]) if enc["flags"].apply_loop_filter else None,
                                                      M.PAD, M.PAD, C.c_void_p(bufs.status.data_ptr())))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        cnt = (C.c_int32 * 8)()
        rc = lib.svt_hip_encdec_work_status(ctx, work, cnt)
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    return rc, list(cnt)


def mixed_equal(enc, bufs):
    W, H = enc["W"], enc["H"]
    st = bufs.status.cpu().numpy().view(np.uint32)
    assert st[0] == 0 and (st[1:] == JUNK).all()
    for it, p in zip(bufs.items, enc["pics"]):
        assert np.array_equal(it["pred_t"].cpu().numpy(), p["pred"]), "prediction (inter blocks from MC, intra blocks from the wavefront kernel)"
        same_picture(it["rec"], it["rec_t"].cpu().numpy(), it["rec_init"], p["rec"], bool(enc["flags"].pad_reference))
        lf = it["lf_t"].cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
        assert np.array_equal(lf["skip"], p["lf"]["skip"]), "skip flags"
        for f in ("sb_type", "tx_size", "is_inter", "filter_level", "pad"):
            assert np.array_equal(lf[f], p["lf"][f]), f
        if enc["flags"].apply_loop_filter:
            assert masks_equal(it["lfm_t"].cpu().numpy().view(B.LF_MASK_DTYPE), p["lfm"]), "loop-filter masks"
        else:
            assert (it["lfm_t"].cpu().numpy() == 0x77).all()
        assert np.array_equal(it["emap_t"].cpu().numpy().view(np.uint16), p["emap"]) and np.array_equal(it["q_t"].cpu().numpy(), p["q"])      # inputs stay


@pytest.mark.parametrize("skip_as_coded", [True, False])
@pytest.mark.parametrize("k", range(len(MIXED)))
def test_mixed_pictures(ctx, k, skip_as_coded):
    """the encode pass's grids, coefficients and eob maps of inter pictures with a share of intra leaves -> svt_hip_decode_mixed_batch_device:
    planes, padding, skip flags and masks equal; thr and no_pad follow the configuration's flags"""
    enc = mixed_encoded(ctx, k)
    assert all((p["lf"]["is_inter"] == 0).any() and (p["lf"]["is_inter"] == 1).any() for p in enc["pics"])
    bufs = MixedBuffers(enc, skip_as_coded)
    rc, cnt = mixed_decode(ctx, enc, bufs, bufs.structs(enc))
    assert rc == 0 and cnt == enc["counts"]
    mixed_equal(enc, bufs)


def test_batch_of_a_mixed_and_a_pure_inter_picture(ctx):
    """picture 1 holds inter leaves only and arrives with has_intra = 0: the wavefront kernel runs for picture 0 alone"""
    enc = mixed_encoded(ctx, 2, pure=(1,))
    assert (enc["pics"][1]["lf"]["is_inter"] == 1).all() and [p["has_intra"] for p in enc["pics"]] == [1, 0]
    bufs = MixedBuffers(enc)
    rc, cnt = mixed_decode(ctx, enc, bufs, bufs.structs(enc))
    assert rc == 0 and cnt == enc["counts"]
    mixed_equal(enc, bufs)


def test_intra_leaf_in_a_picture_flagged_inter_only_is_reported(ctx):
    """has_intra = 0 on a picture whose grid holds intra leaves: svt_hip_decode_mixed_batch_device reports it, like svt_hip_decode_batch_device"""
    lib = B.load()
    enc = mixed_encoded(ctx, 2)
    bufs = MixedBuffers(enc)
    n, W, H = len(enc["pics"]), enc["W"], enc["H"]
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_decode_mixed_batch_device(ctx, work, n, bufs.structs(enc, has_intra=[1, 0]), W, H, W // 8, enc["q_index"], C.byref(enc["thr"]), M.PAD, M.PAD,
                                                      C.c_void_p(bufs.status.data_ptr())))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) != 0
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0            # (the flag is cleared by the call that reports it)
        # the inter-only entry still refuses the flag, before anything is launched
        assert lib.svt_hip_decode_batch_device(ctx, work, n, bufs.structs(enc), W, H, W // 8, enc["q_index"], C.byref(enc["thr"]), M.PAD, M.PAD,
                                               C.c_void_p(bufs.status.data_ptr())) == -4
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)


# ---------------------------------------------------------------------------------------------------------------------------------------
# packets to a key frame
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_packet_of_a_key_frame_back_to_the_encode_pass_planes(ctx):
    """intra encode pass -> tokeniser -> key-frame mode info -> bool coder -> frame on one stream; the arena copied to the host, the packet
    read by svt_hip_frame_read_host: its grid, coefficients and eob map equal the device buffers; uploaded into fresh buffers,
    svt_hip_decode_intra_device returns the encode pass's prediction, planes with their padding, skip flags and masks"""
    lib = B.load()
    W, H, q_index = 136, 72, 120
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 1)
    src = T.gen_yuv(W, H, 2)
    mi = M.gen_intra_grid(32, W, H, sizes=ALL, filter_level=level)
    assert set(np.unique(mi["sb_type"])) == {0, 3, 6, 9}
    srcb = dev(np.concatenate([p.ravel() for p in src]))
    predb = torch.zeros_like(srcb)
    nco = T.n_sb(W, H) * B.SB_COEFFS
    q_t, dq_t = torch.zeros(nco, dtype=torch.int16, device="cuda"), torch.zeros(nco, dtype=torch.int16, device="cuda")
    rec = M.RefPic(W, H)
    rec_t, lf_t = dev(rec.buf), dev(np.ascontiguousarray(mi).view(np.uint8))
    emap_t = torch.full((M.eob_map_offsets(W, H)[3],), 77, dtype=torch.int16, device="cuda")
    lfm_t, nz_t = torch.zeros(T.n_sb(W, H) * 160, dtype=torch.uint8, device="cuda"), torch.full((mi.size,), 7, dtype=torch.uint8, device="cuda")

    def tight(base):
        d = B.YuvPlanes()
        d.y, d.u, d.v = base, base + W * H, base + W * H + (W // 2) * (H // 2)
        d.y_stride, d.uv_stride, d.width, d.height = W, W // 2, W, H
        return d
    p = B.EncdecPicture()
    p.d_lf_mi, p.src, p.pred, p.recon = lf_t.data_ptr(), tight(srcb.data_ptr()), tight(predb.data_ptr()), rec.desc(rec_t.data_ptr())
    p.d_qcoeff, p.d_dqcoeff, p.d_eob_map, p.d_lfm, p.d_nz = q_t.data_ptr(), dq_t.data_ptr(), emap_t.data_ptr(), lfm_t.data_ptr(), nz_t.data_ptr()
    flags, thr = flags_of(**KEY), thresholds()
    head = FM.host_header_bytes(FM.params(width=W, height=H, base_qindex=q_index, filter_level=level))
    tb, mb = TokBuffers(W, H, counts=False), ModesBuffers(W, H)
    tile = Tile(W, H, tb, mb)
    arena, packets = frame_batch(ctx, [tile], [head])
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, 1, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_encdec_intra_device(ctx, work, C.byref(p), W, H, W // 8, q_index, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
        tokenize_device(ctx, W, H, [(lf_t, q_t, emap_t)], [tb])
        modes_device(ctx, W, H, [(lf_t, emap_t, tb.tok_off)], [mb])
        B.check(lib.svt_hip_boolcode_batch_device(ctx, 1, (B.BoolStream * 1)(tile.struct)))
        B.check(lib.svt_hip_frame_batch_device(ctx, 1, packets, arena.address, arena.cap, arena.table.data_ptr()))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    g = dict(pred=predb.cpu().numpy(), rec=rec_t.cpu().numpy(), q=q_t.cpu().numpy(), emap=emap_t.cpu().numpy().view(np.uint16), lfm=lfm_t.cpu().numpy(),
             lf=lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(mi.shape))
    assert (g["lf"]["skip"] == 0).any() and g["emap"].any()
    data, table, _, _, _ = arena.result()
    off, size = (int(v) for v in table[0])
    packet = bytes(data[off:off + size])
    assert packet[:len(head)] == head and size > len(head)
    rc, info, r = read_frame(packet, W, H)
    assert rc == 0, lib.svt_hip_last_error()
    assert r["guards"] and (info.params.width, info.params.height, info.params.base_qindex, info.params.filter_level) == (W, H, q_index, level)
    assert r["lf_mi"].tobytes() == g["lf"].tobytes(), [f for f in g["lf"].dtype.names if not np.array_equal(r["lf_mi"][f], g["lf"][f])]
    assert np.array_equal(r["qcoeff"], g["q"]) and np.array_equal(r["eob_map"], g["emap"])
    # from the bytes alone, into fresh buffers
    d = run_decode(ctx, W, H, np.ascontiguousarray(r["lf_mi"]), np.ascontiguousarray(r["qcoeff"]), np.ascontiguousarray(r["eob_map"]), int(info.params.base_qindex),
                   thr if info.params.filter_level else None)
    assert d["rc"] == 0 and d["status"][0] == 0 and (d["status"][1:] == JUNK).all()
    assert np.array_equal(d["pred"], g["pred"]), "prediction"
    same_picture(d["refpic"], d["rec"], d["rec_init"], g["rec"], True)
    assert d["lf"].tobytes() == g["lf"].tobytes(), "grid with its skip flags"
    assert masks_equal(d["lfm"].view(B.LF_MASK_DTYPE), g["lfm"].view(B.LF_MASK_DTYPE)), "loop-filter masks"


# ---------------------------------------------------------------------------------------------------------------------------------------
# packets to a mixed inter picture
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_packets_of_mixed_inter_pictures_back_to_the_encode_pass_planes(ctx):
    """the chain of tests/test_gpu_decode.py's packet test on grids that hold intra leaves (make_mixed on the stand-in decision): encode pass
    with has_intra = 1 -> tokeniser -> labelling -> inter mode info -> bool coder -> frame, two B pictures under REFERENCE_SELECT on one
    stream; the arena copied to the host, every packet read by svt_hip_frame_read_host -- grids, coefficients and eob map equal the device
    buffers --, uploaded into fresh buffers: svt_hip_decode_mixed_batch_device returns the encode pass's prediction, planes with their
    padding, skip flags and masks"""
    lib = B.load()
    B.check(lib.svt_hip_modes_inter_set_tables(ctx, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    W, H, q_index, n = 136, 72, 120, 2
    srcs, refs, me = make_inputs(W, H, n, seed=67)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(q_index), 0)
    grids = []
    for i, m in enumerate(me):
        mc, lf = md_host(m, W, H, 300, level)
        lf, mc, cnt = M.make_mixed(50 + i, lf, mc, share=0.3, level=level)
        assert cnt > 3
        grids.append((mc, lf))
    assert any((lf["sb_type"] == 0).any() for _, lf in grids), "a unit of four 4x4 intra blocks"
    fr, lrf = IM.frame(**IM.B_PICTURE), (IM.LAST, IM.ALTREF)
    fp = FM.inter(width=W, height=H, reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1), base_qindex=q_index, filter_level=level,
                  frame_parallel_decoding_mode=1)
    head = FM.host_header_bytes(fp)
    pic, nco = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS
    slab_src, slab_pred = torch.zeros(n * pic, dtype=torch.uint8, device="cuda"), torch.zeros(n * pic, dtype=torch.uint8, device="cuda")
    slab_q, slab_dq = torch.zeros(n * nco, dtype=torch.int16, device="cuda"), torch.zeros(n * nco, dtype=torch.int16, device="cuda")
    refs_dev = [dev(r.buf) for r in refs]
    dp = [DevPicture(W, H, srcs[i], refs_dev, grids[i][0], grids[i][1], slab_src, slab_pred, slab_q, slab_dq, i, M.RefPic(W, H)) for i in range(n)]
    arr = (B.EncdecPicture * n)(*[d.struct(refs, has_intra=1) for d in dp])
    flags, thr = flags_of(**KEY), thresholds()
    tbs, vbs, mbs = [TokBuffers(W, H, counts=False) for _ in dp], [MdBuffers(W, H, want_cand=False) for _ in dp], [InterBuffers(W, H) for _ in dp]
    tiles = [Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]
    arena, packets = frame_batch(ctx, tiles, [head] * n)
    metas = [dict(W=W, H=H, frame=fr, restrict=rs, lrf=lrf) for rs in (0, 1)]
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        B.check(lib.svt_hip_encdec_batch_device(ctx, work, n, arr, W, H, W // 8, q_index, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
        tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t) for d in dp], tbs)
        md_device(ctx, W, H, [vb.struct((d.lf_t, d.mc_t), m, ref_mask=0) for vb, d, m in zip(vbs, dp, metas)])
        inter_modes_device(ctx, W, H, [((d.lf_t, d.mc_t, vb.ext), d.emap_t, tb.tok_off, fr) for d, vb, tb in zip(dp, vbs, tbs)], mbs)
        B.check(lib.svt_hip_boolcode_batch_device(ctx, n, (B.BoolStream * n)(*[t.struct for t in tiles])))
        B.check(lib.svt_hip_frame_batch_device(ctx, n, packets, arena.address, arena.cap, arena.table.data_ptr()))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        cnt = (C.c_int32 * 8)()
        assert lib.svt_hip_encdec_work_status(ctx, work, cnt) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    data, table, _, _, _ = arena.result()
    pics = []
    for i, (d, vb, m) in enumerate(zip(dp, vbs, metas)):
        got = vb.result()
        assert got["guards"] and got["status"][2] == 0, got["status"]                     # every NEWMV leaf codable faithfully
        g = dict(lf=d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8), mc=d.mc_t.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8),
                 q=d.q_t.cpu().numpy(), emap=d.emap_t.cpu().numpy().view(np.uint16), pred=d.pred_t.cpu().numpy(), rec=d.rec_t.cpu().numpy(),
                 lfm=d.lfm_t.cpu().numpy().view(B.LF_MASK_DTYPE))
        assert (g["lf"]["is_inter"] == 0).any() and (g["lf"]["is_inter"] == 1).any()
        off, size = (int(v) for v in table[i])
        packet = bytes(data[off:off + size])
        assert packet[:len(head)] == head and size > len(head)
        rc, info, r = read_frame(packet, W, H, restrict=m["restrict"], lrf=lrf)
        assert rc == 0, lib.svt_hip_last_error()
        assert r["guards"] and r["res"]["past_end"] == 0
        assert 0 < r["res"]["inter_leaves"] < r["res"]["leaves"], "inter and intra leaves in one picture"
        assert r["lf_mi"].tobytes() == g["lf"].tobytes(), [f for f in g["lf"].dtype.names if not np.array_equal(r["lf_mi"][f], g["lf"][f])]
        inter = g["lf"]["is_inter"] == 1
        for f in g["mc"].dtype.names:                                                      # (the MC records of inter leaves: what the prediction reads)
            assert np.array_equal(r["mc_mi"][f][inter], g["mc"][f][inter]), f
        assert np.array_equal(r["qcoeff"], g["q"]) and np.array_equal(r["eob_map"], g["emap"])
        # from the bytes alone
        pics.append(dict(g, lf=np.ascontiguousarray(r["lf_mi"]), mc=np.ascontiguousarray(r["mc_mi"]), q=np.ascontiguousarray(r["qcoeff"]),
                         emap=np.ascontiguousarray(r["eob_map"]), has_intra=1))
    enc = dict(W=W, H=H, q_index=q_index, flags=flags, thr=thr, refs=refs, refs_dev=refs_dev, pics=pics, counts=list(cnt))
    bufs = MixedBuffers(enc)
    rc, got_cnt = mixed_decode(ctx, enc, bufs, bufs.structs(enc))
    assert rc == 0 and got_cnt == enc["counts"]
    mixed_equal(enc, bufs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals and malformed grids
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    """null fields, misaligned planes, geometry that differs from the workspace, q 256, null status: non-zero, every buffer as it was"""
    lib = B.load()
    W, H = 64, 40
    mi = M.gen_intra_grid(3, W, H, sizes=ALL)
    lf_t = dev(np.ascontiguousarray(mi).view(np.uint8))
    q_t = torch.full((T.n_sb(W, H) * B.SB_COEFFS,), 3, dtype=torch.int16, device="cuda")
    emap_t = torch.full((M.eob_map_offsets(W, H)[3],), 1, dtype=torch.int16, device="cuda")
    predb = torch.full((W * H * 3 // 2,), 0x3C, dtype=torch.uint8, device="cuda")
    rec = M.RefPic(W, H, fill=0x42)
    rec_t = dev(rec.buf)
    lfm_t, nz_t = torch.full((T.n_sb(W, H) * 160,), 0x77, dtype=torch.uint8, device="cuda"), torch.full((mi.size,), 7, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), JUNK, dtype=torch.int32, device="cuda")
    thr = thresholds()

    def pic():
        p = B.EncdecPicture()
        p.d_lf_mi = lf_t.data_ptr()
        base = predb.data_ptr()
        p.pred.y, p.pred.u, p.pred.v, p.pred.y_stride, p.pred.uv_stride, p.pred.width, p.pred.height = base, base + W * H, base + W * H + (W // 2) * (H // 2), W, W // 2, W, H
        p.recon = rec.desc(rec_t.data_ptr())
        p.d_qcoeff, p.d_eob_map, p.d_lfm, p.d_nz = q_t.data_ptr(), emap_t.data_ptr(), lfm_t.data_ptr(), nz_t.data_ptr()
        return p
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, 1, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        def rc(p, w=W, h=H, stride=W // 8, q=100, t=thr, st=status.data_ptr(), wk=work, c=ctx):
            return lib.svt_hip_decode_intra_device(c, wk, C.byref(p) if p is not None else None, w, h, stride, q, C.byref(t) if t is not None else None, M.PAD, M.PAD,
                                                   C.c_void_p(st) if st else None)
        for field in ("d_lf_mi", "d_qcoeff", "d_eob_map", "d_nz", "d_lfm"):
            p = pic()
            setattr(p, field, None)
            assert rc(p) != 0, field
        for plane in "yuv":
            p = pic()
            setattr(p.recon, plane, None)
            assert rc(p) != 0, plane
        p = pic(); p.pred.u = None
        assert rc(p) != 0                                                       # prediction planes: all or none
        p = pic(); p.recon.y += 1
        assert rc(p) != 0                                                       # planes: 4-byte aligned
        p = pic(); p.recon.uv_stride += 2
        assert rc(p) != 0                                                       # strides too
        p = pic(); p.pred.v += 2
        assert rc(p) != 0
        p = pic(); p.d_qcoeff += 2
        assert rc(p) != 0                                                       # coefficients: 16-byte aligned
        assert rc(pic(), w=W + 8) != 0 and rc(pic(), h=H - 8) != 0 and rc(pic(), stride=W // 8 - 1) != 0
        assert rc(pic(), q=256) != 0 and rc(pic(), q=-1) != 0 and rc(pic(), st=None) != 0 and rc(None) != 0 and rc(pic(), wk=None) != 0 and rc(pic(), c=None) != 0
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    assert (status.cpu().numpy().view(np.uint32) == JUNK).all() and (predb.cpu().numpy() == 0x3C).all() and (rec_t.cpu().numpy() == 0x42).all()
    assert (lfm_t.cpu().numpy() == 0x77).all() and (nz_t.cpu().numpy() == 7).all() and lf_t.cpu().numpy().tobytes() == np.ascontiguousarray(mi).tobytes()


def test_mixed_entry_refusals(ctx):
    """the mixed entry refuses what the inter entry refuses, and misaligned planes of a picture with has_intra"""
    lib = B.load()
    enc = mixed_encoded(ctx, 2)
    bufs = MixedBuffers(enc)
    n, W, H = len(enc["pics"]), enc["W"], enc["H"]
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    torch.cuda.synchronize()
    try:
        def rc(arr, count=n, w=W, q=enc["q_index"], st=bufs.status.data_ptr()):
            return lib.svt_hip_decode_mixed_batch_device(ctx, work, count, arr, w, H, W // 8, q, C.byref(enc["thr"]), M.PAD, M.PAD, C.c_void_p(st) if st else None)
        ok = bufs.structs(enc)
        for field in ("d_mc_mi", "d_lf_mi", "d_qcoeff", "d_eob_map", "d_lfm", "d_nz"):
            arr = bufs.structs(enc)
            setattr(arr[1], field, None)
            assert rc(arr) != 0, field
        arr = bufs.structs(enc)
        arr[0].recon.y += 2
        assert rc(arr) != 0
        assert rc(ok, count=0) != 0 and rc(ok, w=W + 8) != 0 and rc(ok, q=256) != 0 and rc(ok, st=None) != 0 and rc(None) != 0
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    finally:
        lib.svt_hip_encdec_work_destroy(ctx, work)
    assert (bufs.status.cpu().numpy().view(np.uint32) == JUNK).all() and (bufs.slab_pred.cpu().numpy() == 0x3C).all()
    for it in bufs.items:
        assert np.array_equal(it["rec_t"].cpu().numpy(), it["rec_init"]) and (it["lfm_t"].cpu().numpy() == 0x77).all() and (it["nz_t"].cpu().numpy() == 7).all()


def test_a_64x64_intra_block_terminates_and_is_reported(ctx):
    W, H = 128, 64
    mi = M.gen_intra_grid(3, W, H)
    mi["sb_type"][0:8, 0:8], mi["tx_size"][0:8, 0:8] = 12, 3            # outside this entry, as in the encode pass
    q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
    emap = np.ones(M.eob_map_offsets(W, H)[3], np.uint16)
    d = run_decode(ctx, W, H, mi, q, emap, 100, thresholds())
    assert d["rc"] != 0
    assert d["status"][0] == 0 and (d["status"][1:] == JUNK).all()

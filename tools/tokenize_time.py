#!/usr/bin/env python3
"""Times svt_hip_tokenize_batch_device on 16 pictures of 2160p as the encode pass leaves them (md_default grids, q index 160), counts on
and off, and beside it -- same process, alternating -- svt_hip_coeff_rate_batch_device over the same transform blocks (their
descriptors are read back from the tokeniser's own output: a block's first record names its size, plane type, inter flag and context).
Device events around each call (svt_hip_last_kernel_ms); warm-ups, then the median of --reps calls with min / max.

    python tools/tokenize_time.py [--pics 16] [--reps 25] [--save picture.npz]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                     # noqa: E402
import encdec_model as M         # noqa: E402
import me_configs as MC          # noqa: E402
import svt_testlib as T          # noqa: E402
import tokenize_model as TM      # noqa: E402
import test_gpu_tokenize as G    # noqa: E402

B = T.B
W, H, Q_INDEX = 3840, 2160, 160


def clip(n):
    """n + 2 pictures: one gen_yuv picture drifting by (1, 2) samples per picture, with a little noise"""
    y, _, _ = T.gen_yuv(W, H, 7)
    rng = np.random.default_rng(1)
    out = []
    for k in range(n + 2):
        f = np.roll(y, (k, 2 * k), axis=(0, 1)).astype(np.int16) + rng.integers(-2, 3, y.shape, dtype=np.int16)
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


def rate_blocks(res, lf, emap, pic, nco):
    """svt_rate_block records of the coded transform blocks of one picture from the tokeniser's output"""
    idx = np.nonzero(res["tok_off"] != TM.NO_OFFSET)[0]
    first = res["tokens_all"][res["tok_off"][idx]]
    row = (first >> 4) & 0xFFF
    ts, ptype, inter, ctx = row // 144, (row // 72) % 2, (row // 36) % 2, row % 6
    w4, h4 = W // 4, H // 4
    e1, e2 = w4 * h4, w4 * h4 + (w4 // 2) * (h4 // 2)
    plane = (idx >= e1).astype(np.int64) + (idx >= e2)
    local = idx - np.array([0, e1, e2])[plane]
    pw4 = np.where(plane == 0, w4, w4 // 2)
    y4, x4 = local // pw4, local % pw4
    u = np.where(plane == 0, 16, 8)
    sb = (y4 // u) * ((W + 63) // 64) + x4 // u
    lx, ly, z = x4 % u, y4 % u, np.zeros_like(x4)
    for b in range(4):
        z |= ((lx >> b) & 1) << (2 * b) | ((ly >> b) & 1) << (2 * b + 1)
    offs, _ = T.rate_scan_offsets()
    blocks = np.zeros(len(idx), dtype=B.RATE_BLOCK_DTYPE)
    blocks["coeff_off"] = pic * nco + sb * B.SB_COEFFS + np.array([0, 4096, 5120])[plane] + z * 16
    blocks["scan_off"] = np.array([offs[(t, 0)] for t in range(4)])[ts]
    blocks["eob"], blocks["tx_size"], blocks["plane_type"], blocks["is_inter"], blocks["ctx"] = emap[idx], ts, ptype, inter, ctx
    return blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, default=16)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--save", default=None, help="write picture 0 (grid, coefficients, eob map) to this .npz")
    a = ap.parse_args()
    lib = B.load()
    ctx = G.new_ctx()
    n = a.pics
    frames = clip(2)            # two distinct pictures between two references, repeated to fill the batch
    refs = [M.RefPic(W, H).set_padded(frames[k], *G._chroma(frames[k], k)) for k in (0, 3)]
    pa = [T.PaPic(f) for f in frames]
    p = MC.preset("c3_2160p_m8", 2, 1)
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(Q_INDEX), 0)
    grids, srcs = [], []
    for k in (1, 2):
        res = np.zeros((T.n_sb(W, H), 85), dtype=B.ME_RESULT_DTYPE)
        dc, d0, d1 = pa[k].desc(), pa[0].desc(), pa[3].desc()
        B.check(lib.svt_hip_me_picture(ctx, C.byref(dc), C.byref(d0), C.byref(d1), C.byref(p), res.ctypes.data_as(C.c_void_p), None))
        grids.append(G.md_host(res, W, H, 300, level))
        srcs.append((frames[k],) + G._chroma(frames[k], k))
    dp, work, keep = G.encode_batch(ctx, W, H, [srcs[i & 1] for i in range(n)], refs, [grids[i & 1] for i in range(n)], Q_INDEX)
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    inputs = [(d.lf_t, d.q_t, d.emap_t) for d in dp]
    bufs_on = [G.TokBuffers(W, H) for _ in range(n)]
    bufs_off = [G.TokBuffers(W, H, counts=False) for _ in range(n)]
    torch.cuda.synchronize()

    def tok(bufs):
        G.tokenize_device(ctx, W, H, inputs, bufs)
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        return float(lib.svt_hip_last_kernel_ms(ctx))
    tok(bufs_on)
    # the same blocks for the rate kernel
    nco = T.n_sb(W, H) * B.SB_COEFFS
    all_blocks, totals = [], []
    for i in (0, 1):
        r = bufs_on[i].result()
        r["tokens_all"] = bufs_on[i].tokens.cpu().numpy().view(np.uint32)
        totals.append(int(r["sb_off"][-1]))
        lf, q, emap = G.downloaded(dp[i], W, H)
        per_pic = rate_blocks(r, lf, emap, 0, nco)
        if i == 0 and a.save:
            np.savez_compressed(a.save, lf_mi=lf.view(np.uint8), qcoeff=q, eob_map=emap, size=np.array([W, H], np.int32))
        all_blocks.append(per_pic)
    blocks = []
    for i in range(n):
        b = all_blocks[i & 1].copy()
        b["coeff_off"] += i * nco
        blocks.append(b)
    blocks = np.concatenate(blocks)
    tables, scan = T.rate_tables()
    d_blocks, d_tab, d_scan = G.dev(blocks.view(np.uint8)), G.dev(np.ascontiguousarray(tables).reshape(1).view(np.uint8)), G.dev(scan)
    d_bits = torch.zeros(len(blocks), dtype=torch.int32, device="cuda")
    q_base = keep[2].data_ptr()
    torch.cuda.synchronize()

    def rate():
        B.check(lib.svt_hip_coeff_rate_batch_device(ctx, C.c_void_p(q_base), C.c_void_p(d_blocks.data_ptr()), len(blocks), C.c_void_p(d_tab.data_ptr()),
                                                    C.c_void_p(d_scan.data_ptr()), C.c_void_p(d_bits.data_ptr())))
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        return float(lib.svt_hip_last_kernel_ms(ctx))
    for _ in range(a.warmup):
        tok(bufs_on), tok(bufs_off), rate()
    t_on, t_off, t_rate = [], [], []
    for _ in range(a.reps):
        t_on.append(tok(bufs_on)); t_rate.append(rate()); t_off.append(tok(bufs_off))
    lib.svt_hip_encdec_work_destroy(ctx, work)
    lib.svt_hip_ctx_destroy(ctx)
    stat = lambda t: dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
    tokens_batch = sum(totals[i & 1] for i in range(n))
    written = 4 * tokens_batch + n * 4 * (M.eob_map_offsets(W, H)[3] + T.n_sb(W, H) + 1)
    out = dict(pictures=n, width=W, height=H, q_index=Q_INDEX, reps=a.reps, tokens_per_picture=totals, transform_blocks=int(len(blocks)),
               tokenize_counts_on=stat(t_on), tokenize_counts_off=stat(t_off), coeff_rate=stat(t_rate),
               ratio_counts_on=round(float(np.median(t_on) / np.median(t_rate)), 3), ratio_counts_off=round(float(np.median(t_off) / np.median(t_rate)), 3),
               bytes_written=written, write_gb_per_s=round(written / (np.median(t_on) * 1e-3) / 1e9, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the MV-reference stage on a batch of 2160p B pictures, in the setup of tools/modes_inter_time.py: the clip, the motion estimation
preset and the synthesised mode decision of bench.py, the inter encode pass at the bench's q index, extension records that hold the
reference frames and a random inter mode per leaf.  Device events on the context's stream around svt_hip_mvrefs_batch_device alone
(with and without d_cand), around svt_hip_modes_inter_batch_device alone on the same pictures (reading the new stage's d_ext_out), and
around the chain svt_hip_tokenize_batch_device -> [svt_hip_mvrefs_batch_device ->] svt_hip_modes_inter_batch_device ->
svt_hip_boolcode_batch_device with and without the new stage, one call each for the whole batch.  Warm-ups, then the median of --reps
calls with min / max.  Every picture's records are compared with the host form (svt_hip_mvrefs_picture) and every tile with the host
chain, byte for byte, before a number is printed.  Prints one JSON line, with the reference's seconds for the fixture pictures on one
core from tests/golden/mvrefs_reference.npz beside it.

    python tools/mvrefs_time.py [--pics 4] [--reps 25]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import torch                      # noqa: E402
import bench                      # noqa: E402
import boolcode_model as BM       # noqa: E402
import encdec_model as M          # noqa: E402
import me_configs as MC           # noqa: E402
import modes_inter_model as IM    # noqa: E402
import modes_time as KT           # noqa: E402
import mvrefs_model as VM         # noqa: E402
import svt_testlib as T           # noqa: E402
import test_gpu_modes as GM       # noqa: E402
import test_gpu_modes_inter as GI # noqa: E402
import test_gpu_mvrefs as GV      # noqa: E402
import test_gpu_tokenize as G     # noqa: E402
import tokenize_model as TM       # noqa: E402
from test_gpu_encdec import _chroma, dev   # noqa: E402
from test_mvrefs import stripped  # noqa: E402

B = T.B
W, H, Q_INDEX = 3840, 2160, 160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, default=4)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = a.pics
    lib = B.load()
    stream = torch.cuda.Stream()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))
    B.check(lib.svt_hip_boolcode_set_tables(ctx, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(ctx, IM.tables()[1].ctypes.data_as(C.c_void_p)))

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    # the B pictures: both references, motion estimation, the bench's synthesised decision, the inter encode pass
    frames = T.gen_clip(W, H, n + 2, seed=11)
    refs = [M.RefPic(W, H).set_padded(frames[k], *_chroma(frames[k], k)) for k in (0, n + 1)]
    pa = [T.PaPic(f) for f in frames]
    preset = MC.preset("c3_2160p_m8", 2, 1)
    n_sb, nsbx, mi_rows, mi_cols = T.n_sb(W, H), (W + 63) // 64, H // 8, W // 8
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(Q_INDEX), 0)
    rng = np.random.default_rng(5)
    grids, d0, d1 = [], pa[0].desc(), pa[n + 1].desc()
    for i in range(1, n + 1):
        res = np.zeros((n_sb, 85), dtype=B.ME_RESULT_DTYPE)
        dc = pa[i].desc()
        B.check(lib.svt_hip_me_picture(ctx, C.byref(dc), C.byref(d0), C.byref(d1), C.byref(preset), res.ctypes.data_as(C.c_void_p), None))
        kinds = np.maximum(bench.partition_kinds(rng, W, H), 1)
        mc, k_cell = bench.build_mode_info(B, res, kinds, mi_rows, mi_cols, nsbx)
        grids.append((mc, bench.build_lf_mode_info(B, k_cell, mi_rows, mi_cols, level)))
    srcs = [(frames[i],) + _chroma(frames[i], i) for i in range(1, n + 1)]
    dp, work, keep = G.encode_batch(ctx, W, H, srcs, refs, grids, Q_INDEX)
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    lib.svt_hip_encdec_work_destroy(ctx, work)
    fr = IM.frame(**IM.B_PICTURE)
    exts = [stripped(dict(ext=GI.seeded_ext(mc, fr, 90 + i)))["ext"] for i, (mc, _) in enumerate(grids)]
    ext_t = [dev(e.view(np.uint8)) for e in exts]
    pic = dict(W=W, H=H, frame=fr, restrict=0)

    # the host chain on the downloaded pictures
    want_refs, want, want_tok, want_tiles, n_bools = [], [], [], [], []
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    for d, (mc, _), ext in zip(dp, grids, exts):
        lf, q, emap = G.downloaded(d, W, H)
        full = dict(pic, lf_mi=lf, mc_mi=mc, ext=ext, eob_map=emap)
        r = VM.host_mvrefs(full)
        assert r["rc"] == 0 and r["guards"] and r["status"][0] != B.MODES_BAD_GRID
        tok = TM.host_tokenize_picture(lf, q, emap, W, H, counts=False)
        m = IM.host_modes(dict(full, ext=r["ext_out"]), tok["tok_off"])
        assert m["rc"] == 0 and m["n_bools"] != B.MODES_BAD_GRID
        seg = np.ascontiguousarray(m["segments"])
        nb = m["n_bools"] + KT.count_token_bools(tok["tokens"])
        cap = int(lib.svt_hip_boolcode_capacity(nb))
        tile, size = np.zeros(cap, np.uint8), C.c_uint32()
        assert lib.svt_hip_boolcode_host(vp(BM.tables()[1]), vp(tok["tokens"]), len(tok["tokens"]), vp(m["bools"]), len(m["bools"]), vp(seg), len(seg), vp(tile), cap,
                                         C.byref(size)) == 0
        want_refs.append(r); want.append(m); want_tok.append(tok); want_tiles.append(bytes(tile[:size.value])); n_bools.append(nb)

    tbs, vbs, mbs = [G.TokBuffers(W, H, counts=False) for _ in dp], [GV.MvBuffers(W, H) for _ in dp], [GI.InterBuffers(W, H) for _ in dp]
    tiles = [GM.Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]
    for t, nb in zip(tiles, n_bools):
        t.struct.max_bools = nb + nb // 8
    torch.cuda.synchronize()
    tok_arr = (B.TokPicture * n)(*[tb.struct(d.lf_t, d.q_t, d.emap_t) for tb, d in zip(tbs, dp)])
    mv_arr = (B.MvrefsPicture * n)(*[vb.struct((d.lf_t, d.mc_t, e), pic) for vb, d, e in zip(vbs, dp, ext_t)])
    mv_lean = (B.MvrefsPicture * n)(*[vb.struct((d.lf_t, d.mc_t, e), pic, ref_mask=0) for vb, d, e in zip(vbs, dp, ext_t)])
    for s in mv_lean:
        s.d_cand = None
    mod_arr = (B.ModesInterPicture * n)(*[mb.struct((d.lf_t, d.mc_t, vb.ext), d.emap_t, tb.tok_off, fr) for mb, d, vb, tb in zip(mbs, dp, vbs, tbs)])
    bc_arr = (B.BoolStream * n)(*[t.struct for t in tiles])
    tokenize = lambda: B.check(lib.svt_hip_tokenize_batch_device(ctx, n, tok_arr, W, H, W // 8))          # noqa: E731
    mvrefs = lambda: B.check(lib.svt_hip_mvrefs_batch_device(ctx, n, mv_arr, W, H, W // 8))               # noqa: E731
    mvrefs_lean = lambda: B.check(lib.svt_hip_mvrefs_batch_device(ctx, n, mv_lean, W, H, W // 8))         # noqa: E731
    modes = lambda: B.check(lib.svt_hip_modes_inter_batch_device(ctx, n, mod_arr, W, H, W // 8))          # noqa: E731
    boolcode = lambda: B.check(lib.svt_hip_boolcode_batch_device(ctx, n, bc_arr))                         # noqa: E731

    def check_refs():
        for vb, r in zip(vbs, want_refs):
            GV.same(vb.result(), r)

    def check_tiles():
        for mb, m, t, wt in zip(mbs, want, tiles, want_tiles):
            GI.same(mb.result(), m)
            got, got_size, guard = t.result()
            assert got == wt and got_size == len(wt) and np.all(guard == GM.GUARD8), "2160p B picture: device tile differs from the host chain"
    tokenize()
    out = dict(reps=a.reps, pictures=n, q_index=Q_INDEX, width=W, height=H, inter_leaves=[r["status"][1] for r in want_refs],
               contradicting_leaves=[r["status"][0] for r in want_refs], mode_info_bools=[m["n_bools"] for m in want], tile_bytes=[len(t) for t in want_tiles])
    r_full = timed(mvrefs)
    check_refs()
    r_lean = timed(mvrefs_lean)
    check_refs()                                          # (d_cand keeps the full call's records, d_ext_out is rewritten)
    out["mvrefs_alone_ext_and_cand"], out["mvrefs_alone_ext_only"] = r_full, r_lean
    out["mode_info_alone"] = timed(modes)
    out["chain_without_mvrefs"] = timed(lambda: (tokenize(), modes(), boolcode()))
    check_tiles()
    out["chain_with_mvrefs"] = timed(lambda: (tokenize(), mvrefs_lean(), modes(), boolcode()))
    check_refs()
    check_tiles()
    g = VM.fixture()
    out["reference_one_core"] = {str(k): float(s) for k, s in zip(g["names"], g["seconds"])}
    lib.svt_hip_ctx_destroy(ctx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

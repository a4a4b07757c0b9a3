#!/usr/bin/env python3
"""Times the entropy pass on 2160p pictures as the encode pass leaves them (the set of tools/tokenize_time.py: md_default grids, q index
160, the fixture tables): svt_hip_entropy_batch_device for batches of 1 and 16, per stage through the stage hook and for the call, with
the tokens, mode bools, coded bools and tile bytes of a picture and the device bytes the workspace took under the limits the tool chose.

    python tools/entropy_time.py [--pics 1,16] [--reps 20] [--warmup 3] [--q 160] [--coef] [--separate]

--coef switches the workspace to the coefficient-update mode (svt_hip_entropy_work_set_coef_update; refresh_frame_context 0, which the
mode asks for): the stage list then holds "coef_update" between "modes" and "gate", the packets are compared with
svt_hip_entropy_picture_coef, and packet_bytes_per_picture are the frames tools/coef_update_bytes.py records as "frame, updated".
--q takes a list of q indexes; the pictures are encoded anew for each.

--separate makes the six existing stage calls over hand-allocated buffers instead (tokeniser, labelling, inter mode info, bool coder,
frame), under the same limits: it uses nothing of the entropy pass and so also runs on a commit that does not have it.

Limits.  A sizing pass runs the tokeniser alone on the two distinct pictures with the worst-case capacity (one picture at a time) and
reads the totals; max_tokens = the largest total * 5 / 4, max_bools = max_tokens * --bools-per-token + the inter mode-info capacity,
max_tile_bytes = svt_hip_boolcode_capacity(max_bools) / 8.  A picture the limits do not hold fails the run.
Device events on the context's stream (a torch stream): around the call; then, in a second series, also inside it at every hook call
(the "headers" interval is host work in front of the first launch: it holds no kernel); warm-ups, then the median of --reps calls with
min / max.  One JSON line per batch size.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                        # noqa: E402
import boolcode_model as BM         # noqa: E402
import encdec_model as M            # noqa: E402
import frame_model as FM            # noqa: E402
import me_configs as MC             # noqa: E402
import modes_inter_model as IM      # noqa: E402
import svt_testlib as T             # noqa: E402
import test_gpu_tokenize as G       # noqa: E402

B = T.B
W, H, Q_INDEX = 3840, 2160, 160
HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int32)
LRF = (IM.LAST, IM.ALTREF)


def clip(n):
    """tools/tokenize_time.py's: one gen_yuv picture drifting by (1, 2) samples per picture, with a little noise"""
    y, _, _ = T.gen_yuv(W, H, 7)
    rng = np.random.default_rng(1)
    out = []
    for k in range(n + 2):
        f = np.roll(y, (k, 2 * k), axis=(0, 1)).astype(np.int16) + rng.integers(-2, 3, y.shape, dtype=np.int16)
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


def encoded_batch(lib, ctx, n):
    frames = clip(2)
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
    return dp, work, keep, level


def sizing(lib, ctx, dp, bools_per_token):
    totals = []
    for d in dp[:2]:
        tb = G.TokBuffers(W, H, counts=False)
        torch.cuda.synchronize()
        G.tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t)], [tb])
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        totals.append(int(tb.sb_off.cpu().numpy().view(np.uint32)[-1]))
        del tb
    max_tokens = max(totals) * 5 // 4
    max_bools = max_tokens * bools_per_token + int(lib.svt_hip_modes_inter_bools_capacity(W, H))
    return totals, max_tokens, max_bools, int(lib.svt_hip_boolcode_capacity(max_bools)) // 8


def stat(t):
    return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))


def frame_params(level, coef=False):
    fp = FM.inter(width=W, height=H, reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1), base_qindex=Q_INDEX, filter_level=level,
                  frame_parallel_decoding_mode=1)
    return dict(fp, refresh_frame_context=0) if coef else fp


def driver(lib, ctx, stream, dp, level, limits, a):
    import entropy_model as E
    n = len(dp)
    max_tokens, max_bools, max_tile = limits
    lim = E.limits(W, H, n, max_tokens=max_tokens, max_bools=max_bools, max_tile_bytes=max_tile)
    fp = frame_params(level, a.coef)
    arr = (B.EntropyPicture * n)(*[E.fill_struct(B.EntropyPicture(), (d.lf_t.data_ptr(), d.mc_t.data_ptr(), d.q_t.data_ptr(), d.emap_t.data_ptr()), fp, LRF, i & 1)
                                   for i, d in enumerate(dp)])
    work = C.c_void_p()
    B.check(lib.svt_hip_entropy_work_create(ctx, W, H, W // 8, C.byref(lim), C.byref(work)))
    if a.coef:
        B.check(lib.svt_hip_entropy_work_set_coef_update(ctx, work, 1))
    header_max = B.FRAME_UNCOMPRESSED_MAX + int(lib.svt_hip_boolcode_capacity(lib.svt_hip_coef_update_bools_capacity())) if a.coef else B.FRAME_HEADER_MAX
    arena = torch.zeros(n * (header_max + max_tile), dtype=torch.uint8, device="cuda")
    table = torch.zeros(2 * (n + 1), dtype=torch.int32, device="cuda")
    results = torch.zeros(8 * n, dtype=torch.int32, device="cuda")
    marks = {}

    def on_stage(_user, stage):
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        marks[stage] = e
    hook = HOOK(on_stage)
    torch.cuda.synchronize()
    names = B.ENT_STAGES_COEF
    order = [0, 1, 2, 3, B.ENT_STAGE_COEF_UPDATE, 4, 5, 6, 7, 8] if a.coef else list(range(9))      # the hook's sequence; the last is "end"
    call_ms, hooked_ms, stage_ms = [], [], {names[k]: [] for k in order[:-1]}
    for hooked in (False, True):                          # the call alone first; then with an event at every stage boundary
        lib.svt_hip_entropy_work_set_stage_hook(work, hook if hooked else None, None)
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            B.check(lib.svt_hip_entropy_batch_device(ctx, work, n, arr, arena.data_ptr(), arena.numel(), table.data_ptr(), results.data_ptr()))
            e1.record(stream)
            e1.synchronize()
            if i < a.warmup:
                continue
            (hooked_ms if hooked else call_ms).append(e0.elapsed_time(e1))
            if hooked:
                for k, nxt in zip(order, order[1:]):
                    stage_ms[names[k]].append(marks[k].elapsed_time(marks[nxt]))
    res = results.cpu().numpy().view(B.ENTROPY_RESULT_DTYPE)
    tab = table.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert not res["flags"].any() and int(tab[n, 1]) == 0, ("a picture was withheld", res["flags"].tolist())
    # the coded bools of the two distinct pictures: the host form over the downloaded grids
    coded = []
    for i in range(min(n, 2)):
        d = dp[i]
        pic = dict(W=W, H=H, lf_mi=d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8),
                   mc_mi=d.mc_t.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8), qcoeff=d.q_t.cpu().numpy(), eob_map=d.emap_t.cpu().numpy().view(np.uint16),
                   lrf=LRF, restrict=i & 1)
        if a.coef:
            import entropy_coef_model as EC
            h = EC.host_entropy_coef(pic, fp, lim)
        else:
            h = E.host_entropy(pic, fp, lim)
        off, size = (int(v) for v in tab[i])
        assert h["rc"] == 0 and h["packet"] == bytes(arena[off:off + size].cpu().numpy()), "the device's packet differs from the host form's"
        coded.append(h["stream_bools"])
    out = dict(mode="driver_coef" if a.coef else "driver", pictures=n, packet_bytes_per_picture=tab[:2, 1].tolist(), call=stat(call_ms), call_with_stage_events=stat(hooked_ms), stages={s: stat(t) for s, t in stage_ms.items()},
               tokens_per_picture=res["tokens"][:2].tolist(), mode_bools_per_picture=res["mode_bools"][:2].tolist(), coded_bools_per_picture=coded,
               tile_bytes_per_picture=res["tile_bytes"][:2].tolist(), inter_leaves=res["inter_leaves"][:2].tolist(), newmv_leaves=res["newmv_leaves"][:2].tolist(),
               workspace_bytes=int(lib.svt_hip_entropy_work_bytes(W, H, W // 8, C.byref(lim))) + (int(lib.svt_hip_entropy_coef_update_bytes(C.byref(lim))) if a.coef else 0))
    lib.svt_hip_entropy_work_destroy(ctx, work)
    return out


def separate(lib, ctx, stream, dp, level, limits, a):
    from test_gpu_frame import frame_batch
    from test_gpu_md_inter import MdBuffers, md_device
    from test_gpu_modes import Tile
    from test_gpu_modes_inter import InterBuffers, modes_device
    n = len(dp)
    max_tokens, max_bools, max_tile = limits
    fr = IM.frame(**IM.B_PICTURE)
    head = FM.host_header_bytes(frame_params(level))
    tbs, vbs, mbs = [G.TokBuffers(W, H, capacity=max_tokens, counts=False) for _ in dp], [MdBuffers(W, H, want_cand=False) for _ in dp], [InterBuffers(W, H) for _ in dp]
    tiles = [Tile(W, H, tb, mb) for tb, mb in zip(tbs, mbs)]          # (sized from the capacities: replaced by the limits below)
    for t in tiles:
        t.max_bools, t.cap = max_bools, max_tile
        t.bytes = torch.zeros(max_tile + 64, dtype=torch.uint8, device="cuda")
        t.struct.max_bools, t.struct.capacity, t.struct.d_bytes = max_bools, max_tile, t.bytes.data_ptr()
    arena, packets = frame_batch(ctx, tiles, [head] * n)
    metas = [dict(W=W, H=H, frame=fr, restrict=i & 1, lrf=LRF) for i in range(n)]
    md = [vb.struct((d.lf_t, d.mc_t), m, ref_mask=0) for vb, d, m in zip(vbs, dp, metas)]
    streams = (B.BoolStream * n)(*[t.struct for t in tiles])
    torch.cuda.synchronize()

    def chain():
        G.tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t) for d in dp], tbs)
        md_device(ctx, W, H, md)
        modes_device(ctx, W, H, [((d.lf_t, d.mc_t, vb.ext), d.emap_t, tb.tok_off, fr) for d, vb, tb in zip(dp, vbs, tbs)], mbs)
        B.check(lib.svt_hip_boolcode_batch_device(ctx, n, streams))
        B.check(lib.svt_hip_frame_batch_device(ctx, n, packets, arena.address, arena.cap, arena.table.data_ptr()))
    call_ms = []
    for i in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        chain()
        e1.record(stream)
        e1.synchronize()
        if i >= a.warmup:
            call_ms.append(e0.elapsed_time(e1))
    tab = arena.table.cpu().numpy().view(np.uint32)[:2 * (n + 1)].reshape(-1, 2)
    assert int(tab[n, 1]) == 0, "a picture has no packet: the limits do not hold it"
    totals = [int(tb.sb_off.cpu().numpy().view(np.uint32)[-1]) for tb in tbs[:2]]
    assert max(totals) <= max_tokens
    return dict(mode="separate", pictures=n, call=stat(call_ms), tokens_per_picture=totals, packet_bytes_per_picture=tab[:2, 1].tolist())


def main():
    global Q_INDEX                  # (tools/coef_update_bytes.py sets it from outside as well)
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", default="1,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bools-per-token", type=int, default=2)
    ap.add_argument("--separate", action="store_true")
    ap.add_argument("--coef", action="store_true")
    ap.add_argument("--q", default=str(Q_INDEX))
    a = ap.parse_args()
    lib = B.load()
    stream = torch.cuda.Stream()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))
    B.check(lib.svt_hip_boolcode_set_tables(ctx, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(ctx, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    sizes = [int(v) for v in a.pics.split(",")]
    for Q_INDEX in (int(v) for v in a.q.split(",")):
        dp, work, keep, level = encoded_batch(lib, ctx, max(sizes))
        totals, max_tokens, max_bools, max_tile = sizing(lib, ctx, dp, a.bools_per_token)
        for n in sizes:
            out = (separate if a.separate else driver)(lib, ctx, stream, dp[:n], level, (max_tokens, max_bools, max_tile), a)
            out.update(width=W, height=H, q_index=Q_INDEX, reps=a.reps, limits=dict(max_tokens=max_tokens, max_bools=max_bools, max_tile_bytes=max_tile))
            print(json.dumps(out), flush=True)
        lib.svt_hip_encdec_work_destroy(ctx, work)
        del dp, keep
    lib.svt_hip_ctx_destroy(ctx)


if __name__ == "__main__":
    main()

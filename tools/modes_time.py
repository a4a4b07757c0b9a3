#!/usr/bin/env python3
"""Times the key-frame mode-info stage on one 2160p key frame (T.gen_yuv, the grid of svt_hip_md_intra_search_device and the intra encode
pass of tools/intra_search_time.py, q index 160): device events on the context's stream around svt_hip_modes_kf_batch_device alone, and
around the chain svt_hip_tokenize_batch_device -> svt_hip_modes_kf_batch_device -> svt_hip_boolcode_batch_device.  Warm-ups, then the
median of --reps calls with min / max.  Every timed result is compared byte for byte with the host chain (svt_hip_tokenize_picture ->
svt_hip_modes_kf_picture -> svt_hip_boolcode_host) before it is reported.  Prints one JSON line, with the reference's seconds for the
fixture pictures on one core from tests/golden/modes_reference.npz beside it.

    python tools/modes_time.py [--reps 25]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                      # noqa: E402
import boolcode_model as BM       # noqa: E402
import encdec_model as M          # noqa: E402
import modes_model as MM          # noqa: E402
import svt_testlib as T           # noqa: E402
import test_gpu_intra as TI       # noqa: E402
import test_gpu_modes as GM       # noqa: E402
import test_gpu_tokenize as G     # noqa: E402
import tokenize_model as TM       # noqa: E402
from test_gpu_encdec import dev, flags_of   # noqa: E402

B = T.B
W, H, Q_INDEX = 3840, 2160, 160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    lib = B.load()
    stream = torch.cuda.Stream()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))
    B.check(lib.svt_hip_boolcode_set_tables(ctx, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_set_tables(ctx, MM.tables()[1].ctypes.data_as(C.c_void_p)))

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

    # the key frame: open-loop search, searched grid, intra encode pass
    src = T.gen_yuv(W, H, 11)
    srcb = dev(np.concatenate([p.ravel() for p in src]))
    planes, base = B.YuvPlanes(), srcb.data_ptr()
    planes.y, planes.u, planes.v, planes.y_stride, planes.uv_stride, planes.width, planes.height = base, base + W * H, base + W * H + (W // 2) * (H // 2), W, W // 2, W, H
    n_sb = T.n_sb(W, H)
    ois_t = torch.zeros(n_sb * B.OIS_PER_SB * 12, dtype=torch.uint8, device="cuda")
    lf_t = torch.zeros((H // 8) * (W // 8) * 8, dtype=torch.uint8, device="cuda")
    q_t = torch.zeros(n_sb * B.SB_COEFFS, dtype=torch.int16, device="cuda")
    rec = M.RefPic(W, H)
    rec_t = dev(rec.buf)
    emap_t = torch.zeros(M.eob_map_offsets(W, H)[3], dtype=torch.int16, device="cuda")
    lfm_t, nz_t = torch.zeros(n_sb * 160, dtype=torch.uint8, device="cuda"), torch.zeros(W * H // 64, dtype=torch.uint8, device="cuda")
    ac = lib.svt_hip_vp9_ac_step(Q_INDEX)
    flags, thr = flags_of(**TI.KEY), B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    p = B.EncdecPicture()
    p.d_lf_mi, p.src, p.recon = lf_t.data_ptr(), planes, rec.desc(rec_t.data_ptr())
    p.d_qcoeff, p.d_eob_map, p.d_lfm, p.d_nz = q_t.data_ptr(), emap_t.data_ptr(), lfm_t.data_ptr(), nz_t.data_ptr()
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, 1, W, H, C.byref(work)))
    torch.cuda.synchronize()
    B.check(lib.svt_hip_intra_search_device(ctx, C.byref(planes), W, H, C.c_void_p(ois_t.data_ptr())))
    B.check(lib.svt_hip_md_intra_search_device(ctx, C.c_void_p(ois_t.data_ptr()), W, H, C.c_uint32(4 * ac), lib.svt_hip_lf_level_from_q(ac, 1), C.c_void_p(lf_t.data_ptr()), W // 8))
    B.check(lib.svt_hip_encdec_intra_device(ctx, work, C.byref(p), W, H, W // 8, Q_INDEX, C.byref(flags), C.byref(thr), M.PAD, M.PAD))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    lib.svt_hip_encdec_work_destroy(ctx, work)

    # the host chain on the downloaded picture
    lf = lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
    q, emap = q_t.cpu().numpy(), emap_t.cpu().numpy().view(np.uint16)
    tok = TM.host_tokenize_picture(lf, q, emap, W, H, counts=False)
    want = MM.host_modes(lf, emap, tok["tok_off"], W, H)
    assert want["rc"] == 0 and want["n_bools"] != B.MODES_BAD_GRID
    seg = np.ascontiguousarray(want["segments"])
    n_bools = want["n_bools"] + count_token_bools(tok["tokens"])
    cap = int(lib.svt_hip_boolcode_capacity(n_bools))
    tile, size = np.zeros(cap, np.uint8), C.c_uint32()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.svt_hip_boolcode_host(vp(BM.tables()[1]), vp(tok["tokens"]), len(tok["tokens"]), vp(want["bools"]), len(want["bools"]), vp(seg), len(seg), vp(tile), cap,
                                     C.byref(size)) == 0
    want_tile = bytes(tile[:size.value])

    # device buffers; the bool coder's scratch is sized from the measured bools plus an eighth
    tb, mb = G.TokBuffers(W, H, counts=False), GM.ModesBuffers(W, H)
    st = GM.Tile(W, H, tb, mb)
    st.struct.max_bools = n_bools + n_bools // 8
    torch.cuda.synchronize()
    tok_arr = (B.TokPicture * 1)(tb.struct(lf_t, q_t, emap_t))
    mod_arr = (B.ModesPicture * 1)(mb.struct(lf_t, emap_t, tb.tok_off))
    bc_arr = (B.BoolStream * 1)(st.struct)
    tokenize = lambda: B.check(lib.svt_hip_tokenize_batch_device(ctx, 1, tok_arr, W, H, W // 8))         # noqa: E731
    modes = lambda: B.check(lib.svt_hip_modes_kf_batch_device(ctx, 1, mod_arr, W, H, W // 8))             # noqa: E731
    boolcode = lambda: B.check(lib.svt_hip_boolcode_batch_device(ctx, 1, bc_arr))                        # noqa: E731
    tokenize()
    out = dict(reps=a.reps, q_index=Q_INDEX, width=W, height=H, leaves={str(t): int(np.sum(lf["sb_type"] == t)) // (MM.UNITS[t] ** 2) for t in (0, 3, 6, 9)},
               skipped_units=int(lf["skip"].sum()), tokens=len(tok["tokens"]), mode_info_bools=want["n_bools"], bools=n_bools, tile_bytes=len(want_tile))
    r = timed(modes)
    GM.same(mb.result(), want)
    out["mode_info_alone"] = dict(**r, bools_per_s=round(want["n_bools"] / (r["median_ms"] * 1e-3)))
    r = timed(lambda: (tokenize(), modes(), boolcode()))
    GM.same(mb.result(), want)
    got, got_size, guard = st.result()
    assert got == want_tile and got_size == len(want_tile) and np.all(guard == GM.GUARD8), "2160p key frame: device tile differs from the host chain"
    out["chain_tokenise_modes_boolcode"] = dict(**r, bools_per_s=round(n_bools / (r["median_ms"] * 1e-3)))
    g = MM.fixture()
    out["reference_one_core"] = {str(n): dict(seconds=float(s), tile_bytes=int(len(g[f"tile_bytes|{n}"]))) for n, s in zip(g["names"], g["seconds"])}
    lib.svt_hip_ctx_destroy(ctx)
    print(json.dumps(out))


def count_token_bools(records):
    """bools the token records expand to, counted on the bool coder's model"""
    tabs = BM.tables()[0]
    count = np.array([[len(BM.token_bools(t, 0, 0, s, tabs)) for t in range(12)] for s in (False, True)], np.int64)
    tok, row, _ = BM.unpack(records)
    skip = np.zeros(len(tok), np.int64)
    skip[1:] = (tok[:-1] == 0) & ((row[1:] // 6) % 6 != 0)
    return int(count[skip, tok].sum())


if __name__ == "__main__":
    main()

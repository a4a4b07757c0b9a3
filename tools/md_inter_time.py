#!/usr/bin/env python3
"""Times inter mode labelling on a batch of 2160p grids, in the style of tools/tokenize_time.py: device events on the context's stream
around one svt_hip_md_inter_modes_batch_device for the whole batch, against what the same records cost without the stage -- download of
both grids of every picture, svt_hip_md_inter_modes_picture on the host (one thread), upload of the records -- timed by the host clock
around work that ends in a synchronise.  The two are run alternately; medians with min / max of --reps repetitions after warm-ups.
Every picture's records and status words are compared with the host form, byte for byte, before a number is printed.

The grids are seeded, not encoded: per SB one leaf size (8 .. 64; 8 or 16 in the partial SB row), 5 % intra leaves, single leaves of
either list and compound leaves, and an MV field per list that is constant over 32x32 regions with a small even disturbance on a
quarter of the leaves, so that a good share of the leaves carry a neighbour's MV.  Prints one JSON line.

    python tools/md_inter_time.py [--pics 32] [--reps 9]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import modes_inter_model as IM    # noqa: E402
import svt_testlib as T           # noqa: E402

B = T.B
W, H = 3840, 2160
GUARD = 64


def seeded_grids(seed):
    """(lf_mi, mc_mi) of one picture, drawn with array operations only"""
    rng = np.random.default_rng(seed)
    rows, cols = H // 8, W // 8
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    sb_rows, sb_cols = (rows + 7) // 8, (cols + 7) // 8
    level = rng.integers(0, 4, (sb_rows, sb_cols))
    level[(np.arange(sb_rows) * 8 + 8 > rows), :] = rng.integers(0, 2, (int((np.arange(sb_rows) * 8 + 8 > rows).sum()), sb_cols))
    n = 1 << level[r // 8, c // 8]
    r0, c0 = r - r % n, c - c % n                       # every unit takes the draws of its leaf's origin
    at = lambda a: a[r0, c0]                            # noqa: E731
    intra = at(rng.random((rows, cols)) < 0.05)
    kind = at(rng.choice(3, (rows, cols), p=(0.5, 0.25, 0.25)))             # list 0, list 1, both
    region = lambda: 2 * rng.integers(-32, 33, ((rows + 3) // 4, (cols + 3) // 4))[r // 4, c // 4]       # noqa: E731
    noise = lambda on: at(np.where(on, 2 * rng.integers(-4, 5, (rows, cols)), 0))      # noqa: E731
    lf, mc = np.zeros((rows, cols), B.LF_MODE_INFO_DTYPE), np.zeros((rows, cols), B.MC_MODE_INFO_DTYPE)
    lf["sb_type"], lf["tx_size"], lf["skip"], lf["is_inter"], lf["filter_level"] = 3 * (level[r // 8, c // 8] + 1), np.minimum(level[r // 8, c // 8] + 1, 3), 1, ~intra, 12
    mc["bw8"] = mc["bh8"] = n
    mc["ref_list"][..., 0] = np.where(intra, -1, np.where(kind == 1, 1, 0))
    mc["ref_list"][..., 1] = np.where(~intra & (kind == 2), 1, -1)
    for k in range(2):
        on = rng.random((rows, cols)) < 0.25
        mc["mv_row"][..., k], mc["mv_col"][..., k] = np.where(intra, 0, at(region()) + noise(on)), np.where(intra, 0, at(region()) + noise(on))
    return lf, mc


def fill(p, fr):
    p.list_ref_frame[0], p.list_ref_frame[1] = IM.LAST, IM.ALTREF
    p.reference_mode, p.allow_hp, p.comp_fixed_ref, p.restrict_ref_mvs, p.ref_mask = fr["reference_mode"], fr["allow_hp"], fr["comp_fixed_ref"], 0, 0
    p.comp_var_ref[0], p.comp_var_ref[1] = fr["comp_var_ref"]
    for i in range(4):
        p.ref_frame_sign_bias[i] = fr["sign_bias"][i]


def host_records(lib, lf, mc, fr):
    """svt_hip_md_inter_modes_picture -> (records, status)"""
    ext, st = np.zeros(lf.shape, B.MI_INTER_EXT_DTYPE), np.zeros(4, np.uint32)
    p = B.MdInterPicture()
    p.d_lf_mi, p.d_mc_mi, p.d_ext_out, p.d_cand, p.d_status = lf.ctypes.data, mc.ctypes.data, ext.ctypes.data, None, st.ctypes.data
    fill(p, fr)
    B.check(lib.svt_hip_md_inter_modes_picture(C.byref(p), W, H, W // 8))
    return ext, tuple(int(v) for v in st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    n = a.pics
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("md_inter_time: no GPU -- this tool measures on the device and has no fallback")
    lib = B.load()
    stream = torch.cuda.Stream()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))
    fr = IM.frame(**IM.B_PICTURE)
    units = (H // 8) * (W // 8)
    grids = [seeded_grids(500 + i) for i in range(n)]
    want = [host_records(lib, lf, mc, fr) for lf, mc in grids]
    assert all(st[0] > 0 and st[0] != B.MODES_BAD_GRID for _, st in want)
    lf_t = [torch.from_numpy(lf.view(np.uint8).reshape(-1)).cuda() for lf, _ in grids]
    mc_t = [torch.from_numpy(mc.view(np.uint8).reshape(-1)).cuda() for _, mc in grids]
    ext_t = [torch.full((units * 12 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for _ in grids]
    st_t = [torch.full((8,), 0x77777777, dtype=torch.int32, device="cuda") for _ in grids]
    arr = (B.MdInterPicture * n)()
    for p, l, m, e, s in zip(arr, lf_t, mc_t, ext_t, st_t):
        p.d_lf_mi, p.d_mc_mi, p.d_ext_out, p.d_cand, p.d_status = l.data_ptr(), m.data_ptr(), e.data_ptr(), None, s.data_ptr()
        fill(p, fr)
    torch.cuda.synchronize()

    def device():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        B.check(lib.svt_hip_md_inter_modes_batch_device(ctx, n, arr, W, H, W // 8))
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    up_t = [torch.empty(units * 12, dtype=torch.uint8, device="cuda") for _ in grids]

    def round_trip():
        """what the records cost without the stage: (total ms, ms of the host walk alone)"""
        torch.cuda.synchronize()
        t0, walk = time.perf_counter(), 0.0
        with torch.cuda.stream(stream):
            for l, m, u in zip(lf_t, mc_t, up_t):
                lf = l.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
                mc = m.cpu().numpy().view(B.MC_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
                t1 = time.perf_counter()
                ext, _ = host_records(lib, lf, mc, fr)
                walk += time.perf_counter() - t1
                u.copy_(torch.from_numpy(ext.view(np.uint8).reshape(-1)))
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3, walk * 1e3

    dev_ms, trip_ms, walk_ms = [], [], []
    for i in range(a.warmup + a.reps):                   # alternately
        d = device()
        t, w = round_trip()
        if i >= a.warmup:
            dev_ms.append(d); trip_ms.append(t); walk_ms.append(w)
    for (ext, st), e, s, u in zip(want, ext_t, st_t, up_t):
        raw = e.cpu().numpy()
        assert bytes(raw[:-GUARD]) == ext.tobytes() and (raw[-GUARD:] == 0xA5).all(), "2160p grid: device records differ from the host form"
        assert tuple(int(v) for v in s.cpu().numpy().view(np.uint32)[:4]) == st and (s.cpu().numpy()[4:] == 0x77777777).all()
        assert bytes(u.cpu().numpy()) == ext.tobytes()
    stat = lambda v: dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))     # noqa: E731
    out = dict(pictures=n, width=W, height=H, reps=a.reps, warmup=a.warmup, units_per_picture=units,
               inter_leaves=int(np.sum([st[0] for _, st in want])), newmv_leaves=int(np.sum([st[1] for _, st in want])),
               unfaithful_leaves=int(np.sum([st[2] for _, st in want])), device_batch=stat(dev_ms), host_round_trip=stat(trip_ms),
               host_walk_alone=stat(walk_ms))
    lib.svt_hip_ctx_destroy(ctx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the decode pass on a batch of 2160p pictures, in the manner of tools/md_inter_time.py: device events on the context's stream around
one svt_hip_decode_batch_device for the whole batch, against one svt_hip_encdec_batch_device on the same batch (same grids, same padded
references, all stage flags on), run alternately; and the transform stage of each alone, between the events a stage hook records at the
stage's boundaries (SVT_ENCDEC_STAGE_TQ .. SVT_ENCDEC_STAGE_SKIP: svt_rc_kernel for the decode pass, svt_tq_kernel for the encode pass).
Median (min .. max) of --reps repetitions after warm-ups.  Before a number is printed every picture's reconstruction (padding included), skip
flags and masks from the decode pass are compared with the encode pass's, byte for byte.

The grids are seeded (tools/md_inter_time.py's, every leaf inter), the sources are seeded clips and the coefficient sets are what the encode
pass makes of them at --q-index.  The header reader is timed on the host beside it (one thread, per frame; it is a verification tool and
not on the product's timed path).  Prints one JSON line and, with --write, profiles/decode.md.

The key-frame row: one seeded 2160p key frame (encdec_model.gen_intra_grid, filter and padding on), svt_hip_decode_intra_device beside
svt_hip_encdec_intra_device, alternately, same statistics; the reconstruction (padding included), skip flags and masks are compared before a number is printed (no prediction planes
are passed on either side).
--key-frame-only measures that row alone and, with --write, replaces only its section of profiles/decode.md.

    python tools/decode_time.py [--pics 32] [--reps 9] [--q-index 120] [--key-frame-only] [--write]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import encdec_model as EM          # noqa: E402
import frame_model as FM           # noqa: E402
import svt_testlib as T            # noqa: E402
from md_inter_time import seeded_grids   # noqa: E402

B = T.B
W, H = 3840, 2160
HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int32)
STAGE_TQ, STAGE_SKIP = 2, 3


def chroma(y, k):
    return (y[::2, ::2] // 2 + 32 + k).astype(np.uint8), (255 - y[::2, ::2] // 2).astype(np.uint8)


KEY_HEADING = "## Key frame"


def stat(v):
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def fmt(s):
    return f"{s['median_ms']} ms ({s['min_ms']} .. {s['max_ms']})"


def key_frame(lib, torch, a):
    """one seeded key frame through svt_hip_encdec_intra_device and, from its grid, coefficients and eob map, svt_hip_decode_intra_device"""
    stream = torch.cuda.Stream()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(a.q_index), 1)
    src = T.gen_yuv(W, H, 11)
    mi = EM.gen_intra_grid(11, W, H, filter_level=level)
    src_t = dev(np.concatenate([p.ravel() for p in src]))
    nco, emap_n, rec0 = T.n_sb(W, H) * B.SB_COEFFS, (W // 4) * (H // 4) * 3 // 2, EM.RefPic(W, H)

    def side(with_src):
        t = dict(lf=dev(mi.view(np.uint8).reshape(-1)), q=torch.zeros(nco, dtype=torch.int16, device="cuda"), dq=torch.zeros(nco, dtype=torch.int16, device="cuda"),
                 emap=torch.zeros(emap_n, dtype=torch.int16, device="cuda"), rec=torch.zeros(rec0.nbytes, dtype=torch.uint8, device="cuda"),
                 lfm=torch.zeros(T.n_sb(W, H) * 160, dtype=torch.uint8, device="cuda"), nz=torch.zeros(mi.size, dtype=torch.uint8, device="cuda"))
        p = B.EncdecPicture()
        p.d_lf_mi, p.recon = t["lf"].data_ptr(), rec0.desc(t["rec"].data_ptr())
        p.d_qcoeff, p.d_eob_map, p.d_lfm, p.d_nz = t["q"].data_ptr(), t["emap"].data_ptr(), t["lfm"].data_ptr(), t["nz"].data_ptr()
        if with_src:
            base = src_t.data_ptr()
            p.src.y, p.src.u, p.src.v = base, base + W * H, base + W * H + (W // 2) * (H // 2)
            p.src.y_stride, p.src.uv_stride, p.src.width, p.src.height = W, W // 2, W, H
            p.d_dqcoeff = t["dq"].data_ptr()
        return t, p
    (enc, ep), (dec, dp) = side(True), side(False)
    flags = B.EncdecFlags()
    flags.do_recon = flags.apply_loop_filter = flags.pad_reference = 1
    thr = B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, 1, W, H, C.byref(work)))
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        B.check(call())
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)
    encode = lambda: lib.svt_hip_encdec_intra_device(ctx, work, C.byref(ep), W, H, W // 8, a.q_index, C.byref(flags), C.byref(thr), EM.PAD, EM.PAD)      # noqa: E731
    decode = lambda: lib.svt_hip_decode_intra_device(ctx, work, C.byref(dp), W, H, W // 8, a.q_index, C.byref(thr), EM.PAD, EM.PAD, C.c_void_p(status.data_ptr()))   # noqa: E731
    timed(encode)                                         # the grid with its skip flags, the coefficients and the eob map: what the encode pass leaves
    for k in ("lf", "q", "emap"):
        dec[k].copy_(enc[k])
    torch.cuda.synchronize()
    res = dict(enc=[], dec=[])
    for i in range(a.warmup + a.reps):                    # alternately
        e, d = timed(encode), timed(decode)
        if i >= a.warmup:
            res["enc"].append(e); res["dec"].append(d)
    assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    assert int(status.cpu()[0]) == 0, "the seeded key frame overflows 16 bits"
    assert torch.equal(enc["rec"], dec["rec"]), "key frame: the decode pass's reconstruction differs from the encode pass's"
    assert torch.equal(enc["lf"], dec["lf"]) and torch.equal(enc["lfm"], dec["lfm"]), "key frame: skip flags or masks differ"
    lib.svt_hip_encdec_work_destroy(ctx, work)
    lib.svt_hip_ctx_destroy(ctx)
    return dict(width=W, height=H, q_index=a.q_index, reps=a.reps, warmup=a.warmup, encode_intra_pass=stat(res["enc"]), decode_intra_pass=stat(res["dec"]))


def key_frame_section(k):
    return (f"{KEY_HEADING}\n\nOne seeded {k['width']}x{k['height']} key frame (`gen_intra_grid`: blocks of 8x8, 16x16 and 32x32, random modes), q index {k['q_index']}, deblocking and "
            f"padding on, the pass alone on the device; median (min .. max) of {k['reps']} alternating repetitions after {k['warmup']} warm-ups, device time between stream "
            "events.  The decode pass's reconstruction (padding included), skip flags and masks equalled the encode pass's; no prediction planes were passed on either side.\n\n| | time |\n|---|---|\n"
            f"| `svt_hip_encdec_intra_device` | {fmt(k['encode_intra_pass'])} |\n| `svt_hip_decode_intra_device` | {fmt(k['decode_intra_pass'])} |\n\n"
            "Both walk the same chain of dependent blocks and do unequal work on each (the decode pass has no forward transform or quantiser and reads the "
            "coefficients the encode pass writes): the table records both, it claims no gain.  The pass beside other kernels was not measured.\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--q-index", type=int, default=120)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--key-frame-only", action="store_true")
    a = ap.parse_args()
    n = a.pics
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("decode_time: no GPU -- this tool measures on the device and has no fallback")
    lib = B.load()
    path = os.path.join(ROOT, "profiles", "decode.md")
    if a.key_frame_only:
        k = key_frame(lib, torch, a)
        print(json.dumps(dict(key_frame=k)))
        if a.write:
            text = open(path).read() if os.path.exists(path) else ""
            with open(path, "w") as fh:
                fh.write(text.split(KEY_HEADING)[0].rstrip("\n") + "\n\n" + key_frame_section(k))
        return
    stream = torch.cuda.Stream()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    frames = T.gen_clip_subpel(W, H, 3, 11)
    refs = [EM.RefPic(W, H).set_padded(frames[k], *chroma(frames[k], k)) for k in (0, 2)]
    refs_dev = [dev(r.buf) for r in refs]
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(a.q_index), 0)
    pic, nco, units = W * H * 3 // 2, T.n_sb(W, H) * B.SB_COEFFS, (H // 8) * (W // 8)
    src_t = dev(np.concatenate([frames[1].ravel()] + [c.ravel() for c in chroma(frames[1], 1)]))     # one source serves every picture
    emap_n = (W // 4) * (H // 4) * 3 // 2
    rec0 = EM.RefPic(W, H)

    class Side:
        """the buffers of one pass over the batch"""

        def __init__(self, grids):
            self.pred = torch.zeros(n * pic, dtype=torch.uint8, device="cuda")
            self.q = torch.zeros(n * nco, dtype=torch.int16, device="cuda")
            self.lf = [dev(lf.view(np.uint8).reshape(-1)) for lf, _ in grids]
            self.mc = [dev(mc.view(np.uint8).reshape(-1)) for _, mc in grids]
            self.emap = [torch.zeros(emap_n, dtype=torch.int16, device="cuda") for _ in grids]
            self.rec = [torch.zeros(rec0.nbytes, dtype=torch.uint8, device="cuda") for _ in grids]
            self.lfm = [torch.zeros(T.n_sb(W, H) * 160, dtype=torch.uint8, device="cuda") for _ in grids]
            self.nz = [torch.zeros(units, dtype=torch.uint8, device="cuda") for _ in grids]
            self.arr = (B.EncdecPicture * n)()
            for i, p in enumerate(self.arr):
                p.d_mc_mi, p.d_lf_mi = self.mc[i].data_ptr(), self.lf[i].data_ptr()
                for planes, base in ((p.src, src_t.data_ptr()), (p.pred, self.pred.data_ptr() + i * pic)):
                    planes.y, planes.u, planes.v = base, base + W * H, base + W * H + (W // 2) * (H // 2)
                    planes.y_stride, planes.uv_stride, planes.width, planes.height = W, W // 2, W, H
                p.recon = rec0.desc(self.rec[i].data_ptr())
                for l in range(2):
                    p.ref[l] = refs[l].desc(refs_dev[l].data_ptr())
                p.d_qcoeff, p.d_dqcoeff, p.d_eob_map = self.q.data_ptr() + 2 * i * nco, None, self.emap[i].data_ptr()
                p.d_lfm, p.d_nz, p.use_subpel = self.lfm[i].data_ptr(), self.nz[i].data_ptr(), 1

    grids = []
    for i in range(n):
        lf, mc = seeded_grids(900 + i)
        inter = lf["is_inter"] != 0                       # every leaf inter: the decode pass takes no intra blocks
        lf["is_inter"], lf["skip"], lf["filter_level"] = 1, 0, level
        mc["ref_list"][..., 0] = np.where(inter, mc["ref_list"][..., 0], 0)
        grids.append((lf, mc))
    enc, dec = Side(grids), Side(grids)
    flags = B.EncdecFlags()
    flags.do_recon = flags.apply_loop_filter = flags.pad_reference = 1
    thr = B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    work = C.c_void_p()
    B.check(lib.svt_hip_encdec_work_create(ctx, n, W, H, C.byref(work)))
    marks = {}

    def on_stage(_user, stage):
        if stage in (STAGE_TQ, STAGE_SKIP):
            e = torch.cuda.Event(enable_timing=True)
            e.record(stream)
            marks[stage] = e
    hook = HOOK(on_stage)
    lib.svt_hip_encdec_work_set_stage_hook(work, hook, None)
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        B.check(call())
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), marks[STAGE_TQ].elapsed_time(marks[STAGE_SKIP])

    encode = lambda: lib.svt_hip_encdec_batch_device(ctx, work, n, enc.arr, W, H, W // 8, a.q_index, C.byref(flags), C.byref(thr), EM.PAD, EM.PAD)      # noqa: E731
    decode = lambda: lib.svt_hip_decode_batch_device(ctx, work, n, dec.arr, W, H, W // 8, a.q_index, C.byref(thr), EM.PAD, EM.PAD, C.c_void_p(status.data_ptr()))   # noqa: E731
    timed(encode)                                         # the coefficient sets: what the encode pass makes of the seeded batch
    dec.q.copy_(enc.q)
    for d, e in zip(dec.emap, enc.emap):
        d.copy_(e)
    torch.cuda.synchronize()
    res = dict(enc=[], enc_tq=[], dec=[], dec_rc=[])
    for i in range(a.warmup + a.reps):                    # alternately
        e_all, e_tq = timed(encode)
        d_all, d_rc = timed(decode)
        if i >= a.warmup:
            res["enc"].append(e_all); res["enc_tq"].append(e_tq); res["dec"].append(d_all); res["dec_rc"].append(d_rc)
    assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    assert int(status.cpu()[0]) == 0, "the seeded batch overflows 16 bits"
    for i in range(n):
        assert torch.equal(enc.rec[i], dec.rec[i]), f"picture {i}: the decode pass's reconstruction differs from the encode pass's"
        assert torch.equal(enc.lf[i], dec.lf[i]) and torch.equal(enc.lfm[i], dec.lfm[i]), f"picture {i}: skip flags or masks differ"
    assert torch.equal(enc.pred, dec.pred)
    lib.svt_hip_encdec_work_destroy(ctx, work)
    lib.svt_hip_ctx_destroy(ctx)
    # the header reader, host, one thread
    head = np.frombuffer(FM.host_header_bytes(FM.inter(width=W, height=H, frame_parallel_decoding_mode=1, base_qindex=a.q_index)), np.uint8).copy()
    info, lr, lm = B.FrameReadInfo(), (C.c_int8 * 4)(1, 0, -1, -1), (C.c_int8 * 2)(0, 0)
    t0, calls = time.perf_counter(), 20000
    for _ in range(calls):
        lib.svt_hip_frame_read_header_host(head.ctypes.data_as(C.c_void_p), len(head), lr, lm, C.byref(info))
    header_us = (time.perf_counter() - t0) / calls * 1e6
    out = dict(pictures=n, width=W, height=H, q_index=a.q_index, reps=a.reps, warmup=a.warmup, encode_pass=stat(res["enc"]), decode_pass=stat(res["dec"]),
               encode_transform_stage=stat(res["enc_tq"]), decode_recon_stage=stat(res["dec_rc"]), header_reader_us_per_frame_incl_ctypes=round(header_us, 2))
    out["key_frame"] = key_frame(lib, torch, a)
    print(json.dumps(out))
    if a.write:
        f = fmt
        with open(path, "w") as fh:
            fh.write(f"# Decode pass against encode pass (tools/decode_time.py)\n\nOne MI355X; {n} seeded pictures of {W}x{H} in one call, q index {a.q_index}, every stage flag on; "
                     f"median (min .. max) of {a.reps} alternating repetitions after {a.warmup} warm-ups, device time between stream events.  The decode pass's planes, padding, "
                     "skip flags and masks equalled the encode pass's for every picture.\n\n| | time |\n|---|---|\n"
                     f"| `svt_hip_encdec_batch_device` | {f(out['encode_pass'])} |\n| `svt_hip_decode_batch_device` | {f(out['decode_pass'])} |\n"
                     f"| transform stage of the encode pass (`svt_tq_kernel`, stage hook events) | {f(out['encode_transform_stage'])} |\n"
                     f"| reconstruction stage of the decode pass (`svt_rc_kernel`, stage hook events) | {f(out['decode_recon_stage'])} |\n\n"
                     f"Header reader (`svt_hip_frame_read_header_host`), host, one thread, through ctypes: {out['header_reader_us_per_frame_incl_ctypes']} us per frame.  "
                     "It is a verification tool, not on the product's timed path.  The tile reader's time per picture was not taken.  The two passes do unequal work (the decode pass has no forward transform or quantiser): the table records both, it claims no gain.\n\n"
                     + key_frame_section(out["key_frame"]))


if __name__ == "__main__":
    main()

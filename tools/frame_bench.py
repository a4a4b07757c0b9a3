#!/usr/bin/env python3
"""Times the delivery of a batch of 32 coded tiles as dense frame packets, two ways, alternating in one process:
  (a) svt_hip_frame_batch_device: one descriptor upload and one kernel, sizes read on the device;
  (b) what a caller had to do before that entry point existed: svt_hip_ctx_synchronize, a read-back of the 32 sizes
      (svt_hip_mem_download), and 32 device-to-device copies (svt_hip_mem_copy_2d_device, one row each) into the same dense layout --
      headers and trailers left out of (b), so it moves slightly less.
The tiles have sizes spread around 256 KiB and start at mixed offsets mod 16 inside slots as large as the bool coder's; the stream is
idle when either starts, which favours (b): in a chain its synchronise also drains the stages in front.  Per repetition: device time
between two events on the context's stream (for (b) that includes the device idling while the host reads the sizes) and host wall time
up to a final synchronise.  Warm-ups, then --reps repetitions; median, min, max.  Prints one JSON line and, with --markdown, the table
of profiles/frame.md.

    python tools/frame_bench.py [--reps 30] [--markdown]
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
import torch                      # noqa: E402
import svt_testlib as T           # noqa: E402

B = T.B
N, MEAN = 32, 256 * 1024
SLOT = 1 << 20                    # bytes between two tiles' slots


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 20
    if not torch.cuda.is_available():
        raise SystemExit("frame_bench: no GPU")
    lib = B.load()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(ctx), 0))
    stream = torch.cuda.ExternalStream(lib.svt_hip_ctx_stream(ctx))
    rng = np.random.default_rng(5)
    sizes = rng.integers(MEAN // 2, MEAN * 3 // 2, N).astype(np.uint32)
    mis = rng.integers(0, 16, N)
    src = torch.from_numpy(rng.integers(0, 256, N * SLOT, dtype=np.uint8)).cuda()
    size_t = torch.from_numpy(sizes.view(np.int32)).cuda()
    heads = [rng.integers(0, 256, int(rng.integers(14, 23)), dtype=np.uint8).tobytes() for _ in range(N)]
    total = int(sizes.sum()) + sum(len(h) for h in heads)
    arena = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    arena_b = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    table = torch.zeros(2 * (N + 1), dtype=torch.int32, device="cuda")
    arr = (B.FramePacket * N)()
    for i, q in enumerate(arr):
        q.d_tile, q.d_tile_size, q.tile_capacity, q.header_len = src.data_ptr() + i * SLOT + int(mis[i]), size_t.data_ptr() + 4 * i, SLOT - 16, len(heads[i])
        C.memmove(q.header, heads[i], len(heads[i]))
    torch.cuda.synchronize()
    host_sizes = np.zeros(N, np.uint32)

    def run_a():
        B.check(lib.svt_hip_frame_batch_device(ctx, N, arr, arena.data_ptr(), total, table.data_ptr()))

    def run_b():
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        B.check(lib.svt_hip_mem_download(ctx, host_sizes.ctypes.data_as(C.c_void_p), C.c_void_p(size_t.data_ptr()), C.c_size_t(4 * N)))
        at = 0
        for i in range(N):
            at += len(heads[i])
            n = C.c_size_t(int(host_sizes[i]))
            B.check(lib.svt_hip_mem_copy_2d_device(ctx, C.c_void_p(arena_b.data_ptr() + at), n, C.c_void_p(src.data_ptr() + i * SLOT + int(mis[i])), n, n, C.c_size_t(1)))
            at += n.value

    dev = dict(a=[], b=[])
    wall = dict(a=[], b=[])
    for rep in range(a.warmup + a.reps):
        for name, fn in (("a", run_a), ("b", run_b)) if rep % 2 == 0 else (("b", run_b), ("a", run_a)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            B.check(lib.svt_hip_ctx_synchronize(ctx))
            t0 = time.perf_counter()
            e0.record(stream)
            fn()
            e1.record(stream)
            B.check(lib.svt_hip_ctx_synchronize(ctx))
            t1 = time.perf_counter()
            if rep >= a.warmup:
                dev[name].append(e0.elapsed_time(e1))
                wall[name].append((t1 - t0) * 1e3)
    # both produced the same tile bytes at the same places
    got, alt, tab = arena.cpu().numpy(), arena_b.cpu().numpy(), table.cpu().numpy().view(np.uint32).reshape(-1, 2)
    at = 0
    for i in range(N):
        assert tab[i].tolist() == [at, len(heads[i]) + int(sizes[i])]
        assert bytes(got[at:at + len(heads[i])]) == heads[i]
        at += len(heads[i])
        assert np.array_equal(got[at:at + sizes[i]], alt[at:at + sizes[i]])
        at += int(sizes[i])
    assert tab[N].tolist() == [total, 0]
    out = dict(reps=a.reps, tiles=N, bytes=total, min_tile=int(sizes.min()), max_tile=int(sizes.max()),
               a_device_ms=stats(dev["a"]), b_device_ms=stats(dev["b"]), a_wall_ms=stats(wall["a"]), b_wall_ms=stats(wall["b"]))
    out["a_effective_GBps"] = round(2 * total / (out["a_device_ms"]["median"] * 1e-3) / 1e9, 1)       # read + written
    out["a_not_slower_than_b"] = bool(out["a_device_ms"]["median"] <= out["b_device_ms"]["median"])
    lib.svt_hip_ctx_destroy(ctx)
    print(json.dumps(out))
    if a.markdown:
        print("| | device ms between stream events, median (min .. max) | host wall ms, median (min .. max) |\n|---|---|---|")
        for k, label in (("a", "(a) svt_hip_frame_batch_device"), ("b", "(b) synchronise, read 32 sizes, 32 device-to-device copies")):
            d, w = out[f"{k}_device_ms"], out[f"{k}_wall_ms"]
            print(f"| {label} | {d['median']} ({d['min']} .. {d['max']}) | {w['median']} ({w['min']} .. {w['max']}) |")


if __name__ == "__main__":
    main()

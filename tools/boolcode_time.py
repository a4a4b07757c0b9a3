#!/usr/bin/env python3
"""Times svt_hip_boolcode_batch_device (device events around the whole call, svt_hip_last_kernel_ms):
  - on a synthetic stream of 2M raw bools (bits drawn to match their probabilities);
  - on one 2160p picture as the encode pass and the tokeniser leave it (the clip and grids of tools/tokenize_time.py, the bench's q
    index 160), coded straight from the tokeniser's buffer with the record count read on the device;
  - on the three fixture token streams tiled to that picture's record count, in one batch.
Prints one JSON line: milliseconds per stream, bools/s, the measured bools of the 2160p picture, and the reference's bools/s on one core
from tests/golden/boolcode_reference.npz.  Warm-ups, then the median of --reps calls with min / max.  The per-kernel split comes from the
same run under a kernel trace:

    python tools/boolcode_time.py [--reps 25]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/boolcode_time.py --reps 5
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
import torch                      # noqa: E402
import boolcode_model as BM       # noqa: E402
import me_configs as MC           # noqa: E402
import encdec_model as M          # noqa: E402
import svt_testlib as T           # noqa: E402
import test_gpu_boolcode as GB    # noqa: E402
import test_gpu_tokenize as G     # noqa: E402
import tokenize_time as TT        # noqa: E402

B = T.B
W, H, Q_INDEX = TT.W, TT.H, TT.Q_INDEX
# bools of a token record: [node 0 left out][token], counted on the model's expansion
COUNT = np.array([[len(BM.token_bools(t, 0, 0, s, BM.tables()[0])) for t in range(12)] for s in (False, True)], np.int64)


def count_bools(records):
    tok, row, _ = BM.unpack(records)
    skip = np.zeros(len(tok), np.int64)
    skip[1:] = (tok[:-1] == 0) & ((row[1:] // 6) % 6 != 0)
    return int(COUNT[skip, tok].sum())


def picture_tokens(ctx):
    """device token buffer of one coded 2160p picture: (TokBuffers, records)"""
    lib = B.load()
    frames = TT.clip(1)
    refs = [M.RefPic(W, H).set_padded(frames[k], *G._chroma(frames[k], k)) for k in (0, 2)]
    pa = [T.PaPic(f) for f in frames]
    level = lib.svt_hip_lf_level_from_q(lib.svt_hip_vp9_ac_step(Q_INDEX), 0)
    res = np.zeros((T.n_sb(W, H), 85), dtype=B.ME_RESULT_DTYPE)
    dc, d0, d1 = pa[1].desc(), pa[0].desc(), pa[2].desc()
    B.check(lib.svt_hip_me_picture(ctx, C.byref(dc), C.byref(d0), C.byref(d1), C.byref(MC.preset("c3_2160p_m8", 2, 1)), res.ctypes.data_as(C.c_void_p), None))
    dp, work, keep = G.encode_batch(ctx, W, H, [(frames[1],) + G._chroma(frames[1], 1)], refs, [G.md_host(res, W, H, 300, level)], Q_INDEX)
    bufs = G.tokenize_device(ctx, W, H, [(dp[0].lf_t, dp[0].q_t, dp[0].emap_t)])
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert lib.svt_hip_encdec_work_status(ctx, work, None) == 0
    lib.svt_hip_encdec_work_destroy(ctx, work)
    return bufs[0], int(bufs[0].sb_off.cpu().numpy().view(np.uint32)[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bools", type=int, default=2_000_000)
    a = ap.parse_args()
    lib = B.load()
    ctx = GB.new_ctx()

    def timed(streams):
        arr = (B.BoolStream * len(streams))(*[s.struct for s in streams])
        t = []
        for i in range(a.warmup + a.reps):
            B.check(lib.svt_hip_boolcode_batch_device(ctx, len(streams), arr))
            B.check(lib.svt_hip_ctx_synchronize(ctx))
            if i >= a.warmup:
                t.append(float(lib.svt_hip_last_kernel_ms(ctx)))
        return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))

    out = dict(reps=a.reps, q_index=Q_INDEX)
    # 1. synthetic raw bools
    rng = np.random.default_rng(11)
    p = rng.integers(1, 256, a.bools)
    bools = (((rng.random(a.bools) >= p / 256.0).astype(np.uint16) << 8) | p.astype(np.uint16)).astype(np.uint16)
    s = GB.Stream(bools=bools, segments=[(0, len(bools), 1)])
    r = timed([s])
    got, size, _ = s.result()
    want = BM.host_code(bools=bools, segments=[(0, len(bools), 1)])[0]
    assert got == want, "synthetic stream: device bytes differ from the host form"
    out["synthetic"] = dict(bools=a.bools, bytes=size, **r, bools_per_s=round(a.bools / (r["median_ms"] * 1e-3)))
    # 2. a coded 2160p picture, from the tokeniser's buffer
    buf, n_rec = picture_tokens(ctx)
    rec = buf.tokens.cpu().numpy().view(np.uint32)[:n_rec]
    n_bools = count_bools(rec)
    s = GB.Stream(tokens=rec[:1], d_tokens=buf.tokens, max_bools=n_bools + n_bools // 8)
    s.struct.d_n_tokens, s.struct.n_tokens = buf.sb_off.data_ptr() + 4 * T.n_sb(W, H), 0
    r = timed([s])
    got, size, _ = s.result()
    assert got == BM.host_code(tokens=rec)[0], "2160p picture: device bytes differ from the host form"
    out["picture_2160p"] = dict(records=n_rec, bools=n_bools, bytes=size, **r, bools_per_s=round(n_bools / (r["median_ms"] * 1e-3)))
    # 3. the fixture streams tiled to that record count, one batch
    tiled = [np.tile(t, n_rec // len(t) + 1)[:n_rec] for t in BM.fixture_token_streams()]
    counts = [count_bools(t) for t in tiled]
    streams = [GB.Stream(tokens=t, max_bools=c + c // 8) for t, c in zip(tiled, counts)]
    r = timed(streams)
    for t, st in zip(tiled, streams):
        assert st.result()[0] == BM.host_code(tokens=t)[0], "tiled fixture stream: device bytes differ from the host form"
    out["fixture_tiled"] = dict(streams=len(streams), records=n_rec, bools=counts, **r, ms_per_stream=round(r["median_ms"] / len(streams), 4),
                                bools_per_s=round(sum(counts) / (r["median_ms"] * 1e-3)))
    g = BM.fixture()
    out["reference_one_core_bools_per_s"] = [round(float(b / s)) for b, s in zip(g["token_bools"], g["token_seconds"])]
    lib.svt_hip_ctx_destroy(ctx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

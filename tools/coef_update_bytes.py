#!/usr/bin/env python3
"""What forward coefficient-probability updates save, and what they cost, on 2160p pictures as the encode pass leaves them (the clip and
md_default grids of tools/entropy_time.py): frame bytes with and without updates at several q indices, the time of the stage alone, and
the bool coder through svt_hip_boolcode_batch_tables_device against svt_hip_boolcode_batch_device on the same inputs.

    python tools/coef_update_bytes.py [--q 100,160,220] [--time-pics 16] [--reps 20] [--warmup 3]

Bytes.  Per q index the two distinct inter pictures of the clip go through tokeniser -> labelling -> inter mode info on the device; then
(a) the bool coder under the default table, the plain headers (svt_hip_frame_header_host): the baseline, the same chain on the same
inputs; (b) the stage, the bool coder under each picture's d_probs for the tile and under no table for the header's records.  A frame =
uncompressed header + compressed header + tile.  The stage's own estimate (its summed savings, 1/512 bit) is printed beside the bytes
it was an estimate of.
Time.  --time-pics pictures at the middle q index: device events on the context's stream (a torch stream), warm-ups, then the median of
--reps calls with min / max: the stage alone; the bool coder through the old entry and through the new one with a NULL table array and
with every picture's own table, the three interleaved call by call.  One JSON line per q index and one for the times.
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
import torch                        # noqa: E402
import boolcode_model as BM         # noqa: E402
import coef_update_model as CM      # noqa: E402
import entropy_time as ET           # noqa: E402
import frame_model as FM            # noqa: E402
import modes_inter_model as IM      # noqa: E402
import svt_testlib as T             # noqa: E402
import test_gpu_tokenize as G       # noqa: E402
from test_gpu_coef_update import Picture                      # noqa: E402
from test_gpu_md_inter import MdBuffers, md_device            # noqa: E402
from test_gpu_modes import Tile                               # noqa: E402
from test_gpu_modes_inter import InterBuffers, modes_device   # noqa: E402

B = T.B
W, H = ET.W, ET.H


class Chain:
    """the device buffers of n pictures from the tokeniser to the two coded streams"""

    def __init__(self, lib, ctx, dp, level, q_index):
        self.lib, self.ctx, self.dp, n = lib, ctx, dp, len(dp)
        self.fr = IM.frame(**IM.B_PICTURE)
        self.fp = dict(ET.frame_params(level), base_qindex=q_index, refresh_frame_context=0)
        self.tbs, self.vbs, self.mbs = [G.TokBuffers(W, H) for _ in dp], [MdBuffers(W, H, want_cand=False) for _ in dp], [InterBuffers(W, H) for _ in dp]
        torch.cuda.synchronize()
        G.tokenize_device(ctx, W, H, [(d.lf_t, d.q_t, d.emap_t) for d in dp], self.tbs)
        md_device(ctx, W, H, [vb.struct((d.lf_t, d.mc_t), dict(W=W, H=H, frame=self.fr, restrict=i & 1, lrf=ET.LRF), ref_mask=0) for i, (vb, d) in enumerate(zip(self.vbs, dp))])
        modes_device(ctx, W, H, [((d.lf_t, d.mc_t, vb.ext), d.emap_t, tb.tok_off, self.fr) for d, vb, tb in zip(dp, self.vbs, self.tbs)], self.mbs)
        B.check(lib.svt_hip_ctx_synchronize(ctx))
        self.totals = [int(tb.sb_off.cpu().numpy().view(np.uint32)[-1]) for tb in self.tbs]
        self.tiles = [Tile(W, H, tb, mb) for tb, mb in zip(self.tbs, self.mbs)]
        max_bools = max(self.totals) * 5 // 4 * 2 + self.mbs[0].cap          # tools/entropy_time.py's limits: the worst case would take gigabytes of scratch
        max_tile = int(lib.svt_hip_boolcode_capacity(max_bools)) // 4
        for t in self.tiles:
            t.max_bools, t.cap = max_bools, max_tile
            t.bytes = torch.zeros(max_tile + 64, dtype=torch.uint8, device="cuda")
            t.struct.max_bools, t.struct.capacity, t.struct.d_bytes = max_bools, max_tile, t.bytes.data_ptr()
        pre, suf = CM.header_parts(self.fp)
        self.pics = []
        for tb, total in zip(self.tbs, self.totals):
            p = Picture(np.zeros(0, np.uint32), counts=np.zeros(B.TOK_COUNTS, np.uint32), prefix=pre, suffix=suf)
            p.struct.d_tokens, p.struct.d_counts, p.struct.max_tokens = tb.tokens.data_ptr(), tb.counts.data_ptr(), tb.cap
            p.struct.d_n_tokens = tb.sb_off.data_ptr() + 4 * (len(tb.sb_off) - 1)
            self.pics.append(p)
        cap = int(lib.svt_hip_boolcode_capacity(self.pics[0].cap))
        self.hdr_bytes = [torch.zeros(cap + 64, dtype=torch.uint8, device="cuda") for _ in dp]
        self.hdr_size = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in dp]
        self.hdrs = []
        for p, hb, hs in zip(self.pics, self.hdr_bytes, self.hdr_size):
            s = B.BoolStream()
            s.d_bools, s.d_segments, s.n_segments, s.max_bools, s.capacity = p.keep["bools"].data_ptr(), p.keep["seg"].data_ptr(), 1, p.cap, cap
            s.d_bytes, s.d_size = hb.data_ptr(), hs.data_ptr()
            self.hdrs.append(s)
        self.tile_arr = (B.BoolStream * n)(*[t.struct for t in self.tiles])
        self.both_arr = (B.BoolStream * (2 * n))(*([t.struct for t in self.tiles] + self.hdrs)) if 2 * n <= B.BOOL_MAX_STREAMS else None
        self.hdr_arr = (B.BoolStream * n)(*self.hdrs)
        self.cu_arr = (B.CuPicture * n)(*[p.struct for p in self.pics])
        self.own = (C.c_void_p * n)(*[p.keep["probs"].data_ptr() for p in self.pics])
        torch.cuda.synchronize()

    def stage(self):
        B.check(self.lib.svt_hip_coef_update_batch_device(self.ctx, len(self.dp), self.cu_arr))

    def code_old(self):
        B.check(self.lib.svt_hip_boolcode_batch_device(self.ctx, len(self.dp), self.tile_arr))

    def code_new(self, own):
        B.check(self.lib.svt_hip_boolcode_batch_tables_device(self.ctx, len(self.dp), self.tile_arr, self.own if own else None))

    def tile_sizes(self):
        B.check(self.lib.svt_hip_ctx_synchronize(self.ctx))
        sizes = [int(t.size.cpu().numpy().view(np.uint32)[0]) for t in self.tiles]
        assert B.BOOL_SIZE_OVERFLOW not in sizes, "a stream has more bools than the limits hold"
        return sizes


def bytes_at(lib, ctx, q_index):
    ET.Q_INDEX = q_index
    dp, work, keep, level = ET.encoded_batch(lib, ctx, 2)
    ch = Chain(lib, ctx, dp, level, q_index)
    ch.code_old()
    base_tiles = ch.tile_sizes()
    ch.stage()
    ch.code_new(True)
    B.check(lib.svt_hip_boolcode_batch_device(ctx, 2, ch.hdr_arr))
    tiles = ch.tile_sizes()
    plain = FM.host_header_bytes(ch.fp)
    out = dict(q_index=q_index, width=W, height=H, pictures=[])
    for i, p in enumerate(ch.pics):
        got = p.result()
        rc, hdr, ub, cb, _ = CM.header_coef(ch.fp, got["bools"])
        assert rc == 0 and cb == int(ch.hdr_size[i].cpu().numpy().view(np.uint32)[0]) and hdr[ub:] == bytes(ch.hdr_bytes[i][:cb].cpu().numpy())
        res = got["result"]
        est = sum(int(s) for s, t in zip(res["savings"], res["sent"]) if t) / 512 / 8
        out["pictures"].append(dict(type="inter", tokens=ch.totals[i], frame_bytes_default=len(plain) + base_tiles[i], frame_bytes_updated=len(hdr) + tiles[i],
                                    header_bytes_default=len(plain), header_bytes_updated=len(hdr), tile_bytes_default=base_tiles[i], tile_bytes_updated=tiles[i],
                                    updated_entries=[int(v) for v in res["updated"]], sent=[int(v) for v in res["sent"]], header_bools=int(res["hdr_bools"]),
                                    estimated_saving_bytes=round(est), saved_percent=round(100 * (1 - (len(hdr) + tiles[i]) / (len(plain) + base_tiles[i])), 2)))
    lib.svt_hip_encdec_work_destroy(ctx, work)
    return out


def times_at(lib, ctx, stream, q_index, n, a):
    ET.Q_INDEX = q_index
    dp, work, keep, level = ET.encoded_batch(lib, ctx, n)
    ch = Chain(lib, ctx, dp, level, q_index)
    ch.stage()
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    legs = dict(stage=ch.stage, boolcode_old_entry=ch.code_old, boolcode_new_entry_null_tables=lambda: ch.code_new(False), boolcode_new_entry_own_tables=lambda: ch.code_new(True))
    ms = {k: [] for k in legs}
    for i in range(a.warmup + a.reps):
        for k, f in legs.items():                              # interleaved: every leg once per round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            f()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    out = dict(times=True, q_index=q_index, pictures=n, reps=a.reps, tokens_per_picture=ch.totals[:2], **{k: ET.stat(v) for k, v in ms.items()})
    lib.svt_hip_encdec_work_destroy(ctx, work)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", default="100,160,220")
    ap.add_argument("--time-pics", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    lib = B.load()
    stream = torch.cuda.Stream()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create_on_stream(C.byref(ctx), 0, C.c_void_p(stream.cuda_stream)))
    B.check(lib.svt_hip_boolcode_set_tables(ctx, BM.tables()[1].ctypes.data_as(C.c_void_p)))
    B.check(lib.svt_hip_modes_inter_set_tables(ctx, IM.tables()[1].ctypes.data_as(C.c_void_p)))
    qs = [int(v) for v in a.q.split(",")]
    for q in qs:
        print(json.dumps(bytes_at(lib, ctx, q)), flush=True)
    if a.time_pics:
        print(json.dumps(times_at(lib, ctx, stream, qs[len(qs) // 2], a.time_pics, a)), flush=True)
    lib.svt_hip_ctx_destroy(ctx)


if __name__ == "__main__":
    main()

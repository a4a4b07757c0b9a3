"""GPU parity of the software-pipelined walks of the transform kernels (csrc/tq_kernel.hip): while a workgroup computes one group of
blocks, the rows of its next group and the position codes of the one after are already in flight.  What can go wrong in such a walk is
an off-by-one at either end, a register set of one iteration used by another, and a partly filled last group -- so the cases here are
about walk LENGTHS: a child process runs with SVT_HIP_TQ_GRID=8,8,8,8 (one workgroup per XCD), where 1, 8, 9, 24, 25 and 31 groups of
blocks make walks of 0, 1, 2, 3 and 4 iterations side by side in one launch, every count once with its last group full and once with
the fewest blocks the list form allows in it.  Both list forms: descriptors (svt_hip_tq_batch) and position codes (the picture-level
driver, svt_hip_encdec_batch_device).  Everything is compared byte for byte with the oracle; nothing looks at generated code.

The child computes every case once and hands back one verdict per case; the tests below only read them."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import svt_testlib as T

B = T.B
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GROUP = (256, 32, 16, 8)             # blocks per workgroup and iteration: 4x4 (one per lane), 8x8, 16x16, 32x32 (N lanes per block)
GROUPS = (1, 8, 9, 24, 25, 31)       # at 8 workgroups: walks of 1 | 1 | 2,1.. | 3 | 4,3.. | 4,..,3 iterations, some workgroups with none
NAMES = ("recon", "qcoeff", "dqcoeff", "eob")


# ---------------------------------------------------------------------------------------------------
# descriptor lists: svt_hip_tq_batch
# ---------------------------------------------------------------------------------------------------
def direct_specs():
    """(id, counts[4]): for every size every group count, last group full / one block; the other sizes empty in half of the cases (an
    empty size launches nothing), otherwise with group counts of their own"""
    out = []
    for s in range(4):
        for gi, g in enumerate(GROUPS):
            for full in (True, False):
                cnt = [0, 0, 0, 0]
                cnt[s] = g * GROUP[s] if full else (g - 1) * GROUP[s] + 1
                if (gi + full) % 2:
                    for o in range(4):
                        if o != s:
                            go = GROUPS[(gi + o + 1) % len(GROUPS)]
                            cnt[o] = (go - 1) * GROUP[o] + 1 + (o * 5) % GROUP[o]
                out.append(("n%d_g%d_%s_%s" % (4 << s, g, "full" if full else "one", "alone" if (gi + full) % 2 == 0 else "mixed"), cnt))
    return out


def subset_case(base, counts, do_recon=True):
    """the first counts[s] blocks of every size of `base` (make_tq_case: every block has its own position, content, transform type and
    quantiser), coefficients repacked"""
    blocks = np.concatenate([base["blocks"][base["blocks"]["tx_size"] == s][:counts[s]] for s in range(4)])
    assert [int((blocks["tx_size"] == s).sum()) for s in range(4)] == list(counts), "base case too small"
    nn = 16 << (2 * blocks["tx_size"].astype(np.int64))
    blocks["coeff_off"] = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(np.uint32)
    blocks["do_recon"] = int(do_recon)
    return dict(src=base["src"], pred=base["pred"], blocks=blocks, counts=np.array(counts, np.int32), qtabs=base["qtabs"], iscan=base["iscan"],
                n_coeff=int(nn.sum()))


def compare_direct(ctx, case, do_recon=True):
    o, g = T.oracle_tq_batch(case), T.hip_tq_batch(ctx, case)
    bad = [n for n, a, b in zip(NAMES, o, g) if not (n == "recon" and not do_recon) and not np.array_equal(a, b)]
    return dict(bad=bad, counts=[int(v) for v in case["counts"]], eob_classes=[len(set(o[3][case["blocks"]["tx_size"] == s].tolist())) for s in range(4)])


# ---------------------------------------------------------------------------------------------------
# position-code lists: the picture-level driver on crafted partitions
# ---------------------------------------------------------------------------------------------------
PW, PH = 256, 128                     # 8 superblocks of 16 cells (16x16 luma) each
# what a cell / a 32x32 area / a superblock of one kind adds to the lists, per transform size (luma + both chroma planes)
KINDS = {
    "c4":   (1, (24, 0, 0, 0)),       # cell: four 8x8 blocks, 4x4 transforms
    "c4b":  (1, (20, 1, 0, 0)),       # cell: one 8x8 block with an 8x8 transform, three with 4x4
    "c4c":  (1, (8, 4, 0, 0)),        # cell: four 8x8 blocks with 8x8 transforms (chroma 4x4)
    "c8":   (1, (0, 6, 0, 0)),        # cell: a 16x16 block, 8x8 transforms
    "c16":  (1, (0, 2, 1, 0)),        # cell: a 16x16 block, 16x16 transform (chroma 8x8)
    "q16":  (4, (0, 0, 6, 0)),        # 32x32 block, 16x16 transforms
    "q32":  (4, (0, 0, 2, 1)),        # 32x32 block, 32x32 transform (chroma 16x16)
    "s32":  (16, (0, 0, 0, 6)),       # 64x64 block, 32x32 transforms
}
FILLERS = (("s32", "c8"), ("s32", "c4"), ("s32", "c8"), ("q16", "c4"))   # per target size: a big and a small kind that add no block of that size


def pos_items(s, n):
    """kinds whose blocks of size s add up to exactly n"""
    if s == 0:
        assert n % 4 == 0             # a cell's 4x4 count is a multiple of 4 (eight chroma blocks, luma in fours)
        z = (n // 4) % 2
        rem = n - 20 * z
        return ["c4"] * (rem // 24) + ["c4c"] * (rem % 24 // 8) + ["c4b"] * z
    if s == 1:
        return ["c8"] * (n // 6) + ["c16"] * (n % 6 // 2) + ["c4b"] * (n % 2)
    if s == 2:
        return ["q16"] * (n // 6) + ["c16"] * (n % 6)
    return ["s32"] * (n // 6) + ["q32"] * (n % 6)


def pos_specs():
    """(id, size, count): the group counts of the descriptor cases; a partition cannot end a 4x4 list on one block (a cell adds a
    multiple of four, pos_items), there the short last group holds eight"""
    out = []
    for s in range(4):
        for g in GROUPS:
            for full in (True, False):
                n = g * GROUP[s] if full else (g - 1) * GROUP[s] + (8 if s == 0 else 1)
                out.append(("pos_n%d_g%d_%s" % (4 << s, g, "full" if full else "short"), s, n))
    return out


def pos_grids(s, n, seed, min_pics=1):
    """mode-info grids (motion, partition) of as many PW x PH pictures as the n blocks of size s need; the rest of the pictures is
    covered with kinds that add none of that size.  Superblocks are dealt out in a seeded order, so the list of size s crosses pictures."""
    rng = np.random.default_rng(seed)
    items = sorted(pos_items(s, n), key=lambda k: -KINDS[k][0])
    cells = sum(KINDS[k][0] for k in items)
    n_pics = max(min_pics, -(-cells // 128))
    big, small = FILLERS[s]
    while cells % KINDS[big][0]:
        items.append(small); cells += 1
    while cells < n_pics * 128:
        k = big if rng.random() < 0.7 else small
        items += [k] * (KINDS[big][0] // KINDS[k][0]); cells += KINDS[big][0]
    items.sort(key=lambda k: -KINDS[k][0])        # descending sizes: every item lands aligned to its own size
    mi_rows, mi_cols = PH // 8, PW // 8
    mc = [np.zeros((mi_rows, mi_cols), dtype=B.MC_MODE_INFO_DTYPE) for _ in range(n_pics)]
    lf = [np.zeros((mi_rows, mi_cols), dtype=B.LF_MODE_INFO_DTYPE) for _ in range(n_pics)]
    sbs = [(p, r, c) for p in range(n_pics) for r in range(0, mi_rows, 8) for c in range(0, mi_cols, 8)]
    order = rng.permutation(len(sbs))

    def block(p, r, c, n8, tx):
        m = np.zeros((), dtype=B.MC_MODE_INFO_DTYPE)
        m["bw8"], m["bh8"] = n8, n8
        l0 = int(rng.integers(0, 2))
        m["ref_list"] = (l0, 1 - l0 if rng.random() < 0.3 else -1)
        m["mv_row"], m["mv_col"] = rng.integers(-90, 91, 2), rng.integers(-90, 91, 2)
        mc[p][r:r + n8, c:c + n8] = m
        cell = lf[p][r:r + n8, c:c + n8]
        cell["sb_type"], cell["tx_size"], cell["is_inter"], cell["filter_level"] = {1: 3, 2: 6, 4: 9, 8: 12}[n8], tx, 1, 20

    at = 0
    for k in items:
        p, r0, c0 = sbs[order[at // 16]]
        z = at % 16                                # z-order of the cell inside its superblock
        r, c = r0 + 2 * ((z >> 1 & 1) | (z >> 3 & 1) << 1), c0 + 2 * ((z & 1) | (z >> 2 & 1) << 1)
        if k in ("c4", "c4b", "c4c"):
            n8x8 = {"c4": 0, "c4b": 1, "c4c": 4}[k]
            for j, (dr, dc) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                block(p, r + dr, c + dc, 1, 1 if j < n8x8 else 0)
        else:
            n8, tx = {"c8": (2, 1), "c16": (2, 2), "q16": (4, 2), "q32": (4, 3), "s32": (8, 3)}[k]
            block(p, r, c, n8, tx)
        at += KINDS[k][0]
    assert at == n_pics * 128
    want = [sum(KINDS[k][1][t] for k in items) for t in range(4)]
    assert want[s] == n
    return mc, lf, want


def compare_pos(ctx, s, n, seed, min_pics=1):
    import encdec_model as M
    import test_gpu_encdec as E
    lib = B.load()
    mc, lf, want = pos_grids(s, n, seed, min_pics)
    n_pics, q_index = len(mc), 90 + 10 * (seed % 9)
    frames = T.gen_clip_subpel(PW, PH, n_pics + 2, seed)
    refs = [M.RefPic(PW, PH).set_padded(frames[k], *E._chroma(frames[k], k)) for k in (0, n_pics + 1)]
    srcs = [(frames[i],) + E._chroma(frames[i], i) for i in range(1, n_pics + 1)]
    flags = E.flags_of(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=0, loop_filter=1)
    thr = B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    rec_inits = [M.RefPic(PW, PH) for _ in range(n_pics)]
    dp, blocks, pos, eob, cnt = E.run_device(ctx, PW, PH, srcs, refs, [(a, b.copy()) for a, b in zip(mc, lf)], q_index, flags, thr, rec_inits)
    bad, classes = [], set()
    if [cnt[4 + t] for t in range(4)] != want:
        bad.append("counts %s != %s" % ([cnt[4 + t] for t in range(4)], want))
    for i in range(n_pics):
        o = M.oracle_encdec_picture(srcs[i], refs, mc[i], lf[i], q_index, flags, thr, recon_init=M.RefPic(PW, PH))
        d = dp[i]
        for name, got, ref in (("prediction", d.pred_t, np.concatenate([p.ravel() for p in o["pred"]])), ("qcoeff", d.q_t, o["qcoeff"]),
                               ("dqcoeff", d.dq_t, o["dqcoeff"]), ("eob map", d.emap_t, o["eob_map"].view(np.int16)), ("reconstruction", d.rec_t, o["rec"].buf)):
            if not np.array_equal(got.cpu().numpy(), ref):
                bad.append("picture %d: %s" % (i, name))
        classes |= set(o["eob"][o["blocks"]["tx_size"] == s].tolist())
    return dict(bad=bad, counts=[cnt[4 + t] for t in range(4)], n_pics=n_pics, eob_classes=len(classes))


# ---------------------------------------------------------------------------------------------------
# the child: every case once, under SVT_HIP_TQ_GRID=8,8,8,8
# ---------------------------------------------------------------------------------------------------
def child_main(only_oracle=False):
    import torch
    if not only_oracle:
        torch.cuda.init()             # before the library pulls in the system HIP runtime (conftest.py)
    lib = B.load()
    ctx = C.c_void_p()
    if not only_oracle:
        B.check(lib.svt_hip_ctx_create(C.byref(ctx), 0))
    res = {}
    base = T.make_tq_case(41, width=1024, height=1280)
    for name, cnt in direct_specs():
        res[name] = compare_direct(ctx, subset_case(base, cnt))
    res["no_recon"] = compare_direct(ctx, subset_case(base, [3 * 256 + 7, 9 * 32 + 3, 9 * 16 + 5, 9 * 8 + 1], do_recon=False), do_recon=False)
    res["stride_260"] = compare_direct(ctx, T.make_tq_case(7, width=260, height=1024))
    for k, (name, s, n) in enumerate(pos_specs()):
        res[name] = compare_pos(ctx, s, n, 100 + k, min_pics=3 if name == "pos_n8_g25_short" else 1)
    lib.svt_hip_ctx_destroy(ctx)
    print("TQ_PREFETCH_RESULTS " + json.dumps(res))


@pytest.fixture(scope="module")
def verdicts():
    env = dict(os.environ)
    env["SVT_HIP_TQ_GRID"] = "8,8,8,8"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=HERE, env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("TQ_PREFETCH_RESULTS ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(lines[-1][len("TQ_PREFETCH_RESULTS "):])


@pytest.mark.parametrize("name,counts", direct_specs(), ids=[n for n, _ in direct_specs()])
def test_descriptor_walks(verdicts, name, counts):
    v = verdicts[name]
    assert v["counts"] == counts and v["bad"] == [], v


def test_descriptor_cases_cover_many_eob_classes(verdicts):
    """as test_tq_vs_oracle asks of its case: the longest list of every size has blocks of many different eobs"""
    for s in range(4):
        v = [verdicts[n] for n, _ in direct_specs() if n.startswith("n%d_g31_full" % (4 << s))]
        assert len(v) == 1 and v[0]["eob_classes"][s] > 8, (s, v)


def test_descriptor_walk_without_reconstruction(verdicts):
    assert verdicts["no_recon"]["bad"] == [], verdicts["no_recon"]


def test_descriptor_walk_unaligned_stride(verdicts):
    """plane stride 260 = 4 mod 16: consecutive prefetched rows alternate between the vector and the dword path"""
    v = verdicts["stride_260"]
    assert v["bad"] == [] and min(v["counts"]) > 0, v


@pytest.mark.parametrize("name,s,n", pos_specs(), ids=[n for n, _, _ in pos_specs()])
def test_position_code_walks(verdicts, name, s, n):
    v = verdicts[name]
    assert v["counts"][s] == n and v["bad"] == [], v
    if n >= 31 * GROUP[s]:
        assert v["eob_classes"] > 8, v


def test_position_code_walk_crosses_pictures(verdicts):
    """a batch of three pictures: consecutive iterations of a walk belong to different pictures, and with them to different geometry records"""
    v = verdicts["pos_n8_g25_short"]
    assert v["n_pics"] == 3 and v["bad"] == [], v


def test_default_grid_three_iterations_per_workgroup():
    """the built-in grid (no SVT_HIP_TQ_GRID): 3840-wide planes of 4x4 and of 8x8 blocks that hold more than three groups for each of the
    at most 6 x 256 workgroups of a launch of this entry point"""
    assert not os.environ.get("SVT_HIP_TQ_GRID")
    lib = B.load()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(ctx), 0))
    try:
        W, H4, H8 = 3840, 4928, 2464
        rng = np.random.default_rng(5)
        src = T.gen_clip(W, H4 + H8, 1, 9)[0]
        pred = np.clip(np.roll(src, (1, 2), (0, 1)).astype(np.int16) + rng.integers(-12, 13, src.shape), 0, 255).astype(np.uint8)
        iscan, offs = T.iscan_array()
        qtabs = np.array([T.quant_table(a, b) for a, b in ((40, 48), (8, 9), (200, 260))], dtype=B.QUANT_DTYPE)
        parts = []
        for s, (y0, y1) in enumerate(((0, H4), (H4, H4 + H8))):          # 1 182 720 4x4 blocks, then 147 840 8x8 blocks below them
            n = 4 << s
            y, x = np.meshgrid(np.arange(y0, y1, n), np.arange(0, W, n), indexing="ij")
            b = np.zeros(y.size, dtype=B.TQ_BLOCK_DTYPE)
            off = (y * W + x).ravel().astype(np.uint32)
            tt = rng.integers(0, 4, y.size)
            b["src_off"], b["pred_off"], b["recon_off"] = off, off, off
            b["iscan_off"] = np.array([offs[(s, t)] for t in range(4)], np.uint32)[tt]
            b["src_stride"], b["pred_stride"], b["recon_stride"] = W, W, W
            b["tx_size"], b["tx_type"], b["qtab"], b["do_recon"] = s, tt, rng.integers(0, 3, y.size), 1
            parts.append(b)
        blocks = np.concatenate(parts)
        nn = 16 << (2 * blocks["tx_size"].astype(np.int64))
        blocks["coeff_off"] = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(np.uint32)
        counts = np.array([len(parts[0]), len(parts[1]), 0, 0], np.int32)
        assert counts[0] >= 3 * 256 * 6 * 256 and counts[1] >= 3 * 32 * 6 * 256
        case = dict(src=src, pred=pred, blocks=blocks, counts=counts, qtabs=qtabs, iscan=iscan, n_coeff=int(nn.sum()))
        for n, a, b in zip(NAMES, T.oracle_tq_batch(case), T.hip_tq_batch(ctx, case)):
            assert np.array_equal(a, b), (n, int(np.sum(a != b)))
    finally:
        lib.svt_hip_ctx_destroy(ctx)


if __name__ == "__main__":
    child_main(only_oracle="--oracle-only" in sys.argv)

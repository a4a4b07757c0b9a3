"""GPU: the forward half of the transform stage -- residual, forward DCT / ADST, quantiser, distortion, fused rate -- at the ends of its
arithmetic (tests/tq_edges_model.py: basis-aligned +-255 blocks up to the coefficient ceilings 8160 / 16319 / 32639, amplitude ladders, the
4x4 first-sample rule, both sides of every dead-zone boundary, tables at which clamp16 of the quantiser decides the level, partial32),
through every launch form of tq_block_body (csrc/tq_core.h) and tq_lane_block (csrc/tq_kernel.hip): descriptor lists through the plain,
distortion and fused-rate entries; source, prediction and reconstruction in three unlike buffers (own offsets, pairwise different strides up
to 65532, vector and dword rows mixed); and position codes on a 255-against-0 picture pair at the q index where the clamp decides.  Every
comparison is exact, against the oracle and against the reference's recorded outputs (tests/golden/tq_edges_reference.npz)."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_model as D
import encdec_model as M
import svt_testlib as T
import tq_edges_model as E
from test_gpu_encdec import flags_of, masks_equal, run_device

B = T.B
pytestmark = pytest.mark.gpu
GUARD = E.GUARD
OUTPUTS = ("recon", "qcoeff", "dqcoeff", "eob", "dist", "bits")


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


@pytest.fixture(scope="module")
def edge():
    """the cases, the recorded reference per case, the two full layouts with what the oracle gives for them (computed once, left unchanged)"""
    cases = E.edge_cases()
    print(E.check_conditions())
    g = dict(np.load(T.GOLDEN_DIR + "/tq_edges_reference.npz"))
    assert [c["name"] for c in cases] == list(g["names"])
    ref, pos = [], 0
    for i, c in enumerate(cases):
        nn = T.TX_N[c["tx_size"]] ** 2
        ref.append((g["coeff"][pos:pos + nn], g["qcoeff"][pos:pos + nn], g["dqcoeff"][pos:pos + nn], int(g["eob"][i])))
        pos += nn
    out = dict(cases=cases, ref=ref)
    for name, L in (("recon", E.packed_layout(cases, True)), ("norecon", E.packed_layout(cases, False)), ("unlike", E.unlike_layout(cases)),
                    ("unlike2", E.unlike_layout(cases, recon_sets=2))):
        out[name] = (L, E.oracle_batch(L), recorded(L, ref))
    return out


def recorded(L, ref):
    """(qcoeff, dqcoeff, eob, dist) of a layout from the reference's recorded outputs; the distortion pair as full_distortion_kernel32bit
    forms it from the recorded coefficients: the difference through int16, the sums in uint32"""
    q = np.concatenate([ref[i][1] for i in L["idx"]])
    dq = np.concatenate([ref[i][2] for i in L["idx"]])
    eob = np.array([ref[i][3] for i in L["idx"]], np.uint16)
    dist = np.zeros((len(L["idx"]), 2), np.uint64)
    for j, i in enumerate(L["idx"]):
        co, d = ref[i][0].astype(np.int64), ref[i][2].astype(np.int64)
        dd = (co - d).astype(np.int16).astype(np.int64)
        dist[j] = (int((dd * dd).sum()) & 0xFFFFFFFF, int((co * co).sum()) & 0xFFFFFFFF)
    return q, dq, eob, dist


def launch(ctx, L, entry, n_sets=0):
    """one call of an entry point on a layout -> dict of outputs (reconstruction buffers started as GUARD) and the inputs read back"""
    lib = B.load()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()       # noqa: E731
    src, pred, blocks, qt, isc = up(L["src"]), up(L["pred"]), up(L["blocks"]), up(L["qtabs"]), up(L["iscan"])
    rtab, rscan = T.rate_tables()
    tab, scan = up(np.ascontiguousarray(rtab).reshape(1)), up(rscan)
    recs = [torch.full((L["recon_bytes"],), GUARD, dtype=torch.uint8, device="cuda") for _ in range(max(n_sets, 1))]
    nb = len(L["blocks"])
    q, dq = torch.zeros(L["n_coeff"], dtype=torch.int16, device="cuda"), torch.zeros(L["n_coeff"], dtype=torch.int16, device="cuda")
    eob, dist = torch.zeros(nb, dtype=torch.int16, device="cuda"), torch.zeros(2 * nb, dtype=torch.int64, device="cuda")
    bits = torch.zeros(nb, dtype=torch.int32, device="cuda")
    cnt = (C.c_int32 * 4)(*[int(v) for v in L["counts"]])
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    for t in (src, pred, *recs):
        assert t.data_ptr() % 16 == 0            # (the layouts' alignment census counts from the buffers' bases)
    if entry == "plain":
        B.check(lib.svt_hip_tq_batch_device(ctx, p(src), p(pred), p(recs[0]), p(blocks), cnt, p(qt), p(isc), p(q), p(dq), p(eob)))
    elif entry == "dist":
        B.check(lib.svt_hip_tq_batch_dist_device(ctx, p(src), p(pred), p(recs[0]), p(blocks), cnt, p(qt), p(isc), p(q), p(dq), p(eob), p(dist)))
    elif entry == "rd":
        B.check(lib.svt_hip_tq_rd_batch_device(ctx, p(src), p(pred), p(recs[0]), p(blocks), cnt, p(qt), p(isc), p(q), p(dq), p(eob), p(dist), p(tab), p(scan), p(bits)))
    else:
        rset = (C.c_void_p * n_sets)(*[t.data_ptr() for t in recs])
        B.check(lib.svt_hip_tq_rd_batch_multi_device(ctx, p(src), p(pred), rset, n_sets, p(blocks), cnt, p(qt), p(isc), p(q), p(dq), p(eob), p(dist), p(tab), p(scan), p(bits)))
    B.check(lib.svt_hip_ctx_synchronize(ctx))
    assert np.array_equal(src.cpu().numpy(), L["src"]) and np.array_equal(pred.cpu().numpy(), L["pred"]), "source / prediction buffers changed"
    return dict(recon=[t.cpu().numpy() for t in recs], qcoeff=q.cpu().numpy(), dqcoeff=dq.cpu().numpy(), eob=eob.cpu().numpy().view(np.uint16),
                dist=dist.cpu().numpy().view(np.uint64).reshape(-1, 2), bits=bits.cpu().numpy())


def compare(edge, L, got, want, rec, outputs):
    """got == the oracle's `want` and the recorded reference `rec`, output by output; the failing cases are named"""
    names = [edge["cases"][i]["name"] for i in L["idx"]]
    nn = 16 << (2 * L["blocks"]["tx_size"].astype(np.int64))
    first = np.concatenate([[0], np.cumsum(nn)])
    for k in outputs:
        a = got[k]
        for tag, b in (("oracle", dict(zip(OUTPUTS, want))[k]), ("fixture", dict(zip(OUTPUTS[1:5], rec)).get(k))):
            if b is None or np.array_equal(a, b):
                continue
            if k in ("qcoeff", "dqcoeff"):
                bad = [names[j] for j in range(len(names)) if not np.array_equal(a[first[j]:first[j + 1]], b[first[j]:first[j + 1]])]
            else:
                bad = [names[j] for j in range(len(names)) if not np.array_equal(a[j], b[j])]
            raise AssertionError((k, tag, len(bad), bad[:10]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# descriptor lists: every case, one launch per entry point
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,do_recon", [("plain", True), ("plain", False), ("dist", True), ("rd", True)])
def test_every_case_through_the_descriptor_entries(ctx, edge, entry, do_recon):
    """all cases, each at its own position of one plane triple, through svt_hip_tq_batch_device (reconstructing and not),
    svt_hip_tq_batch_dist_device and svt_hip_tq_rd_batch_device: recon, qcoeff, dqcoeff, eob, dist and bits equal the oracle's; qcoeff, dqcoeff,
    eob and the distortion pair equal the recorded reference's.  The 4x4 blocks fill more than one workgroup of the lane form; the rate
    inputs vary over the blocks (add_rate_info); the reconstruction plane keeps its guard bytes outside the blocks."""
    L, want, rec = edge["recon" if do_recon else "norecon"]
    assert L["counts"][0] > 256 and len(set(L["blocks"]["pad"][:, 0].tolist())) >= 10
    assert int(want[4].max()) >= 10 ** 9 and 8000 <= int(np.abs(want[1].astype(np.int32)).max()) <= E.MAX_LEVEL
    got = launch(ctx, L, entry)
    compare(edge, L, got, want, rec, ("qcoeff", "dqcoeff", "eob") + (("dist",) if entry != "plain" else ()) + (("bits",) if entry == "rd" else ()))
    if do_recon:
        assert np.array_equal(got["recon"][0][L["own"]], want[0][L["own"]]), "reconstruction"
        assert (got["recon"][0][~L["own"]] == GUARD).all(), "bytes outside the blocks"
    else:
        assert (got["recon"][0] == GUARD).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# unlike planes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_unlike_source_prediction_and_reconstruction_buffers(ctx, edge):
    """a subset with every size and type (flat 255 and clamp cases among them) whose source, prediction and reconstruction lie in three
    separate buffers at three different offsets with three different strides per block (residues 0, 4, 8, 12 mod 16; one block per size
    near the uint16 ceiling, 65532): every pointer is at least once on the vector path while another takes dwords.  A kernel that read
    the prediction with the source's stride, or chose the store path from the source's alignment, differs here.  The reconstruction
    buffer keeps its guard bytes outside the blocks; source and prediction are unchanged (checked in launch)."""
    L, want, rec = edge["unlike"]
    census = E.alignment_census(L)
    assert all(census[ts] == {0, 1, 2} for ts in (1, 2, 3)), census
    for entry in ("plain", "dist", "rd"):
        got = launch(ctx, L, entry)
        compare(edge, L, got, want, rec, ("qcoeff", "dqcoeff", "eob") + (("dist",) if entry != "plain" else ()) + (("bits",) if entry == "rd" else ()))
        assert np.array_equal(got["recon"][0][L["own"]], want[0][L["own"]]), ("reconstruction", entry)
        assert (got["recon"][0][~L["own"]] == GUARD).all(), ("bytes outside the blocks", entry)


def test_unlike_buffers_through_the_multi_buffer_entry(ctx, edge):
    """the same subset through svt_hip_tq_rd_batch_multi_device: the blocks reconstruct in turn into two buffers, those of the second with
    another stride; each buffer holds exactly its own blocks and guard bytes elsewhere"""
    L, want, rec = edge["unlike2"]
    assert set(L["set"].tolist()) == {0, 1}
    got = launch(ctx, L, "multi", n_sets=2)
    compare(edge, L, got, want, rec, ("qcoeff", "dqcoeff", "eob", "dist", "bits"))
    mine = [np.zeros(L["recon_bytes"], bool) for _ in range(2)]
    for b, k in zip(L["blocks"], L["set"]):
        n = T.TX_N[int(b["tx_size"])]
        for r in range(n):
            o = int(b["recon_off"]) + r * int(b["recon_stride"])
            mine[k][o:o + n] = True
    assert np.array_equal(mine[0] | mine[1], L["own"]) and not (mine[0] & mine[1]).any()
    for k in range(2):
        assert np.array_equal(got["recon"][k][mine[k]], want[0][mine[k]]), ("reconstruction", k)
        assert (got["recon"][k][~mine[k]] == GUARD).all(), ("bytes outside the set's blocks", k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# position codes: a picture pair at the ceilings
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bright_source", [True, False])
def test_picture_of_255_against_references_of_0(ctx, bright_source):
    """svt_hip_encdec_batch_device on two 128x64 pictures (decode_model.inter_grids: 64x64 leaves with 32x32 transforms, 32x32 leaves with
    16x16 and 32x32 transforms, 8x8 and 4x4 below) whose source is 255 everywhere against references of 0, and the reverse, at the q index
    where clamp16 decides the level of the 16x16 and of the 32x32 DC (tq_edges_model.REAL_Q_INDEX): the position-code form of the same
    kernel instances, against encdec_model.oracle_encdec_picture."""
    lib = B.load()
    W, H, q_index = D.INTER_W, D.INTER_H, E.REAL_Q_INDEX
    a, b = (255, 0) if bright_source else (0, 255)
    srcs = [(np.full((H, W), a, np.uint8), np.full((H // 2, W // 2), a, np.uint8), np.full((H // 2, W // 2), a, np.uint8)) for _ in range(2)]
    refs = [M.RefPic(W, H, fill=b), M.RefPic(W, H, fill=b)]
    grids = [D.inter_grids(v) for v in range(2)]
    flags = flags_of(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=0, loop_filter=1)
    thr = B.LfThresh()
    lib.svt_hip_lf_thresh_init(C.byref(thr), 0)
    rng = np.random.default_rng(9)
    rec_inits = [M.RefPic(W, H) for _ in range(2)]
    for r in rec_inits:
        r.buf[:] = rng.integers(0, 256, r.buf.size, dtype=np.uint8)
    dp, blocks, pos, eob, cnt = run_device(ctx, W, H, srcs, refs, grids, q_index, flags, thr, rec_inits)
    assert cnt[4 + 2] > 0 and cnt[4 + 3] > 0
    qt = E.qindex_tables(q_index)[0]
    for i in range(2):
        rec0 = M.RefPic(W, H)
        rec0.buf[:] = rec_inits[i].buf
        o = M.oracle_encdec_picture(srcs[i], refs, grids[i][0], grids[i][1], q_index, flags, thr, recon_init=rec0)
        # the oracle's own picture reaches the clamp: the DC of a 16x16 and of a 32x32 luma block holds the clamped level, not the other
        for ts in (2, 3):
            k = next(j for j, bl in enumerate(o["blocks"]) if bl["tx_size"] == ts and (int(o["pos"][j]) >> 22) & 3 == 0)
            lvl = abs(int(o["qcoeff"][int(o["blocks"][k]["coeff_off"])]))
            assert lvl == E.level_of(32639, qt, 0, ts == 3) != E.level_of(32639, qt, 0, ts == 3, clamp=False), (ts, lvl)
        d = dp[i]
        assert np.array_equal(d.pred_t.cpu().numpy(), np.concatenate([p.ravel() for p in o["pred"]])), "prediction"
        assert np.array_equal(d.q_t.cpu().numpy(), o["qcoeff"]), ("qcoeff", i)
        assert np.array_equal(d.dq_t.cpu().numpy(), o["dqcoeff"]), ("dqcoeff", i)
        assert np.array_equal(d.emap_t.cpu().numpy().view(np.uint16), o["eob_map"]), "eob map"
        lf_g = d.lf_t.cpu().numpy().view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
        assert np.array_equal(lf_g["skip"], o["lf_mi"]["skip"]), "skip flags"
        if flags.apply_loop_filter:
            assert masks_equal(d.lfm_t.cpu().numpy().view(B.LF_MASK_DTYPE).reshape(o["lfm"].shape), o["lfm"]), "loop-filter masks"
        rec_g = d.rec_t.cpu().numpy()
        assert np.array_equal(rec_g, o["rec"].buf), ("reconstruction", i, int(np.sum(rec_g != o["rec"].buf)))

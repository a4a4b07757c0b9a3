"""CPU: the inverse transform on coefficients no forward transform produces (tests/decode_model.py: coeff_edge_cases) -- the oracle
(oracle_inv_txfm_add on decode_model's dequantised coefficients) against what the reference's own *_add_c kernels reconstructed
(tests/golden/recon_edges_reference.npz, written by tests/gen_golden_recon_edges.py), live against oracle/_ref when that is built, the
conditions on the table of excluded amplitudes, the dequantiser's wrap and 32x32 halving against hand-computed products, and statements that
every family's inputs are what they were built to be.  The GPU counterpart is tests/test_gpu_recon_edges.py."""
import os

import numpy as np
import pytest

import decode_model as D
import svt_testlib as T

B = T.B
GOLDEN = os.path.join(T.GOLDEN_DIR, "recon_edges_reference.npz")


@pytest.fixture(scope="module")
def edge():
    """cases, their dqcoeff and overflow counts, the fixture's bytes per case -- computed once, left unchanged"""
    cases = D.coeff_edge_cases()
    g = np.load(GOLDEN)
    assert [c["name"] for c in cases] == list(g["names"]), "the fixture was written for other cases: python tests/gen_golden_recon_edges.py"
    want, pos = [], 0
    for c in cases:
        n = T.TX_N[c["tx_size"]]
        want.append(g["recon"][pos:pos + n * n].reshape(n, n))
        pos += n * n
    assert pos == g["recon"].size
    dq = [D.case_dqcoeff(c) for c in cases]
    return dict(cases=cases, want=want, dq=[d for d, _ in dq], over=[o for _, o in dq])


def oracle_recon(c, dq):
    return c["pred"] if c["eob"] == 0 else T.oracle_inv_add(dq, c["pred"], c["tx_size"], c["tx_type"], c["eob"])


def test_oracle_equals_the_recorded_reference(edge):
    for c, dq, want in zip(edge["cases"], edge["dq"], edge["want"]):
        assert np.array_equal(oracle_recon(c, dq), want), c["name"]


@pytest.mark.skipif(not T.have_ref("libsvtref_kernels.so"), reason="oracle/_ref not built")
def test_oracle_equals_the_live_reference(edge):
    for c, dq, want in zip(edge["cases"], edge["dq"], edge["want"]):
        assert np.array_equal(T.ref_inv_add(dq, c["pred"], c["tx_size"], c["tx_type"], c["eob"]), want), c["name"]


def test_conditions_on_the_exclusion_table(edge):
    """no DCT_DCT, 32x32 or 4x4 entry; ADST entries of 8x8 and 16x16 only above 2048 (the sanitized reference moved the 8x8 bound of the
    ADST-over-columns types down from 8192: DESIGN.md section 5.17); every (size, type) keeps the 2048 and 300 rungs of every family"""
    for (ts, tt), bound in D.OUTSIDE_DOMAIN_ABOVE.items():
        assert tt != 0 and ts in (1, 2) and bound >= 2048 and bound in D.LADDER, (ts, tt, bound)
    assert D.LADDER[0] == 32767 and D.TOKEN_MAX == 16450 and 2048 in D.LADDER and 300 in D.LADDER
    names = {c["name"] for c in edge["cases"]}
    for ts, tt in D.GROUPS:
        n = T.TX_N[ts]
        for fam in ("dense", "sparse", "uniform"):
            for a in D.LADDER:
                assert (f"{fam}/{n}x{n}/t{tt}/a{a}" in names) == D.in_domain(ts, tt, a), (fam, ts, tt, a)
            assert D.in_domain(ts, tt, 2048) and D.in_domain(ts, tt, 300)
        mine = [c for c in edge["cases"] if (c["tx_size"], c["tx_type"]) == (ts, tt)]
        assert {"dense", "sparse", "uniform", "single", "peak"} <= {c["family"] for c in mine}
        assert all(D.in_domain(ts, tt, c["amplitude"]) for c in mine)
        assert 20 <= len(mine) <= 70, (ts, tt, len(mine))                    # (kept small: a few hundred blocks in all)
        if ts == 0 or tt == 0:
            assert {"q255", "q0"} <= {c["family"] for c in mine}
    assert len(edge["cases"]) < 700


def test_dequantise_against_hand_computed_products():
    """DC with dequant[0], AC with dequant[1], the wrap to 16 bits, 32x32: the product halved TOWARDS ZERO, then wrapped"""
    qt = np.zeros(1, dtype=B.QUANT_DTYPE)
    qt[0]["dequant"] = (1336, 1828)                                         # q index 255's luma steps
    assert list(D.qindex_tables(255)[0]["dequant"]) == [1336, 1828]
    rows = [  # qcoeff DC, qcoeff AC -> 8x8 (dq DC, dq AC, overflows), 32x32 (dq DC, dq AC, overflows)
        (1, -1, (1336, -1828, 0), (668, -914, 0)),
        (24, 17, (32064, 31076, 0), (16032, 15538, 0)),
        (25, 18, (33400 - 65536, 32904 - 65536, 2), (16700, 16452, 0)),
        (-25, -18, (-33400 + 65536, -32904 + 65536, 2), (-16700, -16452, 0)),
        (16450, -16450, (21977200 - 335 * 65536, -30070600 + 459 * 65536, 2), (10988600 - 168 * 65536, -15035300 + 229 * 65536, 2)),
        (-32768, 32767, (-43778048 + 668 * 65536, 59898076 - 914 * 65536, 2), (-21889024 + 334 * 65536, 29949038 - 457 * 65536, 2)),
    ]
    for qdc, qac, want8, want32 in rows:
        for n, want in ((8, want8), (32, want32)):
            q = np.zeros(n * n, np.int16)
            q[0], q[1:] = qdc, qac
            dq, over = D.dequantise_one(q, n, qt[0]["dequant"])
            assert -32768 <= want[0] <= 32767 and -32768 <= want[1] <= 32767
            assert (int(dq[0]), int(dq[1]), int(dq[-1])) == (want[0], want[1], want[1]), (qdc, qac, n)
            assert over == (want[2] and (1 if want[2] == 1 else n * n)), (qdc, qac, n)
            blocks = np.zeros(1, dtype=B.TQ_BLOCK_DTYPE)
            blocks[0]["tx_size"] = {8: 1, 32: 3}[n]
            wdq, wover = D.dequantise(q, blocks, qt)                        # the list form the GPU tests count with is the same rule
            assert np.array_equal(wdq, dq) and wover == over
    # the halving of negative odd products: towards zero, where an arithmetic shift goes down
    for qv, step, want, floor in ((-1, 3, -1, -2), (-3, 3, -4, -5), (-1, 5, -2, -3), (-3, 5, -7, -8), (3, 5, 7, 7), (-2, 3, -3, -3)):
        q = np.full(1024, qv, np.int16)
        assert int(D.dequantise_one(q, 32, (step, step))[0][5]) == want and int(D.dequantise_one(q, 32, (step, step), floor_half=True)[0][5]) == floor
        assert int(D.dequantise_one(q[:64], 8, (step, step))[0][5]) == qv * step          # (no halving below 32x32)


def test_overflowing_products_are_where_they_were_put(edge):
    fam_over = {}
    for c, o in zip(edge["cases"], edge["over"]):
        fam_over.setdefault(c["family"], []).append(o)
        if c["qtab"] in (D.QT_ONE, D.QT_TWO):                               # dqcoeff set directly: nothing to wrap, whatever the amplitude
            assert o == 0, c["name"]
            assert np.array_equal(edge["dq"][edge["cases"].index(c)], c["qcoeff"]), c["name"]
    assert all(o > 0 for o in fam_over["q255"]) and all(o > 0 for o in fam_over["q0"])
    for fam in ("dense", "sparse", "uniform", "single", "peak", "shortcuts", "half"):
        assert sum(fam_over[fam]) == 0, fam
    # the ladder reaches both ends of int16
    top = [c for c in edge["cases"] if c["family"] == "dense" and c["amplitude"] == 32767]
    assert top and all(c["qcoeff"].min() == -32768 and c["qcoeff"].max() == 32767 for c in top)


def test_half_cases_differ_from_their_floor_divided_twins(edge):
    """every product of a `half` block is negative and odd, and reconstructing with product >> 1 in place of product / 2 changes bytes"""
    half = [c for c in edge["cases"] if c["family"] == "half"]
    assert len(half) >= 8
    qt = D.edge_qtabs()
    for c in half:
        assert c["tx_size"] == 3
        step = np.full(1024, int(qt[c["qtab"]]["dequant"][1]))
        step[0] = int(qt[c["qtab"]]["dequant"][0])
        p = c["qcoeff"].astype(np.int64) * step
        nz = p[c["qcoeff"] != 0]
        assert nz.size > 100 and (nz < 0).all() and (nz & 1).all(), c["name"]
        a, b = D.case_dqcoeff(c)[0], D.case_dqcoeff(c, floor_half=True)[0]
        assert np.array_equal(b[c["qcoeff"] != 0], a[c["qcoeff"] != 0] - 1)
        ra, rb = oracle_recon(c, a), oracle_recon(c, b)
        assert ra.ravel()[c["sample"]] != rb.ravel()[c["sample"]], c["name"]


def test_peak_cases_saturate_the_targeted_sample(edge):
    """below the cast: polarity + over a prediction of 0 gives 255 in the sample, polarity - over 255 gives 0; past the cast (`over`) the
    column result has wrapped and the sample moved the other way"""
    peak = [c for c in edge["cases"] if c["family"] == "peak"]
    seen = set()
    for c in peak:
        i = edge["cases"].index(c)
        got = int(edge["want"][i].ravel()[c["sample"]])
        if c["over"]:
            assert got == (0 if c["polarity"] > 0 else 255), c["name"]
        elif "_p0_" in c["name"] and c["polarity"] > 0:
            assert got == 255, c["name"]
            seen.add((c["tx_size"], c["tx_type"], c["sample"] == 0, 1))
        elif "_p255_" in c["name"] and c["polarity"] < 0:
            assert got == 0, c["name"]
            seen.add((c["tx_size"], c["tx_type"], c["sample"] == 0, -1))
    assert len(seen) == 4 * len(D.GROUPS)


@pytest.mark.parametrize("name", ["q0_blocks", "q255_noise", "thin_32x104"])
def test_decode_intra_picture_rebuilds_a_recorded_key_frame(name):
    """the block-by-block CPU walk the GPU test of the intra wavefront compares with, pinned first: from the grid, qcoeff and eob map the
    REFERENCE recorded for a case of tests/golden/intra_reference.npz it rebuilds that case's prediction and reconstruction"""
    import encdec_model as M
    case = next(c for c in M.INTRA_GOLDEN_CASES if c[0] == name)
    _, W, H, _, q_index, _ = case
    g = M.intra_golden()[name]
    _, mi = M.intra_golden_inputs(case)
    assert mi.tobytes() == g["mi"].tobytes()
    pred, rec, over = D.decode_intra_picture(mi, W, H, g["qcoeff"], g["eob_map"], D.qindex_tables(q_index))
    assert over == 0
    assert np.array_equal(np.concatenate([p.ravel() for p in pred]), g["pred"]) and np.array_equal(np.concatenate([p.ravel() for p in rec]), g["rec"])
    assert {b[3] for b in D.intra_walk(mi, W, H)} >= ({4, 8, 16, 32} if W >= 64 else {4, 8})


def test_crafted_key_frame_holds_what_it_was_built_to_hold():
    """the key frame of the GPU test: all four sizes, ADST blocks of every size below 32 with coefficients inside their type's domain
    (crafted_coefficients asserts the bound per block), DCT blocks whose products wrap at q index 255, blocks with eob 0 that hold
    coefficients; and the walk saturates: the reconstruction the neighbours predict from reaches 0 and 255"""
    import encdec_model as M
    W, H = D.KEY_FRAME[:2]
    mi = M.gen_intra_grid(D.KEY_FRAME[2], W, H, sizes=(4, 8, 16, 32))
    walk = D.intra_walk(mi, W, H)
    assert {b[3] for b in walk} == {4, 8, 16, 32} and {(b[3], b[5]) for b in walk if b[5]} == {(n, tt) for n in (4, 8, 16) for tt in (1, 2, 3)}
    for q_index in (0, 255):
        q, emap, recs = D.crafted_coefficients([b[:4] + (b[5],) for b in walk], q_index, W, H, seed=q_index)
        assert sum(1 for e, qv, _ in recs if e == 0 and qv.any()) >= 5
        pred, rec, over = D.decode_intra_picture(mi, W, H, q, emap, D.qindex_tables(q_index))
        assert over > (100 if q_index else 0)         # (step 4 wraps only the top rungs)
        flat = np.concatenate([p.ravel() for p in rec])
        assert (flat == 0).mean() > 0.05 and (flat == 255).mean() > 0.05 and all((p == 0).any() and (p == 255).any() for p in rec)


def test_shortcut_eobs_sit_on_their_side_of_each_threshold(edge):
    """every eob of THRESHOLD_EOBS occurs for its size at both amplitudes, coefficients only in the first eob scan positions with the last
    of them non-zero, and the pair (e, e + 1) straddles a dispatch threshold of VPX/vp9_idct.c"""
    scans = T.scan_tables()
    limits = {0: (1,), 1: (1, 12), 2: (1, 10, 38), 3: (1, 34, 135)}
    for ts in range(4):
        assert set(D.THRESHOLD_EOBS[ts]) == {e for l in limits[ts] for e in (l, l + 1)}
        scan = np.argsort(scans[f"iscan_{ts}_0"])
        for e in D.THRESHOLD_EOBS[ts]:
            mine = [c for c in edge["cases"] if c["family"] == "shortcuts" and c["tx_size"] == ts and c["eob"] == e and "dc_only" not in c["name"]]
            assert sorted(c["amplitude"] for c in mine) == [300, 32767], (ts, e)
            for c in mine:
                assert (c["qcoeff"][scan[:e]] != 0).all() and not c["qcoeff"][scan[e:]].any(), c["name"]
        dc = sorted(int(c["qcoeff"][0]) for c in edge["cases"] if c["family"] == "shortcuts" and c["tx_size"] == ts and "dc_only" in c["name"])
        assert dc == [-32768, -1, 1, 32767]

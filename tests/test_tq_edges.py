"""CPU: the forward transform stage's edge cases (tests/tq_edges_model.py) -- the list's own conditions, the oracle against the reference's
recorded outputs (tests/golden/tq_edges_reference.npz, written by tests/gen_golden_tq_edges.py from the reference's C functions, whose
sanitized build ran clean on every case), the live reference where oracle/_ref is built, and the windows in which clamp16 of the quantiser
decides a level.  No GPU."""
import os

import numpy as np
import pytest

import svt_testlib as T
import tq_edges_model as E

GOLD = os.path.join(T.GOLDEN_DIR, "tq_edges_reference.npz")
KEYS = ("coeff", "qcoeff", "dqcoeff", "eob")


@pytest.fixture(scope="module")
def gold():
    assert os.path.getsize(GOLD) < 512 * 1024
    return dict(np.load(GOLD))          # (every array decompressed once)


def _split(g, cases):
    pos = 0
    for i, c in enumerate(cases):
        nn = T.TX_N[c["tx_size"]] ** 2
        yield g["coeff"][pos:pos + nn], g["qcoeff"][pos:pos + nn], g["dqcoeff"][pos:pos + nn], int(g["eob"][i])
        pos += nn


def test_list_conditions():
    """fewer than 2500 blocks; every (size, type) in basis, ladder and zero-bin; the peak coefficient of every size; a block of energy >=
    1e9; levels up to the CAT6 table's reach and no further; both sides of every dead-zone boundary with the level 0 below it and non-zero
    on it; clamp cases where the clamped and the unclamped level differ; more 4x4 blocks than one workgroup of the lane form takes"""
    f = E.check_conditions()
    print(f)
    assert f["peak"] == E.PEAK and f["energy"] >= 10 ** 9 and 8000 <= f["top_level"] <= E.MAX_LEVEL and f["blocks"] < 2500
    cases = E.edge_cases()
    assert {c["family"] for c in cases} == {"basis", "ladder", "first", "zbin", "clamp"}
    big = [c for c in cases if c["tx_size"] == 3]
    assert sum(c["partial32"] for c in big) * 2 == len(big)
    for c in cases:                                       # real bytes on both sides, residual within +-255
        assert c["src"].dtype == np.uint8 and c["pred"].dtype == np.uint8 and c["src"].shape == (T.TX_N[c["tx_size"]],) * 2


def test_oracle_equals_the_recorded_reference(gold):
    cases, outs = E.edge_cases(), E.oracle_outputs()
    assert [c["name"] for c in cases] == list(gold["names"])
    bad = [(c["name"], k) for c, o, r in zip(cases, outs, _split(gold, cases)) for k, a, b in zip(KEYS, o, r) if not np.array_equal(a, b)]
    assert not bad, (len(bad), bad[:8])


def test_live_reference_equals_the_fixture(gold):
    import gen_golden_tq_edges as G
    if not os.path.exists(G.PLAIN):
        pytest.skip("oracle/_ref/ref_fwdtq is not built (needs the reference's sources)")
    cases = E.edge_cases()
    want = G.pack(cases, G.reference_outputs(cases))
    for k in want:
        assert np.array_equal(want[k], gold[k]), k


def test_clamp_cases_differ_from_the_unclamped_formula(gold):
    """the recorded reference holds the CLAMPED level at every clamp case, and the unclamped formula gives another one (except at the two
    32x32 steps kept as reached-but-equivalent); the windows of tq_edges_model's docstring"""
    cases = E.edge_cases()
    seen = {2: 0, 3: 0}
    for c, r in zip(cases, _split(gold, cases)):
        if c["family"] != "clamp":
            continue
        is32 = c["tx_size"] == 3
        a = abs(int(r[0][0]))
        assert a == 32639
        assert abs(int(r[1][0])) == E.level_of(a, c["qt"], 0, is32)
        if not c["equivalent"]:
            assert E.level_of(a, c["qt"], 0, is32) != E.level_of(a, c["qt"], 0, is32, clamp=False), c["name"]
            seen[c["tx_size"]] += 1
    assert seen[2] >= 6 and seen[3] >= 6
    q684, q700 = T.quant_table(684, 1828), T.quant_table(700, 1828)
    assert (E.level_of(32639, q684, 0, False), E.level_of(32639, q684, 0, False, clamp=False)) == (47, 48)
    assert (E.level_of(32639, q700, 0, False), E.level_of(32639, q700, 0, False, clamp=False)) == (46, 47)
    for s, lvl in ((700, 93), (1336, 49)):
        q = T.quant_table(s, 1828)
        assert E.level_of(32639, q, 0, True) == E.level_of(32639, q, 0, True, clamp=False) == lvl
    w = E.clamp_windows()
    assert (w[(2, "steps")][0][0], len(w[(2, "steps")][1]), w[(2, "steps")][1][0], w[(2, "steps")][1][-1]) == (344, 198, 395, 1325)
    assert (w[(3, "steps")][0][0], len(w[(3, "steps")][1]), w[(3, "steps")][1][:2], w[(3, "steps")][1][-1]) == (686, 67, [771, 790], 1315)
    assert w[(2, "qindex")][0][0] == 191 and w[(2, "qindex")][1] == [201, 214, 215, 217, 218, 234, 235, 242, 249, 250, 251]
    assert w[(3, "qindex")][0][0] == 235 and w[(3, "qindex")][1] == [E.REAL_Q_INDEX]


def test_layouts_are_well_formed():
    """the two descriptor layouts of the GPU tests: blocks grouped by size, disjoint, inside their buffers; the unlike layout's strides
    pairwise different with all four residues mod 16, one block per size at 65532, every pointer on the vector path while another is not"""
    cases = E.edge_cases()
    L = E.packed_layout(cases)
    assert int(L["counts"].sum()) == len(cases) and (np.diff(L["blocks"]["tx_size"].astype(int)) >= 0).all() and len(L["qtabs"]) <= 256
    assert L["counts"][0] > 256
    for sets in (1, 2):
        U = E.unlike_layout(cases, recon_sets=sets)
        b = U["blocks"]
        picked = [cases[i] for i in U["idx"]]
        assert {(c["tx_size"], c["tx_type"]) for c in picked} == set(E.GROUPS)
        assert any(c["family"] == "clamp" for c in picked) and any("/flat/+255" in c["name"] for c in picked)
        st = np.stack([b["src_stride"], b["pred_stride"], b["recon_stride"]], 1).astype(int)
        assert (st[:, 0] != st[:, 1]).all() and (st[:, 0] != st[:, 2]).all() and (st[:, 1] != st[:, 2]).all()
        assert {int(s) % 16 for s in st.ravel()} == {0, 4, 8, 12}
        for ts in range(4):
            assert (st[b["tx_size"] == ts] == 65532).any(), ts
        assert (b["src_off"] != b["pred_off"]).any() and (b["src_off"] != b["recon_off"]).any()
        census = E.alignment_census(U)
        for ts in (1, 2, 3):
            assert census[ts] == {0, 1, 2}, (ts, census)
        assert U["src"].size < 3 * 2 ** 20

"""Inputs of the reconstruction-kernel tests (tests/test_gpu_decode.py), built on the CPU: transform blocks whose eob -- as the oracle's
forward path (tests/svt_testlib.py: oracle_tq_batch) gives it -- falls on chosen values, laid out in planes with strides that are no
multiple of 16 and block origins that alternate between 4-, 8- and 16-byte alignment.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np

import svt_testlib as T

B = T.B

# eobs on each side of every shortcut of the inverse DCT (VPX/vp9_idct.c:111-189): DC only; 4 of 8 rows; 4 / 8 of 16; 8 / 16 of 32
THRESHOLD_EOBS = {0: (1, 2), 1: (1, 2, 12, 13), 2: (1, 2, 10, 11, 38, 39), 3: (1, 2, 34, 35, 135, 136)}
# q index 0 (step 4, zero bin 2): the forward transform of an integer residual that is not constant over the block leaves coefficients of
# +-2 far down the scan, so a block's eob there is 0, 1 or far beyond every threshold -- except for 4x4, where 2 occurs.  Seeded searches
# over smooth, sparse, stepped and sign-pattern residuals (thousands per size) found none of these; they are asked for at 120 and 255.
UNREACHED_AT_Q0 = {1: (2, 12, 13), 2: (2, 10, 11, 38, 39), 3: (2, 34, 35, 135, 136)}
GROUPS = [(ts, tt) for ts in range(4) for tt in (range(4) if ts < 3 else (0,))]          # every size with every type it allows
PER_GROUP = 48
GUARD = 0xA5


def qindex_tables(q_index):
    """[luma, chroma] tables of a q index (svt_hip_quant_tables_for_qindex: pinned against eb_vp9_init_quantizer by tests/test_tq_params.py)"""
    qt = np.zeros(2, dtype=B.QUANT_DTYPE)
    assert B.load().svt_hip_quant_tables_for_qindex(q_index, qt.ctypes.data_as(C.c_void_p)) == 0
    return qt


def _basis(n):
    k = np.arange(n)
    m = np.cos(np.pi * (2 * k[None, :] + 1) * k[:, None] / (2 * n))      # m[frequency, sample]
    m[0] *= np.sqrt(0.5)
    return m


def _candidate(rng, ts, scan, target):
    """a residual whose energy sits in the first `target` scan positions (the last of them strong), as an int array within +-100 (amplitudes
    log-uniform from 0.6: the small ones give the short eobs at the fine quantisers)"""
    n = T.TX_N[ts]
    coef = np.zeros(n * n)
    k = np.arange(target)
    coef[scan[:target]] = rng.choice((-1.0, 1.0), target) * rng.uniform(0.3, 1.0, target) / (1 + 0.05 * k)
    coef[scan[target - 1]] = rng.choice((-1.0, 1.0)) * rng.uniform(0.8, 1.6)
    m = _basis(n)
    res = m.T @ coef.reshape(n, n) @ m
    return np.rint(res * (np.exp(rng.uniform(np.log(0.6), np.log(100))) / max(1e-9, np.abs(res).max()))).astype(np.int64)


def _pool(rng, ts, tt, q_index, scan, per_target=60):
    """candidate (pred, src) pairs of one (size, type) and the eob the oracle's forward path gives each at q_index"""
    n = T.TX_N[ts]
    want = list(THRESHOLD_EOBS[ts]) + [int(v) for v in rng.integers(1, n * n + 1, 4)]
    preds, srcs = [], []
    for target in want:
        for _ in range(per_target):
            pred = np.clip(128 + rng.integers(-20, 21, (n, n)), 0, 255)
            preds.append(pred.astype(np.uint8))
            srcs.append(np.clip(pred + _candidate(rng, ts, scan, target), 0, 255).astype(np.uint8))
    nb = len(preds)
    blocks = np.zeros(nb, dtype=B.TQ_BLOCK_DTYPE)
    iscan, offs = T.iscan_array()
    for i in range(nb):
        blocks[i] = (i * n * n, i * n * n, i * n * n, i * n * n, offs[(ts, tt)], n, n, n, ts, tt, 0, 0, 0, 0)
    case = dict(src=np.concatenate([s.ravel() for s in srcs]), pred=np.concatenate([p.ravel() for p in preds]), blocks=blocks,
                qtabs=qindex_tables(q_index), iscan=iscan, n_coeff=nb * n * n)
    eob = T.oracle_tq_batch(case)[3]
    return preds, srcs, eob


def block_case(q_index, seed=2024):
    """PER_GROUP blocks of every (size, type) at q_index: for DCT_DCT one block at every eob of THRESHOLD_EOBS (found among seeded candidates
    with the oracle's forward path -- an assertion, not a hope), four whose residual is +-255 in every sample, four flat ones (source =
    prediction: eob 0), the rest seeded candidates; luma and chroma tables alternate.  Returns the dict svt_testlib's transform helpers take,
    plus `want_eob` (the oracle's eob of every block, list order) and `groups` ((size, type) of every block)."""
    rng = np.random.default_rng(seed + q_index)
    scans = T.scan_tables()
    iscan, offs = T.iscan_array()
    chosen = []                                      # (ts, tt, pred, src, oracle eob or None)
    for ts, tt in GROUPS:
        n = T.TX_N[ts]
        scan = np.argsort(scans[f"iscan_{ts}_{tt}"])
        preds, srcs, eob = _pool(rng, ts, tt, q_index, scan)
        picked = []
        if tt == 0:
            for e in THRESHOLD_EOBS[ts]:
                if q_index == 0 and e in UNREACHED_AT_Q0.get(ts, ()):
                    continue
                hit = np.flatnonzero(eob == e)
                assert hit.size, f"no candidate with eob {e} for {n}x{n} at q index {q_index}"
                picked.append(int(hit[0]))
        rest = [int(i) for i in rng.permutation(len(preds)) if int(i) not in picked]
        picked += rest[:PER_GROUP - 8 - len(picked)]
        group = [(ts, tt, preds[i], srcs[i], int(eob[i])) for i in picked]
        for _ in range(4):                            # all +-255: prediction 0 / 255 per sample, source the opposite
            pred = np.where(rng.integers(0, 2, (n, n)) > 0, 255, 0).astype(np.uint8)
            group.append((ts, tt, pred, (255 - pred).astype(np.uint8), None))
        for _ in range(4):                            # flat: nothing to code
            pred = rng.integers(0, 256, (n, n)).astype(np.uint8)
            group.append((ts, tt, pred, pred.copy(), 0))
        assert len(group) == PER_GROUP
        chosen += [group[i] for i in rng.permutation(PER_GROUP)]
    # the planes: rows of blocks; a block's origin advances by its size + 4, so origins are 4-byte aligned and alternate between being and
    # not being 8- / 16-byte aligned; the stride is 4 x an odd number; guard bytes everywhere else
    stride = 4 * 173
    x, y, row_h, place = 4, 3, 0, []
    for ts, tt, pred, src, e in chosen:
        n = T.TX_N[ts]
        if x + n + 4 > stride:
            x, y, row_h = 4, y + row_h + 3, 0
        place.append((y, x))
        x, row_h = x + n + 4, max(row_h, n)
    height = y + row_h + 3
    src_p = np.full((height, stride), GUARD, np.uint8)
    pred_p = rng.integers(0, 256, (height, stride)).astype(np.uint8)
    blocks = np.zeros(len(chosen), dtype=B.TQ_BLOCK_DTYPE)
    pos = 0
    for i, ((ts, tt, pred, src, e), (by, bx)) in enumerate(zip(chosen, place)):
        n = T.TX_N[ts]
        src_p[by:by + n, bx:bx + n], pred_p[by:by + n, bx:bx + n] = src, pred
        o = by * stride + bx
        blocks[i] = (o, o, o, pos, offs[(ts, tt)], stride, stride, stride, ts, tt, i & 1, 1, 0, 0)
        pos += n * n
    counts = np.array([sum(PER_GROUP for g in GROUPS if g[0] == s) for s in range(4)], dtype=np.int32)
    return dict(src=src_p, pred=pred_p, blocks=blocks, counts=counts, qtabs=qindex_tables(q_index), iscan=iscan, n_coeff=pos,
                want_eob=[c[4] for c in chosen], groups=[c[:2] for c in chosen], place=place)


def dequantise(q, blocks, qtabs):
    """(wrapped int16 dqcoeff, number of coefficients whose product did not fit) of every block with the rule of the encode pass and of a
    non-high-bit-depth decoder: DC dequant[0], AC dequant[1], 32x32 the product / 2 towards zero"""
    dq = np.zeros_like(q)
    over = 0
    for b in blocks:
        n = T.TX_N[int(b["tx_size"])]
        o = int(b["coeff_off"])
        step = np.full(n * n, int(qtabs[int(b["qtab"])]["dequant"][1]), np.int64)
        step[0] = int(qtabs[int(b["qtab"])]["dequant"][0])
        p = q[o:o + n * n].astype(np.int64) * step
        if n == 32:
            p = np.sign(p) * (np.abs(p) // 2)
        over += int(np.count_nonzero((p < -32768) | (p > 32767)))
        dq[o:o + n * n] = p.astype(np.int16)          # (wraps)
    return dq, over

"""Inputs of the reconstruction-kernel tests (tests/test_gpu_decode.py), built on the CPU: transform blocks whose eob -- as the oracle's
forward path (tests/svt_testlib.py: oracle_tq_batch) gives it -- falls on chosen values, laid out in planes with strides that are no
multiple of 16 and block origins that alternate between 4-, 8- and 16-byte alignment; and, second half, coefficients NO forward transform
produces (coeff_edge_cases, for tests/test_recon_edges.py and tests/test_gpu_recon_edges.py) with CPU walks of whole pictures built on
oracle_inv_txfm_add (decode_intra_picture, decode_inter_picture).  Nothing here needs a GPU."""
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


# ---------------------------------------------------------------------------------------------------------------------------------------
# coefficients no forward transform produces (tests/test_recon_edges.py, tests/test_gpu_recon_edges.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
import boolcode_model as _BM                                               # noqa: E402
import tokenize_model as _TM                                               # noqa: E402

# the largest magnitude a coefficient token carries: the last category's base (csrc/tokenize_core.h: svt_tok_base) plus all of its extra
# bits set (csrc/boolcode_core.h: svt_bool_cat_bits, read back by csrc/read_core.h / host/frame_read.c); the two models restate those headers
TOKEN_MAX = _TM.CAT_BASE[-1] + (1 << _BM.CAT_BITS[len(_TM.CAT_BASE) - 1]) - 1
LADDER = (32767, TOKEN_MAX, 8192, 2048, 300)
# Amplitudes of |dqcoeff| above which a (size, type) is OUTSIDE the domain in which the C reference is defined: the 8- and 16-point inverse
# ADST add several 32-bit products in int32_t, and beyond these bounds the sum overflows in the reference itself (its sanitized build,
# oracle/_ref/ref_invtx_ubsan, run by tests/gen_golden_recon_edges.py: DESIGN.md section 5.17).  A case whose amplitude exceeds its entry is
# not generated.  No DCT_DCT, 32x32 or 4x4 entry: every stored step of the inverse DCT is int16 and every product fits.  Each bound is the
# largest rung of LADDER at which the sanitized reference stayed clean on 9000 random blocks of the type (the generator's probe): an ADST
# over the columns (types 1, 3) meets the row pass's wrapped outputs and gives way one rung sooner than an ADST over the rows alone (type 2).
OUTSIDE_DOMAIN_ABOVE = {(1, 1): 2048, (1, 2): TOKEN_MAX, (1, 3): 8192, (2, 1): 2048, (2, 2): 8192, (2, 3): 2048}
# the table every case's `qtab` indexes: (1, 1) sets dqcoeff = qcoeff for 4x4..16x16, (2, 2) for 32x32 (q * 2 / 2); the real tables of q
# index 0 and 255 (luma, chroma); (3, 3), (5, 5), (3, 5): odd steps for the 32x32 halving
DIRECT_STEPS = ((1, 1), (2, 2))
HALF_STEPS = ((3, 3), (5, 5), (3, 5))
QT_ONE, QT_TWO, QT_Q0, QT_Q255, QT_HALF = 0, 1, 2, 4, 6


def edge_qtabs():
    qt = np.zeros(6 + len(HALF_STEPS), dtype=B.QUANT_DTYPE)
    for i, st in enumerate(DIRECT_STEPS):
        qt[i]["dequant"] = st
    qt[QT_Q0:QT_Q0 + 2], qt[QT_Q255:QT_Q255 + 2] = qindex_tables(0), qindex_tables(255)
    for i, st in enumerate(HALF_STEPS):
        qt[QT_HALF + i]["dequant"] = st
    return qt


def in_domain(ts, tt, amplitude):
    return amplitude <= OUTSIDE_DOMAIN_ABOVE.get((ts, tt), 32768)


def dequantise_one(q, n, steps, floor_half=False):
    """(wrapped int16 dqcoeff, overflow count) of one raster block; floor_half: the 32x32 product >> 1 instead of / 2 (the twin the `half`
    family is built to differ from)"""
    step = np.full(n * n, int(steps[1]), np.int64)
    step[0] = int(steps[0])
    p = q.astype(np.int64) * step
    if n == 32:
        p = p >> 1 if floor_half else np.sign(p) * (np.abs(p) // 2)
    return p.astype(np.int16), int(np.count_nonzero((p < -32768) | (p > 32767)))


_response_cache = {}


def impulse_signs(ts, tt):
    """sign[k, s] of coefficient k's response at output sample s, measured: an impulse of 2048 at k through oracle_inv_txfm_add over a flat
    prediction of 128 (0 where the response rounds to nothing)"""
    if (ts, tt) not in _response_cache:
        n = T.TX_N[ts]
        flat = np.full((n, n), 128, np.uint8)
        sg = np.zeros((n * n, n * n), np.int8)
        for k in range(n * n):
            dq = np.zeros(n * n, np.int16)
            dq[k] = 2048
            sg[k] = np.sign(T.oracle_inv_add(dq, flat, ts, tt, n * n).astype(np.int32).ravel() - 128)
        _response_cache[(ts, tt)] = sg
    return _response_cache[(ts, tt)]


def _peak_layout(ts, tt, sample, polarity):
    """+-1 per coefficient so that every response adds up at `sample` (raster index) with the sign `polarity`"""
    sg = impulse_signs(ts, tt)[:, sample].astype(np.int64)
    return np.where(sg == 0, 1, sg) * polarity


def _peak_amplitude(ts, tt, layout, sample):
    """the amplitude at which the column result of `sample` reaches 0.9 of the int16 range before the rounding shift, from the gain
    measured at amplitudes small enough to stay linear (residual within the clip of a flat 128)"""
    n = T.TX_N[ts]
    shift = {0: 4, 1: 5, 2: 6, 3: 6}[ts]
    flat = np.full((n, n), 128, np.uint8)
    a = 1
    while True:
        r = int(T.oracle_inv_add((layout * a).astype(np.int16), flat, ts, tt, n * n).ravel()[sample]) - 128
        if abs(r) >= 48:
            break
        a += 1
        assert a < 2048
    assert abs(r) < 127
    return int(0.9 * 32767 / (abs(r) / a * (1 << shift)))


def coeff_edge_cases(seed=4242):
    """Named blocks whose coefficients no forward transform and quantiser produce.  Each case: name, family, tx_size, tx_type, eob, pred
    (N x N bytes), qcoeff (N * N, raster), qtab (index into edge_qtabs()), amplitude (the bound of |dqcoeff| the case was built at: what
    OUTSIDE_DOMAIN_ABOVE is compared with; 32767 for the real tables, whose products wrap anywhere), and for `peak` / `half` the target
    sample and polarity.  Deterministic.  Families, for every size with every type it allows: dense / sparse (one in eight) / uniform on
    LADDER; single coefficients at DC, three corners and an interior position; peak: signs measured with impulses so that every response
    adds up in one sample (a corner, an interior one; both polarities; prediction 0, 255, noise), at the amplitude that brings the column
    result to 0.9 of the int16 range and, `over`, 1.3 times that: past the final cast; shortcuts (DCT_DCT): every eob of THRESHOLD_EOBS with
    coefficients in the first eob scan positions at 32767 and 300, and DC-only blocks of -32768, -1, 1, 32767; half (32x32): products that
    are all negative and odd, laid out so that every half-unit difference between / 2 and >> 1 moves one sample the same way; q255 / q0:
    coefficients at the token maximum through the real tables.  """
    rng = np.random.default_rng(seed)
    scans = T.scan_tables()
    cases = []

    def ends(sign):                                   # the ladder's top rung reaches both ends of int16
        return np.where(sign < 0, -32768, 32767)

    def level(sign, a):
        return ends(sign) if a == 32767 else sign * a

    def add(family, label, ts, tt, eob, pred, q, qtab=None, amplitude=0, **extra):
        n = T.TX_N[ts]
        if not in_domain(ts, tt, amplitude):
            return
        qtab = (QT_TWO if ts == 3 else QT_ONE) if qtab is None else qtab
        cases.append(dict(name=f"{family}/{n}x{n}/t{tt}/{label}", family=family, tx_size=ts, tx_type=tt, eob=int(eob), pred=np.ascontiguousarray(pred, np.uint8),
                          qcoeff=np.ascontiguousarray(q, np.int64).astype(np.int16).ravel(), qtab=qtab, amplitude=amplitude, **extra))

    for ts, tt in GROUPS:
        n = T.TX_N[ts]
        nn = n * n
        noise = lambda: rng.integers(0, 256, (n, n)).astype(np.uint8)      # noqa: E731
        sign = lambda: rng.choice((-1, 1), nn)                              # noqa: E731
        for a in LADDER:
            add("dense", f"a{a}", ts, tt, nn, noise(), level(sign(), a), amplitude=a)
            add("sparse", f"a{a}", ts, tt, nn, noise(), np.where(rng.random(nn) < 0.125, level(sign(), a), 0), amplitude=a)
            u = rng.integers(-a, a + 1, nn)
            if a == 32767:
                u[rng.integers(0, nn, 2)] = (-32768, 32767)
            add("uniform", f"a{a}", ts, tt, nn, noise(), u, amplitude=a)
        rungs = [a for a in LADDER if in_domain(ts, tt, a)]
        spots = (("dc", 0, 0), ("top_right", 0, n - 1), ("bottom_left", n - 1, 0), ("bottom_right", n - 1, n - 1), ("interior", n // 2 - 1, n // 2))
        for i, (label, r, c) in enumerate(spots):
            a = rungs[i % len(rungs)]
            q = np.zeros(nn, np.int64)
            q[r * n + c] = level(np.int64(-1 if i & 1 else 1), a)
            add("single", f"{label}_a{a}", ts, tt, nn, noise(), q, amplitude=a)
        for label, s in (("corner", 0), ("interior", (n // 2) * n + n // 2 - 1)):
            for pol in (1, -1):
                lay = _peak_layout(ts, tt, s, pol)
                a = _peak_amplitude(ts, tt, lay, s)
                for pname, pred in (("p0", np.zeros((n, n), np.uint8)), ("p255", np.full((n, n), 255, np.uint8)), ("noise", noise())):
                    add("peak", f"{label}_{'pos' if pol > 0 else 'neg'}_{pname}_a{a}", ts, tt, nn, pred, lay * a, amplitude=a, sample=s, polarity=pol, over=False)
                over = a * 13 // 10                                         # the same layout past the cast: the column result wraps
                add("peak", f"{label}_{'pos' if pol > 0 else 'neg'}_over_a{over}", ts, tt, nn, noise(), lay * over, amplitude=over, sample=s, polarity=pol, over=True)
        if tt == 0:
            scan = np.argsort(scans[f"iscan_{ts}_0"])
            for e in THRESHOLD_EOBS[ts]:
                for a in (32767, 300):
                    q = np.zeros(nn, np.int64)
                    q[scan[:e]] = level(rng.choice((-1, 1), e), a)
                    add("shortcuts", f"eob{e}_a{a}", ts, tt, e, noise(), q, amplitude=a)
            for v in (-32768, -1, 1, 32767):
                q = np.zeros(nn, np.int64)
                q[0] = v
                add("shortcuts", f"dc_only_{v}", ts, tt, 1, noise(), q, amplitude=abs(v))
        if ts == 3:
            for label, s in (("corner", 0), ("interior", (n // 2) * n + n // 2 - 1)):
                for k, (qv, st) in enumerate(((-1, 0), (-3, 0), (-1, 1), (-3, 1), (-3, 2))):
                    lay = _peak_layout(ts, tt, s, 1)
                    pull = -1 if np.count_nonzero(lay < 0) > nn // 2 else 1  # the larger half of the layout: at the corner every response is positive
                    q = np.where(lay == pull, qv, 0)                        # every product negative and odd, every half-unit difference moves the sample one way
                    add("half", f"{label}_q{-qv}_s{k}", ts, tt, nn, np.full((n, n), 128, np.uint8), q, qtab=QT_HALF + st, amplitude=3 * 5, sample=s, polarity=1)
        for qname, base in (("q255", QT_Q255), ("q0", QT_Q0)):
            for k, shape in enumerate(("dense", "sparse")):
                q = sign() * TOKEN_MAX
                if shape == "sparse":
                    q = np.where(rng.random(nn) < 0.125, q, 0)
                    q[0] = TOKEN_MAX                                        # (the DC step is its own)
                add(qname, shape, ts, tt, nn, noise(), q, qtab=base + k, amplitude=32767)
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def case_dqcoeff(c, qtabs=None, floor_half=False):
    qtabs = edge_qtabs() if qtabs is None else qtabs
    return dequantise_one(c["qcoeff"], T.TX_N[c["tx_size"]], qtabs[c["qtab"]]["dequant"], floor_half)


def edge_block_case(cases, reverse=False, drop=0, seed=99):
    """the cases as descriptor lists for svt_hip_recon_batch_device, laid out as block_case lays blocks out (stride 4 x odd, origins
    advancing by size + 4, guard bytes elsewhere); lists are grouped by size as the entry requires, the order inside a size is the cases'
    (reverse: backwards, without the first `drop` of them -- other blocks then share a workgroup, and others sit beside the idle slots of
    each size's last, partly filled workgroup of 256 / N blocks).  Returns the dict of block_case plus q, eob and `order` (index into
    `cases` of every list entry)."""
    rng = np.random.default_rng(seed)
    _, offs = T.iscan_array()
    order = []
    counts = []
    for ts in range(4):
        idx = [i for i, c in enumerate(cases) if c["tx_size"] == ts]
        if reverse:
            idx = idx[drop:][::-1]
        order += idx
        counts.append(len(idx))
    stride = 4 * 173
    x, y, row_h, place = 4, 3, 0, []
    for i in order:
        n = T.TX_N[cases[i]["tx_size"]]
        if x + n + 4 > stride:
            x, y, row_h = 4, y + row_h + 3, 0
        place.append((y, x))
        x, row_h = x + n + 4, max(row_h, n)
    height = y + row_h + 3
    pred_p = rng.integers(0, 256, (height, stride)).astype(np.uint8)
    blocks = np.zeros(len(order), dtype=B.TQ_BLOCK_DTYPE)
    q, eob, pos = [], [], 0
    for j, (i, (by, bx)) in enumerate(zip(order, place)):
        c = cases[i]
        n = T.TX_N[c["tx_size"]]
        pred_p[by:by + n, bx:bx + n] = c["pred"]
        o = by * stride + bx
        blocks[j] = (0, o, o, pos, offs[(c["tx_size"], c["tx_type"])], stride, stride, stride, c["tx_size"], c["tx_type"], c["qtab"], 1, 0, 0)
        q.append(c["qcoeff"]); eob.append(c["eob"])
        pos += n * n
    return dict(pred=pred_p, blocks=blocks, counts=np.array(counts, np.int32), qtabs=edge_qtabs(), n_coeff=pos, place=place, order=order,
                q=np.concatenate(q), eob=np.array(eob, np.uint16))


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole pictures: the decode pass's block walk on the CPU, and pictures whose coefficients come from the families above
# ---------------------------------------------------------------------------------------------------------------------------------------
KEY_FRAME = (64, 40, 10)        # width, height, grid seed: all four sizes, every ADST type at every size below 32 (tests/test_recon_edges.py)


def _zorder(x4, y4):
    v = 0
    for b in range(4):
        v |= ((x4 >> b) & 1) << (2 * b) | ((y4 >> b) & 1) << (2 * b + 1)
    return v


def coeff_offset(plane, x0, y0, W):
    """where the block at sample (x0, y0) of its plane starts in the position-addressed coefficient buffer (include/svtvp9_hip.h: SVT_SB_COEFFS)"""
    sh, mask = (5, 31) if plane else (6, 63)
    return ((y0 >> sh) * ((W + 63) // 64) + (x0 >> sh)) * B.SB_COEFFS + (0, 4096, 5120)[plane] + _zorder((x0 & mask) >> 2, (y0 & mask) >> 2) * 16


def eob_index(plane, x0, y0, W, H):
    import encdec_model as M
    return M.eob_map_offsets(W, H)[plane] + (y0 >> 2) * ((W // 2 if plane else W) // 4) + (x0 >> 2)


def intra_walk(mi, W, H):
    """(plane, x0, y0, n, mode, tx_type, have_right) of every transform block of an intra grid in DECODE order: superblocks in raster
    order, the 8x8 units of one in z-order, per leaf luma, Cb, Cr -- an 8x8 unit of 4x4 blocks is its four luma blocks, then Cb, Cr
    (oracle/oracle_intra.c: svt_oracle_intra_picture walks the same way); the transform type from the luma mode as the encode pass takes it"""
    import encdec_model as M
    out = []
    for sr in range((H + 63) // 64):
        for sc in range((W + 63) // 64):
            for z in range(64):
                r = sum(((z >> (2 * b + 1)) & 1) << b for b in range(3))
                c = sum(((z >> (2 * b)) & 1) << b for b in range(3))
                ur, uc = sr * 8 + r, sc * 8 + c
                if ur >= H // 8 or uc >= W // 8:
                    continue
                m = mi[ur, uc]
                st = int(m["sb_type"])
                n8 = {0: 1, 3: 1, 6: 2, 9: 4}[st]
                if ur % n8 or uc % n8:
                    continue
                if st == 0:
                    md = (int(m["pad"][1]) & 15, int(m["pad"][1]) >> 4, int(m["pad"][0]) & 15, int(m["pad"][0]) >> 4)
                    out += [(0, uc * 8 + 4 * (k & 1), ur * 8 + 4 * (k >> 1), 4, md[k], M.INTRA_TX_TYPE[md[k]], int(not k & 1)) for k in range(4)]
                else:
                    mode = int(m["pad"][1])
                    out.append((0, uc * 8, ur * 8, 8 * n8, mode, M.INTRA_TX_TYPE[mode] if n8 < 4 else 0, 0))
                out += [(p, uc * 4, ur * 4, 4 * n8, int(m["pad"][2]), 0, 0) for p in (1, 2)]
    return out


def decode_intra_picture(mi, W, H, q, emap, qtabs):
    """a key frame rebuilt on the CPU block by block in decode order: reference samples from the reconstruction so far
    (svt_oracle_intra_ref_samples2), prediction (svt_oracle_intra_predict), dequantise (this file's rule), oracle_inv_txfm_add; a block whose
    eob is 0 copies its prediction.  -> (prediction planes, reconstruction planes before deblocking, overflow count); tight planes"""
    ora = T.oracle()
    pred = [np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)]
    rec = [np.zeros_like(p) for p in pred]
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))                   # noqa: E731
    over = 0
    for plane, x0, y0, n, mode, tt, have_right in intra_walk(mi, W, H):
        above, left = np.zeros(65, np.uint8), np.zeros(32, np.uint8)
        ora.svt_oracle_intra_ref_samples2(u8(rec[plane]), rec[plane].shape[1], x0, y0, n, have_right, u8(above), u8(left))
        blk = np.zeros((n, n), np.uint8)
        ora.svt_oracle_intra_predict(mode, n, int(x0 > 0), int(y0 > 0), u8(above[1:]), u8(left), u8(blk), n)
        pred[plane][y0:y0 + n, x0:x0 + n] = blk
        e = int(emap[eob_index(plane, x0, y0, W, H)])
        if e:
            off = coeff_offset(plane, x0, y0, W)
            dq, o = dequantise_one(q[off:off + n * n], n, qtabs[1 if plane else 0]["dequant"])
            over += o
            blk = T.oracle_inv_add(dq, blk, {4: 0, 8: 1, 16: 2, 32: 3}[n], tt, e)
        rec[plane][y0:y0 + n, x0:x0 + n] = blk
    return pred, rec, over


INTER_W, INTER_H = 128, 64


def inter_grids(variant):
    """(mc_mi, lf_mi) of a 128x64 inter picture, zero motion vectors, whose leaves hold every transform size in luma and in chroma: one
    superblock is a 64x64 leaf with 32x32 transforms (chroma 32x32); the other holds a 32x32 leaf with 16x16 transforms (chroma 16x16),
    four 16x16 leaves with 8x8 transforms (chroma 8x8), sixteen 8x8 leaves with 4x4 and 8x8 transforms alternating (chroma 4x4) and a
    32x32 leaf with a 32x32 transform (chroma 16x16).  variant 1 swaps the superblocks.  Leaves take list 0, list 1 or both in turn."""
    mc = np.zeros((INTER_H // 8, INTER_W // 8), dtype=B.MC_MODE_INFO_DTYPE)
    lf = np.zeros((INTER_H // 8, INTER_W // 8), dtype=B.LF_MODE_INFO_DTYPE)
    turn = [0]

    def leaf(r, c, n8, tx):
        a, b = lf[r:r + n8, c:c + n8], mc[r:r + n8, c:c + n8]
        a["sb_type"], a["tx_size"], a["is_inter"], a["filter_level"] = {1: 3, 2: 6, 4: 9, 8: 12}[n8], tx, 1, 20
        b["bw8"], b["bh8"] = n8, n8
        b["ref_list"] = ((0, -1), (1, -1), (0, 1))[turn[0] % 3]
        turn[0] += 1
    big, mixed = (0, 8) if variant == 0 else (8, 0)
    leaf(0, big, 8, 3)
    leaf(0, mixed, 4, 2)
    for r, c in ((0, 4), (0, 6), (2, 4), (2, 6)):
        leaf(r, mixed + c, 2, 1)
    for k in range(16):
        leaf(4 + k // 4, mixed + k % 4, 1, (k + k // 4) & 1)
    leaf(4, mixed + 4, 4, 3)
    return mc, lf


def inter_block_table(lf_mi, W=INTER_W, H=INTER_H):
    """(plane, x0, y0, n, 0) of every transform block in the order of the lists the decode pass builds, from the product's host list builder
    (svt_hip_tq_blocks_from_grid: pinned against an independent enumeration by tests/test_encdec_host.py), and the position codes"""
    import encdec_model as M
    g = B.TqPicGeom()
    g.width, g.height = W, H
    blocks, pos, cnt = M.host_block_list([np.ascontiguousarray(lf_mi)], [g], lf_mi.shape[1])
    table = [(int(p >> 22) & 3, (int(p) & 0x7FF) * 4, ((int(p) >> 11) & 0x7FF) * 4, T.TX_N[int(b["tx_size"])], 0) for b, p in zip(blocks, pos)]
    return table, pos, cnt


def decode_inter_picture(pred, table, W, H, q, emap, qtabs):
    """prediction planes + oracle_inv_txfm_add per block in list order -> (reconstruction planes, overflow count)"""
    rec = [p.copy() for p in pred]
    over = 0
    for plane, x0, y0, n, tt in table:
        e = int(emap[eob_index(plane, x0, y0, W, H)])
        if e:
            off = coeff_offset(plane, x0, y0, W)
            dq, o = dequantise_one(q[off:off + n * n], n, qtabs[1 if plane else 0]["dequant"])
            over += o
            rec[plane][y0:y0 + n, x0:x0 + n] = T.oracle_inv_add(dq, rec[plane][y0:y0 + n, x0:x0 + n], {4: 0, 8: 1, 16: 2, 32: 3}[n], tt, e)
    return rec, over


def _steps_fit(target, n, steps, bound):
    """qcoeff whose dequantised value is `target` rounded towards zero onto the steps (32x32: onto step / 2); asserts that every product
    fits 16 bits and stays within `bound`: the block's amplitude stays inside the defined domain of its type"""
    step = np.full(n * n, int(steps[1]), np.int64)
    step[0] = int(steps[0])
    t = np.asarray(target, np.int64)
    qv = np.sign(t) * ((np.abs(t) * (2 if n == 32 else 1)) // step)
    dq, o = dequantise_one(qv.astype(np.int16), n, steps)
    assert o == 0 and np.abs(dq.astype(np.int64)).max(initial=0) <= bound
    return qv.astype(np.int16)


def crafted_coefficients(table, q_index, W, H, seed, wrap_dct=True):
    """qcoeff buffer and eob map of a picture whose transform blocks -- `table`: (plane, x0, y0, n, tx_type) in any order -- take their
    coefficients from coeff_edge_cases' families dense / sparse / peak / shortcuts, cycling through the cases of the block's (size, type).
    A case's dqcoeff is the target: qcoeff = target / step towards zero, so an ADST block's amplitude stays inside its type's defined
    domain at any q index; wrap_dct: every second DCT_DCT block takes the case's qcoeff as it is, so that at a coarse q index its products
    wrap.  Every seventh block keeps its coefficients and gets eob 0.  -> (q, emap, per-block records (eob, qcoeff block, case name))"""
    import encdec_model as M
    rng = np.random.default_rng(seed)
    qt = qindex_tables(q_index)
    by_group = {}
    for c in coeff_edge_cases():
        if c["family"] in ("dense", "sparse", "peak", "shortcuts"):
            by_group.setdefault((c["tx_size"], c["tx_type"]), []).append(c)
    q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
    emap = np.zeros(M.eob_map_offsets(W, H)[3], np.uint16)
    turn, recs = {}, []
    for k, (plane, x0, y0, n, tt) in enumerate(table):
        ts = {4: 0, 8: 1, 16: 2, 32: 3}[n]
        pool = by_group[(ts, tt)]
        i = turn.get((ts, tt), int(rng.integers(0, len(pool))))
        turn[(ts, tt)] = i + 1
        c = pool[i % len(pool)]
        steps = qt[1 if plane else 0]["dequant"]
        if tt == 0 and wrap_dct and turn[(ts, tt)] % 2 == 0:
            qv = c["qcoeff"].copy()
        else:
            qv = _steps_fit(case_dqcoeff(c)[0], n, steps, OUTSIDE_DOMAIN_ABOVE.get((ts, tt), 32768))
        e = c["eob"]
        if e < n * n:                                 # a shortcut block: the last of the first eob scan positions must stay non-zero
            scan = np.argsort(T.scan_tables()[f"iscan_{ts}_0"])
            if qv[scan[e - 1]] == 0:
                qv[scan[e - 1]] = 1
        if k % 7 == 6:
            e = 0
        off = coeff_offset(plane, x0, y0, W)
        q[off:off + n * n] = qv
        emap[eob_index(plane, x0, y0, W, H)] = e
        recs.append((e, qv, c["name"]))
    return q, emap, recs

"""Inputs of the forward transform stage's edge tests (tests/test_tq_edges.py, tests/test_gpu_tq_edges.py, tests/gen_golden_tq_edges.py):
a deterministic list of named transform blocks, built on the CPU, that drive the residual -> forward DCT / ADST -> quantiser -> distortion
-> rate arithmetic of tq_block_body (csrc/tq_core.h) and tq_lane_block (csrc/tq_kernel.hip) to the ends of its ranges.  The residual of a
case is always source minus prediction of real bytes (+r: source r, prediction 0; -r: source 0, prediction r).

Families (case["family"]):
  basis      +-255 * sign(column basis k_r (x) row basis k_c), DCT or ADST per axis as the transform type says; 4x4 and 8x8 every
             (k_r, k_c), 16x16 and 32x32 k in {0, 1, 2, 3, N/2-1, N/2, N-2, N-1} per axis; the tables of q index 0, q index 255 and the
             steps MID_STEPS in turn.  The flat block (0, 0) of DCT_DCT gives the largest coefficient a size can have: 8160, 16319,
             32639, 32639.
  ladder     the flat block (both signs) and, per (size, type), the basis pattern with the largest coefficient, at the amplitudes LADDER
  first      4x4: the `++v[0]` rule of the forward 4x4 transforms (first residual sample non-zero) -- the sample, its right neighbour and
             two samples of column 0 below it set to 0, +-1, +-255 over a rest of 0, +-3, +-255
  zbin       a DC and an AC coefficient of a basis block and of a natural (gen_clip-like) block, with `zbin` overwritten so that the
             coefficient lies one below, on and one above the quantiser's dead-zone boundary; 32x32: the boundary is (zbin + 1) >> 1, with
             odd and even zbin on either side
  clamp      flat +-255 16x16 / 32x32 blocks at tables where |coefficient| + round passes 32767, so that clamp16 in the quantiser acts
  partial32  every 32x32 case above once more with partial32 = 1

Where clamp16 decides the level (searched here by clamp_windows(), nothing on a GPU; DC of a flat 255 block = 32639):
  16x16, tables quant_table(s, 1828), s = 4 .. 1336: the sum passes 32767 from s = 344 (round 129); the clamped and the unclamped level
      differ at 198 of those 993 steps, between 395 and 1325, among them 684 (47 / 48) and 700 (46 / 47), the two the clamp cases use.
  32x32 (round halved): the sum passes 32767 from s = 686; the levels differ at 67 of those 651 steps, between 771 and 1315; the cases
      use the first two, 771 and 790.  700 and 1336 are reached but equivalent (93 and 49 both ways) and are kept as such.
  real q indices (luma tables of svt_hip_quant_tables_for_qindex): 16x16 is reached from index 191 and differs at 11 indices (201, 214,
      215, 217, 218, 234, 235, 242, 249, 250, 251); 32x32 is reached from 235 and differs at 249 alone.  The list uses REAL_Q_INDEX = 249,
      where both do (tests/test_tq_edges.py pins these lists).
  4x4 and 8x8: the largest coefficients are 8160 and 16319 and a table's round is at most 48 * 32767 >> 7 = 12287, so the sum stays below
      32767 for every table eb_vp9_init_quantizer can produce: the clamp of those instances is unreachable from real tables.

Nothing here needs a GPU."""
import ctypes as C
import functools

import numpy as np

import svt_testlib as T

B = T.B
GROUPS = [(ts, tt) for ts in range(4) for tt in (range(4) if ts < 3 else (0,))]
TYPE_NAMES = ("DCT_DCT", "ADST_DCT", "DCT_ADST", "ADST_ADST")
LADDER = (255, 254, 129, 128, 64, 1)
MID_STEPS = (40, 48)
CLAMP_STEPS_16 = (684, 700)
EQUIVALENT_STEPS_32 = (700, 1336)       # a + round > 32767, the clamp acts, the level is the same without it
REAL_Q_INDEX = 249
PEAK = {0: 8160, 1: 16319, 2: 32639, 3: 32639}          # largest |coefficient| per size (flat +-255, DCT_DCT)
MAX_LEVEL = 16450                       # cat6_high_cost has 64 entries: (|level| - 67) >> 8 <= 63
MAX_BLOCKS = 2500


def qindex_tables(q_index):
    """[luma, chroma] tables of a q index (svt_hip_quant_tables_for_qindex: pinned against eb_vp9_init_quantizer by tests/test_tq_params.py)"""
    qt = np.zeros(2, dtype=B.QUANT_DTYPE)
    assert B.load().svt_hip_quant_tables_for_qindex(q_index, qt.ctypes.data_as(C.c_void_p)) == 0
    return qt


def with_zbin(step_dc, step_ac, zbin_dc=None, zbin_ac=None):
    q = T.quant_table(step_dc, step_ac).copy()
    if zbin_dc is not None:
        q["zbin"][0] = zbin_dc
    if zbin_ac is not None:
        q["zbin"][1] = zbin_ac
    return q


# ---------------------------------------------------------------------------------------------------------------------------------------
# the quantiser's level in numpy, with and without the clamp (VPX/quantize.c:112-157, :206-254)
# ---------------------------------------------------------------------------------------------------------------------------------------
def level_of(a, q, ac, is32, clamp=True):
    """|level| of |coefficient| a (at or beyond the dead zone) under table q"""
    tmp = int(a) + ((int(q["round"][ac]) + 1) >> 1 if is32 else int(q["round"][ac]))
    if clamp:
        tmp = max(-32768, min(32767, tmp))
    return ((((tmp * int(q["quant"][ac])) >> 16) + tmp) * int(q["quant_shift"][ac])) >> (15 if is32 else 16)


def clamp_windows():
    """where clamp16 decides the level of a flat 255 block's DC (32639): {(size, 'steps' | 'qindex'): (reached, differing)} -- lists of the
    DC steps s of quant_table(s, 1828), s = 4 .. 1336, or of the real q indices"""
    out = {}
    for ts in (2, 3):
        for kind, keys in (("steps", range(4, 1337)), ("qindex", range(256))):
            reached, differ = [], []
            for k in keys:
                q = T.quant_table(k, 1828) if kind == "steps" else qindex_tables(k)[0]
                rnd = (int(q["round"][0]) + 1) >> 1 if ts == 3 else int(q["round"][0])
                if PEAK[ts] + rnd > 32767:
                    reached.append(k)
                    if level_of(PEAK[ts], q, 0, ts == 3) != level_of(PEAK[ts], q, 0, ts == 3, clamp=False):
                        differ.append(k)
            out[(ts, kind)] = (reached, differ)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# residual patterns
# ---------------------------------------------------------------------------------------------------------------------------------------
def basis_matrix(n, adst):
    """m[frequency k][sample j] of the N-point DCT, or of VP9's ADST (4-point: sin(pi (j+1)(2k+1) / 9); 8 / 16: sin(pi (2j+1)(2k+1) / 4N))"""
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    if not adst:
        return np.cos(np.pi * (2 * j + 1) * k / (2 * n))
    if n == 4:
        return np.sin(np.pi * (j + 1) * (2 * k + 1) / 9)
    return np.sin(np.pi * (2 * j + 1) * (2 * k + 1) / (4 * n))


def basis_sign(ts, tt, kr, kc):
    """sign pattern [row][column] of the 2-D basis function (vertical frequency kr, horizontal kc); a zero of the basis counts as +"""
    n = T.TX_N[ts]
    col, row = basis_matrix(n, tt in (1, 3)), basis_matrix(n, tt in (2, 3))       # ADST_DCT: ADST down the columns
    v = col[kr][:, None] * row[kc][None, :]
    return np.where(v > -1e-9, 1, -1).astype(np.int16)


def basis_ks(n):
    return list(range(n)) if n <= 8 else [0, 1, 2, 3, n // 2 - 1, n // 2, n - 2, n - 1]


def planes_of(res):
    """residual in [-255, 255] -> (source, prediction) bytes"""
    res = np.asarray(res, np.int16)
    assert np.abs(res).max() <= 255
    return np.clip(res, 0, 255).astype(np.uint8), np.clip(-res, 0, 255).astype(np.uint8)


def residual_of(c):
    return c["src"].astype(np.int16) - c["pred"].astype(np.int16)


def coefficients(c):
    return T.oracle_fwd_txfm(residual_of(c), c["tx_size"], c["tx_type"], bool(c["partial32"]))


def _case(name, family, ts, tt, res, qt, hits, partial32=0, **extra):
    src, pred = planes_of(res)
    return dict(name=name, family=family, tx_size=ts, tx_type=tt, src=src, pred=pred, qt=np.array(qt, dtype=B.QUANT_DTYPE), partial32=partial32, hits=hits, **extra)


def _natural_block(ts, seed):
    """a block of gen_clip material against a shifted, noisy prediction (what make_tq_case codes) whose DC and largest AC are both >= 8"""
    n = T.TX_N[ts]
    rng = np.random.default_rng(seed)
    src = T.gen_clip(128, 64, 1, seed)[0]
    pred = np.clip(np.roll(src, (1, 2), (0, 1)).astype(np.int16) + rng.integers(-12, 13, src.shape), 0, 255).astype(np.uint8)
    for y in range(0, 64, n):
        for x in range(0, 128, n):
            res = src[y:y + n, x:x + n].astype(np.int16) - pred[y:y + n, x:x + n]
            yield res


def _step_for(a):
    return int(max(4, min(1336, a // 2)))


def _zbin_cases(ts, tt):
    """the zero-bin family of one (size, type)"""
    n, is32, out = T.TX_N[ts], ts == 3, []
    nat = None
    for res in _natural_block(ts, 40 + ts):
        co = T.oracle_fwd_txfm(res, ts, tt)
        if abs(int(co[0])) >= 8 and np.abs(co[1:]).max() >= 8:
            nat = res
            break
    assert nat is not None
    contents = (("basis", np.full((n, n), 64, np.int16), (64 if is32 else 255) * basis_sign(ts, tt, 1, 2)), ("natural", nat, nat))
    # (boundary side, zbin as a function of |c|); 32x32: the boundary is (zbin + 1) >> 1, odd and even zbin on each side
    sides = ((("below", lambda a: a + 1), ("at", lambda a: a), ("above", lambda a: a - 1)) if not is32 else
             (("below", lambda a: 2 * a + 1), ("below", lambda a: 2 * a + 2), ("at", lambda a: 2 * a), ("at", lambda a: 2 * a - 1),
              ("above", lambda a: 2 * a - 2), ("above", lambda a: 2 * a - 3)))
    for cname, res_dc, res_ac in contents:
        c_dc = T.oracle_fwd_txfm(res_dc, ts, tt)
        c_ac = T.oracle_fwd_txfm(res_ac, ts, tt)
        a_dc, i_ac = abs(int(c_dc[0])), 1 + int(np.argmax(np.abs(c_ac[1:])))
        a_ac = abs(int(c_ac[i_ac]))
        assert a_dc >= 8 and a_ac >= 8
        for side, f in sides:
            z_dc, z_ac = f(a_dc), f(a_ac)
            assert 0 < z_dc <= 32767 and 0 < z_ac <= 32767
            qt = with_zbin(_step_for(a_dc), _step_for(a_ac), z_dc, z_ac)       # one table serves the DC and the AC case of a side
            tag = f"{side}{'-odd' if is32 and z_dc & 1 else '-even' if is32 else ''}"
            out.append(_case(f"zbin/{n}x{n}/{TYPE_NAMES[tt]}/{cname}/dc/{tag}", "zbin", ts, tt, res_dc, qt, "dead-zone boundary, DC", target=0, side=side))
            out.append(_case(f"zbin/{n}x{n}/{TYPE_NAMES[tt]}/{cname}/ac/{tag}", "zbin", ts, tt, res_ac, qt, "dead-zone boundary, AC", target=i_ac, side=side))
    return out


@functools.lru_cache(maxsize=None)
def _cases():
    q0, q255, mid = qindex_tables(0)[0], qindex_tables(255)[0], T.quant_table(*MID_STEPS)
    turn = (q0, q255, mid)
    cases = []
    # ---- basis ----
    k = 0
    best = {}
    for ts, tt in GROUPS:
        n = T.TX_N[ts]
        top = (-1, None)
        for kr in basis_ks(n):
            for kc in basis_ks(n):
                sg = basis_sign(ts, tt, kr, kc)
                peak = int(np.abs(T.oracle_fwd_txfm(255 * sg, ts, tt)).max())
                if peak > top[0]:
                    top = (peak, (kr, kc))
                for s in (1, -1):
                    cases.append(_case(f"basis/{n}x{n}/{TYPE_NAMES[tt]}/{kr},{kc}/{'+' if s > 0 else '-'}", "basis", ts, tt, s * 255 * sg, turn[k % 3],
                                       "coefficient ceilings, int16 casts between the passes"))
                    k += 1
        best[(ts, tt)] = top[1]
    # ---- ladder ----
    for ts, tt in GROUPS:
        n = T.TX_N[ts]
        flat, pat = np.ones((n, n), np.int16), basis_sign(ts, tt, *best[(ts, tt)])
        shapes = [("flat", flat, (1, -1))] + ([("peak", pat, (1,))] if not np.array_equal(pat, flat) else [])
        for sname, sg, signs in shapes:
            for j, a in enumerate(LADDER):
                for s in signs:
                    cases.append(_case(f"ladder/{n}x{n}/{TYPE_NAMES[tt]}/{sname}/{'+' if s > 0 else '-'}{a}", "ladder", ts, tt, s * a * sg, turn[(j + (s < 0)) % 3],
                                       "amplitude ladder up to the ceiling"))
    # ---- first sample (4x4) ----
    for tt in range(4):
        for pos in ((0, 0), (0, 1), (1, 0), (3, 0)):
            for val in (0, 1, -1, 255, -255):
                for j, rest in enumerate((3, -3, 0, 255, -255)):
                    res = np.full((4, 4), rest, np.int16)
                    if pos != (0, 0):
                        res[0, 0] = 0          # (the rule must then stay off, whatever the neighbour holds)
                    res[pos] = val
                    cases.append(_case(f"first/{TYPE_NAMES[tt]}/r{pos[0]}c{pos[1]}={val}/rest{rest}", "first", 0, tt, res, (q0, mid)[j & 1],
                                       "the 4x4 forward transforms' ++v[0] rule"))
    # ---- zero-bin ----
    for ts, tt in GROUPS:
        cases += _zbin_cases(ts, tt)
    # ---- clamp ----
    win = clamp_windows()
    steps32 = tuple(win[(3, "steps")][1][:2])
    assert REAL_Q_INDEX in win[(2, "qindex")][1] and REAL_Q_INDEX in win[(3, "qindex")][1]
    for ts, steps in ((2, CLAMP_STEPS_16), (3, steps32 + EQUIVALENT_STEPS_32)):
        n = T.TX_N[ts]
        tabs = [(f"step{s}", T.quant_table(s, 1828)) for s in steps] + [(f"q{REAL_Q_INDEX}", qindex_tables(REAL_Q_INDEX)[0])]
        for tname, qt in tabs:
            for s in (1, -1):
                cases.append(_case(f"clamp/{n}x{n}/{tname}/{'+' if s > 0 else '-'}255", "clamp", ts, 0, np.full((n, n), s * 255, np.int16), qt,
                                   "clamp16(a + round) in the quantiser", equivalent=ts == 3 and tname in [f"step{e}" for e in EQUIVALENT_STEPS_32]))
    # ---- partial32 ----
    for c in [c for c in cases if c["tx_size"] == 3]:
        cases.append(dict(c, name="partial32/" + c["name"], partial32=1, hits=c["hits"] + "; partial32"))
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def edge_cases():
    """the list (shared, read-only)"""
    return list(_cases())


@functools.lru_cache(maxsize=None)
def _outputs():
    iscan, offs = T.iscan_array()
    out = []
    for c in _cases():
        co = coefficients(c)
        q, dq, eob = T.oracle_quantize(co, c["tx_size"], c["tx_type"], c["qt"])
        out.append((co, q, dq, eob))
    return tuple(out)


def oracle_outputs():
    """per case (coefficients, qcoeff, dqcoeff, eob) of the oracle's forward transform and quantiser"""
    return list(_outputs())


def check_conditions(cases=None, outs=None):
    """the conditions the list is built to meet; returns a few figures for the tests to print"""
    cases = edge_cases() if cases is None else cases
    outs = oracle_outputs() if outs is None else outs
    assert len(cases) < MAX_BLOCKS, len(cases)
    for fam in ("basis", "ladder", "zbin"):
        assert {(c["tx_size"], c["tx_type"]) for c in cases if c["family"] == fam and not c["partial32"]} == set(GROUPS), fam
    peak = {ts: max(int(np.abs(o[0]).max()) for c, o in zip(cases, outs) if c["tx_size"] == ts) for ts in range(4)}
    assert peak == PEAK, peak
    energy = max(int((o[0].astype(np.int64) ** 2).sum()) for o in outs)
    assert energy >= 10 ** 9, energy
    top_level = max(int(np.abs(o[1].astype(np.int32)).max()) for o in outs)
    assert 8000 <= top_level <= MAX_LEVEL, top_level
    # both sides of every zero-bin boundary, and what the oracle does there
    seen = set()
    for c, o in zip(cases, outs):
        if c["family"] != "zbin":
            continue
        lvl = int(o[1][c["target"]])
        assert (lvl == 0) == (c["side"] == "below"), (c["name"], lvl)
        seen.add((c["tx_size"], c["tx_type"], c["partial32"], c["target"] == 0, c["side"]))
    for ts, tt in GROUPS:
        for dc in (True, False):
            for side in ("below", "at", "above"):
                assert (ts, tt, 0, dc, side) in seen, (ts, tt, dc, side)
    # the clamp cases: the clamped and the unclamped level differ (or, for the two 32x32 steps kept as such, are reached and agree)
    n_clamp = 0
    for c, o in zip(cases, outs):
        if c["family"] != "clamp":
            continue
        is32 = c["tx_size"] == 3
        a = abs(int(o[0][0]))
        assert a == PEAK[c["tx_size"]] and a + ((int(c["qt"]["round"][0]) + 1) >> 1 if is32 else int(c["qt"]["round"][0])) > 32767, c["name"]
        with_c, without = level_of(a, c["qt"], 0, is32), level_of(a, c["qt"], 0, is32, clamp=False)
        assert abs(int(o[1][0])) == with_c, c["name"]
        assert (with_c == without) == bool(c["equivalent"]), (c["name"], with_c, without)
        n_clamp += with_c != without
    assert n_clamp >= 8
    n4 = sum(1 for c in cases if c["tx_size"] == 0)
    assert n4 > 256, n4              # more than one workgroup (four waves) of the one-block-per-lane form
    return dict(blocks=len(cases), peak=peak, energy=energy, top_level=top_level, clamp_cases=n_clamp, blocks_4x4=n4)


# ---------------------------------------------------------------------------------------------------------------------------------------
# descriptor lists over the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
GUARD = 0xA5


def _tables(cases, idx):
    """deduplicated quant tables of the chosen cases -> (array, index per chosen case)"""
    keys, tabs, which = {}, [], []
    for i in idx:
        kb = cases[i]["qt"].tobytes()
        if kb not in keys:
            keys[kb] = len(tabs)
            tabs.append(cases[i]["qt"])
        which.append(keys[kb])
    assert len(tabs) <= 256, len(tabs)          # svt_tq_block.qtab is a byte
    return np.array(tabs, dtype=B.QUANT_DTYPE), which


def _finish(cases, idx, place, sizes, do_recon, rate_seed):
    """place[j] = (src_off, pred_off, recon_off, src_stride, pred_stride, recon_stride) of chosen case idx[j] (idx sorted by size);
    sizes = bytes of the (source, prediction, reconstruction) buffers"""
    iscan, offs = T.iscan_array()
    qtabs, which = _tables(cases, idx)
    src, pred = np.full(sizes[0], 0x11, np.uint8), np.full(sizes[1], 0xEE, np.uint8)
    own = np.zeros(sizes[2], bool)
    blocks = np.zeros(len(idx), dtype=B.TQ_BLOCK_DTYPE)
    pos = 0
    for j, (i, p) in enumerate(zip(idx, place)):
        c = cases[i]
        n = T.TX_N[c["tx_size"]]
        so, po, ro, ss, ps, rs = p
        assert so % 4 == 0 and po % 4 == 0 and ro % 4 == 0 and ss % 4 == 0 and ps % 4 == 0 and rs % 4 == 0 and max(ss, ps, rs) <= 65532
        for r in range(n):
            assert so + r * ss + n <= sizes[0] and po + r * ps + n <= sizes[1] and ro + r * rs + n <= sizes[2]
            src[so + r * ss:so + r * ss + n] = c["src"][r]
            pred[po + r * ps:po + r * ps + n] = c["pred"][r]
            assert not own[ro + r * rs:ro + r * rs + n].any(), c["name"]
            own[ro + r * rs:ro + r * rs + n] = True
        blocks[j] = (so, po, ro, pos, offs[(c["tx_size"], c["tx_type"])], ss, ps, rs, c["tx_size"], c["tx_type"], which[j], int(do_recon), c["partial32"], 0)
        pos += n * n
    counts = np.array([sum(1 for i in idx if cases[i]["tx_size"] == s) for s in range(4)], np.int32)
    case = dict(src=src, pred=pred, recon_bytes=sizes[2], own=own, blocks=blocks, counts=counts, qtabs=qtabs, iscan=iscan, n_coeff=pos, idx=list(idx))
    case["rate_blocks"] = T.add_rate_info(case, rate_seed)
    return case


def packed_layout(cases, do_recon=True, width=1024):
    """every case in one plane triple of the same geometry (stride `width`), each block at its own position, grouped by size"""
    idx = sorted(range(len(cases)), key=lambda i: cases[i]["tx_size"])
    place, x, y, cur = [], 0, 0, None
    for i in idx:
        n = T.TX_N[cases[i]["tx_size"]]
        if cur != n or x + n > width:
            y, x = (y + cur if cur else 0), 0
            cur = n
        o = y * width + x
        place.append((o, o, o, width, width, width))
        x += n
    size = (y + cur) * width
    return _finish(cases, idx, place, (size, size, size), do_recon, rate_seed=17)


BIG_STRIDES = ((65532, 65528, 65524), (65524, 65532, 65528), (65528, 65524, 65532), (65532, 65524, 65528))       # per size: source, prediction, reconstruction
SMALL_STRIDES = (160, 164, 168, 172)
BAND = 32 * 256          # bytes a block of the unlike layout owns in each of the three buffers
# offsets (mod 16) of the three pointers, in turn: each of the three on a 16-byte boundary while another is not, 8-byte ones likewise
UNLIKE_OFFSETS = ((0, 4, 8), (4, 0, 12), (8, 12, 0), (0, 0, 4), (12, 0, 0), (0, 8, 0), (8, 0, 4), (4, 8, 8), (8, 4, 0))


def unlike_subset(cases):
    """every (size, type) with its peak basis block, its flat 255 ladder block and a zero-bin block on the boundary; the clamp cases that
    decide; a first-sample block per type; a partial32 block"""
    pick = []
    for ts, tt in GROUPS:
        grp = [i for i, c in enumerate(cases) if (c["tx_size"], c["tx_type"]) == (ts, tt) and not c["partial32"]]
        pick.append(next(i for i in grp if cases[i]["family"] == "ladder" and "/flat/+255" in cases[i]["name"]))
        pick.append(next(i for i in grp if cases[i]["family"] == "ladder" and "/flat/-255" in cases[i]["name"]))
        pick.append(next(i for i in grp if cases[i]["family"] == "basis" and cases[i]["name"].endswith("/1,2/+")))
        pick.append(next(i for i in grp if cases[i]["family"] == "zbin" and cases[i]["side"] == "at" and cases[i]["target"] != 0))
        if ts == 0:
            pick.append(next(i for i in grp if cases[i]["family"] == "first" and "r0c0=1/rest-3" in cases[i]["name"]))
    pick += [i for i, c in enumerate(cases) if c["family"] == "clamp" and not c["equivalent"] and not c["partial32"]]
    pick.append(next(i for i, c in enumerate(cases) if c["partial32"] and c["family"] == "ladder" and "/flat/+255" in c["name"]))
    assert len(set(pick)) == len(pick)
    return sorted(pick, key=lambda i: cases[i]["tx_size"])


def unlike_layout(cases, recon_sets=1):
    """unlike_subset in three separate buffers: per block its own offsets and three pairwise different strides with the residues 0, 4, 8
    and 12 mod 16 in turn; the first block of each size with strides near 65532 (BIG_STRIDES).  recon_sets = 2: the blocks reconstruct in
    turn into two buffers (SVT_TQ_RECON_SET in pad[0]); those of the second use another stride.  Returns the case; case['set'][j] = the
    buffer of block j."""
    idx = unlike_subset(cases)
    big_rows = 32 * 65532 + 4096
    place, seen, k = [], set(), 0
    for j, i in enumerate(idx):
        ts = cases[i]["tx_size"]
        n = T.TX_N[ts]
        if ts not in seen:
            seen.add(ts)
            x = 256 * ts
            place.append((x + 0, x + 4 * (ts & 1), x + 8 * (ts >> 1), *BIG_STRIDES[ts]))
            continue
        base = big_rows + k * BAND
        ox = UNLIKE_OFFSETS[k % len(UNLIKE_OFFSETS)]
        st = [SMALL_STRIDES[(k + d) % 4] for d in range(3)]
        if recon_sets == 2 and j & 1:
            st[2] += 32
        assert len(set(st)) == 3 and max(ox) + n <= min(st) and (n - 1) * max(st) + max(ox) + n <= BAND
        place.append((base + ox[0], base + ox[1], base + ox[2], *st))
        k += 1
    size = big_rows + k * BAND
    case = _finish(cases, idx, place, (size, size, size), True, rate_seed=23)
    case["set"] = np.array([(j & 1) if recon_sets == 2 else 0 for j in range(len(idx))])
    if recon_sets == 2:
        case["blocks"]["pad"][:, 0] |= (case["set"] << 4).astype(np.uint8)
    return case


def alignment_census(case, base=(0, 0, 0)):
    """{size: set of (pointer on the vector path, another on the dword path)} over the rows of the case's blocks; the vector path of a row
    needs 8-byte (8x8) / 16-byte (16x16, 32x32) alignment -- 4x4 rows are always dwords and only need their offsets to differ"""
    out = {ts: set() for ts in range(4)}
    for b in case["blocks"]:
        ts = int(b["tx_size"])
        n = T.TX_N[ts]
        am = 16 if n >= 16 else 8
        for r in range(n):
            a = [(base[k] + int(b[f + "_off"]) + r * int(b[f + "_stride"])) % am == 0 for k, f in enumerate(("src", "pred", "recon"))]
            for k in range(3):
                if a[k] and not all(a):
                    out[ts].add(k)
    return out


def oracle_batch(case):
    """the oracle on a layout: (recon buffer(s) started as GUARD, qcoeff, dqcoeff, eob, dist, bits)"""
    recon = np.full(case["recon_bytes"], GUARD, np.uint8)
    q, dq = np.zeros(case["n_coeff"], np.int16), np.zeros(case["n_coeff"], np.int16)
    eob, dist = np.zeros(len(case["blocks"]), np.uint16), np.zeros((len(case["blocks"]), 2), np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    blocks = case["blocks"].copy()
    assert T.oracle().svt_oracle_tq_batch_dist(vp(case["src"]), vp(case["pred"]), vp(recon), vp(blocks), len(blocks), vp(case["qtabs"]), vp(case["iscan"]), vp(q), vp(dq),
                                               vp(eob), vp(dist)) == 0
    rb = case["rate_blocks"].copy()
    rb["eob"] = eob
    return recon, q, dq, eob, dist, T.oracle_rate_batch(dict(qcoeff=q, blocks=rb))

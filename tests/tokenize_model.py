"""numpy model of the coefficient tokeniser (csrc/tokenize_core.h), written independently of the C text: scan tables from the inverse
scans and the neighbour rule, tokens of one block, the transform blocks / entropy contexts / offsets / counts of a picture, and the
cost identity that ties a token stream to the reference's coeff_rate_estimate."""
import ctypes as C

import numpy as np

import svt_testlib as T

B = T.B

EOB_TOKEN = 11
ENERGY = (0, 1, 2, 3, 3, 4, 4, 5, 5, 5, 5, 5)
BAND4 = (0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 5)
CAT_BASE = (0, 1, 2, 3, 4, 5, 7, 11, 19, 35, 67)
INTRA_TX_TYPE = (0, 1, 2, 0, 3, 1, 2, 2, 1, 3)
NO_OFFSET = 0xFFFFFFFF
N_COUNTS = 4 * 2 * 2 * 6 * 6 * 12
_W4 = (1, 1, 2, 2, 2, 4, 4, 4, 8, 8, 8, 16, 16)
_H4 = (1, 2, 1, 2, 4, 2, 4, 8, 4, 8, 16, 8, 16)


def band_of(c, ts):
    if ts == 0:
        return BAND4[c]
    return 0 if c == 0 else 1 if c < 3 else 2 if c < 6 else 3 if c < 10 else 4 if c < 21 else 5


def token_of(v):
    a = abs(int(v))
    for tok in range(10, -1, -1):
        if a >= CAT_BASE[tok]:
            return tok
    raise AssertionError


def extra_of(v, tok):
    if tok == 0 or tok == EOB_TOKEN:
        return 0
    return (((abs(int(v)) - CAT_BASE[tok]) << 1) | (1 if v < 0 else 0)) & 0xFFFF


def neighbors_of(ts, tt, p):
    l = 4 << ts
    i, j = divmod(p, l)
    if ts < 3 and tt == 1 and i > 0 and j > 0:
        return p - 1, p - 1
    if ts < 3 and tt == 2 and i > 0 and j > 0:
        return p - l, p - l
    if i > 0 and j > 0:
        return p - l, p - 1
    if i > 0:
        return p - l, p - l
    return p - 1, p - 1


_scan_cache = None


def scan_tables():
    """({(ts, tt): offset}, int16 array) in the canonical layout of svt_rate_block.scan_off: {scan[n], neighbors[2 (n + 1)]} per table"""
    global _scan_cache
    if _scan_cache is None:
        offs, total = T.rate_scan_offsets()
        out = np.zeros(total, np.int16)
        entries = C.c_int32()
        poff = C.POINTER(C.c_uint32)()
        p = B.load().svt_hip_vp9_iscan_tables(C.byref(poff), C.byref(entries))
        for ts in range(4):
            n = 16 << (2 * ts)
            for tt in range(4):
                io = poff[ts * 4 + tt]
                iscan = np.array([p[io + k] for k in range(n)], np.int64)
                scan = np.zeros(n, np.int64)
                scan[iscan] = np.arange(n)
                o = offs[(ts, tt)]
                out[o:o + n] = scan
                for c in range(1, n):
                    out[o + n + 2 * c], out[o + n + 2 * c + 1] = neighbors_of(ts, tt, int(scan[c]))
        _scan_cache = (offs, out)
    return _scan_cache


def record(ts, ptype, inter, band, ctx, tok, extra):
    row = (((ts * 2 + ptype) * 2 + inter) * 6 + band) * 6 + ctx
    return (extra << 16) | (row << 4) | tok


def tokenize_block(q, ts, tt, eob, ptype, inter, ctx0):
    """q: the block's n coefficients in raster order.  Returns the uint32 records, eob + (eob < n) of them."""
    offs, tab = scan_tables()
    n = 16 << (2 * ts)
    scan = tab[offs[(ts, tt)]:offs[(ts, tt)] + n]
    energy = np.zeros(n, np.int64)
    out = []
    for c in range(min(eob + 1, n)):
        p = int(scan[c])
        ctx = ctx0
        if c:
            a, b = neighbors_of(ts, tt, p)
            ctx = (1 + energy[a] + energy[b]) >> 1
        if c == eob:
            tok, extra = EOB_TOKEN, 0
        else:
            tok = token_of(q[p])
            extra = extra_of(q[p], tok)
            energy[p] = ENERGY[tok]
        out.append(record(ts, ptype, inter, band_of(c, ts), int(ctx), tok, extra))
    return np.array(out, np.uint32)


def unpack(rec):
    rec = np.asarray(rec, np.uint32)
    return (rec & 15).astype(np.int64), ((rec >> 4) & 0xFFF).astype(np.int64), (rec >> 16).astype(np.int64)


def counts_of(records):
    tok, row, _ = unpack(records)
    return np.bincount(row * 12 + tok, minlength=N_COUNTS).astype(np.uint32)


def cost_of(records, tables):
    """bits of a block's token stream by the reference's tables: token_costs[ts][ptype][inter][band][prev was ZERO][ctx][token] + the cost
    of the value (value_cost / cat6 costs) -- equals coeff_rate_estimate for the block the stream was made from"""
    tok, row, extra = unpack(records)
    tc = tables["token_costs"].reshape(-1, 6, 2, 6, 12)
    total, prev_zero = 0, 0
    for t, r, e in zip(tok, row, extra):
        slice_, band, ctx = r // 36, (r // 6) % 6, r % 6
        total += int(tc[slice_, band, prev_zero, ctx, t])
        if t == 10:
            x = int(e) >> 1
            total += int(tables["cat6_low_cost"][x & 0xFF]) + int(tables["cat6_high_cost"][x >> 8])
        elif t != EOB_TOKEN:
            v = CAT_BASE[t] + (int(e) >> 1)
            total += int(tables["value_cost"][(-v if e & 1 else v) + 66])
        prev_zero = 1 if t == 0 else 0
    return total


def tokenize_blocks(case):
    """block form: (tokens, tok_off[n + 1], counts) of a rate case (qcoeff, svt_rate_block records, tx_type)"""
    toks, off = [], [0]
    for b, tt in zip(case["blocks"], case["tx_type"]):
        ts = int(b["tx_size"])
        n = 16 << (2 * ts)
        o = int(b["coeff_off"])
        toks.append(tokenize_block(case["qcoeff"][o:o + n], ts, int(tt), int(b["eob"]), int(b["plane_type"]), int(b["is_inter"]), int(b["ctx"])))
        off.append(off[-1] + len(toks[-1]))
    t = np.concatenate(toks) if toks else np.zeros(0, np.uint32)
    return t, np.array(off, np.uint32), counts_of(t)


def _uv_tx(bs, tx):
    m = min(max(_W4[bs] // 2, 1), max(_H4[bs] // 2, 1))
    return min(tx, 3 if m >= 8 else 2 if m >= 4 else 1 if m >= 2 else 0)


def _zorder(x, y):
    v = 0
    for b in range(4):
        v |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
    return v


def picture_blocks(lf_mi, eob_map, W, H):
    """the transform blocks of the coded (non-skipped) blocks of a picture in token order: dicts with plane, x4, y4 (4x4 units of the plane),
    ts, tt, inter, eob, ctx, sb, coeff_off"""
    mi_rows, mi_cols = H // 8, W // 8
    w4, h4 = W // 4, H // 4
    eoff = (0, w4 * h4, w4 * h4 + (w4 // 2) * (h4 // 2))
    maps = [eob_map[eoff[0]:eoff[1]].reshape(h4, w4), eob_map[eoff[1]:eoff[2]].reshape(h4 // 2, w4 // 2),
            eob_map[eoff[2]:eoff[2] + (w4 // 2) * (h4 // 2)].reshape(h4 // 2, w4 // 2)]

    def rec_at(plane, x4, y4):
        return lf_mi[y4 if plane else y4 >> 1, x4 if plane else x4 >> 1]

    def ts_at(plane, x4, y4):
        r = rec_at(plane, x4, y4)
        return _uv_tx(int(r["sb_type"]), int(r["tx_size"])) if plane else int(r["tx_size"])

    def nz_at(plane, x4, y4):
        s = 1 << ts_at(plane, x4, y4)
        return int(maps[plane][y4 - y4 % s, x4 - x4 % s] > 0)

    sb_cols, sb_rows = (W + 63) // 64, (H + 63) // 64
    out = []
    for sb in range(sb_rows * sb_cols):
        sr, sc = divmod(sb, sb_cols)
        for plane in range(3):
            u = 16 if plane == 0 else 8                    # 4x4 units of the SB's plane area per side
            pw4, ph4 = (w4, h4) if plane == 0 else (w4 // 2, h4 // 2)
            order = sorted(((_zorder(x, y), x, y) for y in range(u) for x in range(u)))
            for z, lx, ly in order:
                x4, y4 = sc * u + lx, sr * u + ly
                if x4 >= pw4 or y4 >= ph4:
                    continue
                r = rec_at(plane, x4, y4)
                if int(r["sb_type"]) > 12 or int(r["skip"]):
                    continue
                ts = ts_at(plane, x4, y4)
                s = 1 << ts
                if x4 % s or y4 % s:
                    continue
                tt = 0
                if plane == 0 and ts < 3:
                    if int(r["is_inter"]):
                        tt = int(r["pad"][0]) & 3
                    elif int(r["sb_type"]) == 0:
                        k = (y4 & 1) * 2 + (x4 & 1)
                        mode = (int(r["pad"][1]) >> (4 * k)) & 15 if k < 2 else (int(r["pad"][0]) >> (4 * (k - 2))) & 15
                        tt = INTRA_TX_TYPE[mode]
                    else:
                        tt = INTRA_TX_TYPE[int(r["pad"][1])]
                above = int(any(nz_at(plane, x4 + k, y4 - 1) for k in range(s))) if y4 else 0
                left = int(any(nz_at(plane, x4 - 1, y4 + k) for k in range(s))) if x4 else 0
                out.append(dict(plane=plane, x4=x4, y4=y4, ts=ts, tt=tt, inter=int(r["is_inter"]), eob=int(maps[plane][y4, x4]), ctx=above + left, sb=sb,
                                coeff_off=sb * B.SB_COEFFS + (0, 4096, 5120)[plane] + z * 16, map_index=eoff[plane] + y4 * pw4 + x4))
    return out


def tokenize_picture(lf_mi, qcoeff, eob_map, W, H):
    """picture form: dict(tokens, tok_off (shape of the eob map), sb_off[n_sb + 1], counts, blocks)"""
    blocks = picture_blocks(lf_mi, eob_map, W, H)
    n_sb = ((W + 63) // 64) * ((H + 63) // 64)
    tok_off = np.full(eob_map.size, NO_OFFSET, np.uint32)
    sb_off = np.zeros(n_sb + 1, np.uint32)
    toks, pos = [], 0
    for b in blocks:
        n = 16 << (2 * b["ts"])
        t = tokenize_block(qcoeff[b["coeff_off"]:b["coeff_off"] + n], b["ts"], b["tt"], b["eob"], int(b["plane"] != 0), b["inter"], b["ctx"])
        assert len(t) == b["eob"] + (b["eob"] < n)
        tok_off[b["map_index"]] = pos
        b["tok_off"] = pos
        toks.append(t)
        pos += len(t)
        sb_off[b["sb"] + 1:] = pos
    t = np.concatenate(toks) if toks else np.zeros(0, np.uint32)
    return dict(tokens=t, tok_off=tok_off, sb_off=sb_off, counts=counts_of(t), blocks=blocks)


# ---------------------------------------------------------------------------------------------------
# ctypes wrappers of the product's host entry points
# ---------------------------------------------------------------------------------------------------
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def product_scan_tables():
    """svt_hip_vp9_scan_tables -> ([16 offsets], int16 array)"""
    entries, poff = C.c_int32(), C.POINTER(C.c_uint32)()
    p = B.load().svt_hip_vp9_scan_tables(C.byref(poff), C.byref(entries))
    return [int(poff[i]) for i in range(16)], np.ctypeslib.as_array(p, (entries.value,)).copy()


def blocks_call(fn, case, capacity=None, counts=True, ctx=None):
    """svt_hip_tokenize_blocks_host (ctx None) or svt_hip_tokenize_blocks: (tokens[:min(total, capacity)], tok_off, counts, guard words)"""
    nb = len(case["blocks"])
    cap = int(sum(16 << (2 * int(t)) for t in case["blocks"]["tx_size"])) if capacity is None else capacity
    tokens = np.full(cap + 64, 0xA5A5A5A5, np.uint32)
    tok_off = np.zeros(nb + 1, np.uint32)
    cnt = np.full(N_COUNTS, 7, np.uint32)
    args = (_vp(case["qcoeff"]), C.c_size_t(case["qcoeff"].size), _vp(case["blocks"]), nb, _vp(tokens), C.c_uint32(cap), _vp(tok_off), _vp(cnt) if counts else None)
    rc = fn(*args) if ctx is None else fn(ctx, *args)
    assert rc == 0, rc
    return tokens[:min(int(tok_off[-1]), cap)].copy(), tok_off, cnt if counts else None, tokens[cap:]


def host_tokenize_blocks(case, **kw):
    return blocks_call(B.load().svt_hip_tokenize_blocks_host, case, **kw)


def host_tokenize_picture(lf_mi, qcoeff, eob_map, W, H, capacity=None, counts=True):
    """svt_hip_tokenize_picture -> dict like tokenize_picture's"""
    lib = B.load()
    cap = int(lib.svt_hip_tokenize_capacity(W, H)) if capacity is None else capacity
    mi = np.ascontiguousarray(lf_mi)
    q, em = np.ascontiguousarray(qcoeff, np.int16), np.ascontiguousarray(eob_map, np.uint16)
    n_sb = ((W + 63) // 64) * ((H + 63) // 64)
    tokens = np.full(cap + 64, 0xA5A5A5A5, np.uint32)
    tok_off, sb_off, cnt = np.zeros(em.size, np.uint32), np.zeros(n_sb + 1, np.uint32), np.full(N_COUNTS, 7, np.uint32)
    p = B.TokPicture()
    p.d_lf_mi, p.d_qcoeff, p.d_eob_map, p.d_tokens, p.capacity = mi.ctypes.data, q.ctypes.data, em.ctypes.data, tokens.ctypes.data, cap
    p.d_tok_off, p.d_sb_off, p.d_counts = tok_off.ctypes.data, sb_off.ctypes.data, cnt.ctypes.data if counts else None
    rc = lib.svt_hip_tokenize_picture(C.byref(p), W, H, mi.shape[1])
    assert rc == 0, rc
    return dict(tokens=tokens[:min(int(sb_off[-1]), cap)].copy(), tok_off=tok_off, sb_off=sb_off, counts=cnt if counts else None, guard=tokens[cap:])


def with_stride(lf_mi, extra, seed=0):
    """the grid in rows `extra` records wider (mi_stride = mi_cols + extra; the wrappers above take the stride from the array's shape):
    the records behind the picture's last column hold random bytes, which nothing may read"""
    rows, cols = lf_mi.shape
    noise = np.random.default_rng(7000 + seed).integers(0, 256, rows * (cols + extra) * lf_mi.dtype.itemsize, dtype=np.uint8)
    wide = noise.view(lf_mi.dtype).reshape(rows, cols + extra).copy()
    wide[:, :cols] = lf_mi
    return wide


# ---------------------------------------------------------------------------------------------------
# blocks at the boundaries of the token classes (shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------------------------------
# value -> (token, extra), written out by hand: extra = (|v| - smallest |v| of the class) << 1 | sign, low 16 bits
BOUNDARY = ((1, 1, 0), (-1, 1, 1), (4, 4, 0), (-4, 4, 1), (5, 5, 0), (-5, 5, 1), (6, 5, 2), (-6, 5, 3), (7, 6, 0), (-7, 6, 1), (10, 6, 6), (-10, 6, 7),
            (11, 7, 0), (-11, 7, 1), (18, 7, 14), (-18, 7, 15), (19, 8, 0), (-19, 8, 1), (34, 8, 30), (-34, 8, 31), (35, 9, 0), (-35, 9, 1),
            (66, 9, 62), (-66, 9, 63), (67, 10, 0), (-67, 10, 1), (32767, 10, 65400), (-32768, 10, 65403))


def boundary_case():
    """a block-form case (qcoeff, blocks, tx_type) + per block the expected [(token, extra)] list: the 28 boundary values in two 4x4 blocks
    and one 32x32 block (each followed by an EOB token), a full block (eob == n: no EOB token) and an empty one (eob == 0: one EOB token)
    of each of the four sizes"""
    offs, tab = scan_tables()
    q, blocks, tx_type, expect = [], [], [], []

    def add(ts, tt, ptype, inter, ctx, values):
        n = 16 << (2 * ts)
        so = offs[(ts, tt)]
        coeff = np.zeros(n, np.int16)
        coeff[tab[so:so + len(values)]] = [v for v, _, _ in values]
        blocks.append((sum(len(c) for c in q), so, len(values), ts, ptype, inter, ctx, (0, 0)))
        tx_type.append(tt)
        q.append(coeff)
        expect.append([(t, e) for _, t, e in values] + ([(EOB_TOKEN, 0)] if len(values) < n else []))

    add(0, 1, 0, 0, 1, BOUNDARY[:14])
    add(0, 0, 1, 1, 2, BOUNDARY[14:])
    add(3, 0, 0, 1, 0, BOUNDARY)
    for ts in range(4):
        n = 16 << (2 * ts)
        add(ts, (ts + 1) % 4 if ts < 3 else 0, 0, 0, ts % 3, [BOUNDARY[(5 * i) % len(BOUNDARY)] for i in range(n)])
        add(ts, 0, ts & 1, 1, (ts + 1) % 3, [])
    return dict(qcoeff=np.concatenate(q), blocks=np.array(blocks, dtype=B.RATE_BLOCK_DTYPE), tx_type=np.array(tx_type, np.int32)), expect


def check_boundary(case, expect, tokens, tok_off):
    for i, (b, want) in enumerate(zip(case["blocks"], expect)):
        tok, row, extra = unpack(tokens[int(tok_off[i]):int(tok_off[i + 1])])
        assert [(int(t), int(e)) for t, e in zip(tok, extra)] == want, i
        ts, n = int(b["tx_size"]), 16 << (2 * int(b["tx_size"]))
        assert len(want) == int(b["eob"]) + (int(b["eob"]) < n)
        assert np.all(row // 36 == (ts * 2 + int(b["plane_type"])) * 2 + int(b["is_inter"]))
        if int(b["eob"]) == 0:      # one EOB token, band 0, the block's context
            assert len(tok) == 1 and int(row[0]) % 36 == int(b["ctx"])
        if int(b["eob"]) == n:
            assert EOB_TOKEN not in tok


# ---------------------------------------------------------------------------------------------------
# the reference fixture (tests/golden/tokens_reference.npz, written by gen_golden_tokens.py)
# ---------------------------------------------------------------------------------------------------
_fixture_cache = None


def fixture_pictures():
    """(W, H, [dict(lf_mi, qcoeff, eob_map, blocks [n][plane, x4, y4, n_tokens], tokens [n][token, extra, row], counts)])"""
    global _fixture_cache
    if _fixture_cache is None:
        import os
        g = np.load(os.path.join(T.GOLDEN_DIR, "tokens_reference.npz"))
        W, H = (int(v) for v in g["size"])
        pics, k = [], 0
        while f"lf_mi|{k}" in g.files:
            lf = g[f"lf_mi|{k}"].view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
            tokens = np.stack([g[f"token|{k}"].astype(np.int32), g[f"extra|{k}"].astype(np.int32), g[f"row|{k}"].astype(np.int32)], axis=1)
            pics.append(dict(lf_mi=lf, qcoeff=g[f"qcoeff|{k}"], eob_map=g[f"eob_map|{k}"], blocks=g[f"blocks|{k}"].astype(np.int32), tokens=tokens,
                             counts=g[f"counts|{k}"]))
            k += 1
        _fixture_cache = (W, H, pics)
    return _fixture_cache


def check_against_fixture(pic, got, W, H):
    """got: a picture-form result (tokens, tok_off, sb_off, counts) against the reference's record of the same picture"""
    w4, h4 = W // 4, H // 4
    eoff = (0, w4 * h4, w4 * h4 + (w4 // 2) * (h4 // 2))
    tok, row, extra = unpack(got["tokens"])
    seen, pos = set(), 0
    sb_cols = (W + 63) // 64
    for plane, x4, y4, n in pic["blocks"]:
        idx = eoff[plane] + y4 * (w4 // 2 if plane else w4) + x4
        off = int(got["tok_off"][idx])
        assert off != NO_OFFSET, (plane, x4, y4)
        ref = pic["tokens"][pos:pos + n]
        pos += n
        assert np.array_equal(tok[off:off + n], ref[:, 0]) and np.array_equal(row[off:off + n], ref[:, 2]), (plane, x4, y4)
        has_extra = (ref[:, 0] >= 1) & (ref[:, 0] <= 10)
        assert np.array_equal(extra[off:off + n][has_extra], ref[:, 1][has_extra]), (plane, x4, y4)
        assert np.all(extra[off:off + n][~has_extra] == 0)
        u = 8 if plane else 16
        sb = (y4 // u) * sb_cols + x4 // u
        assert int(got["sb_off"][sb]) <= off and off + n <= int(got["sb_off"][sb + 1])
        seen.add(idx)
    assert set(np.nonzero(got["tok_off"] != NO_OFFSET)[0].tolist()) == seen
    assert int(got["sb_off"][0]) == 0 and int(got["sb_off"][-1]) == pos == len(got["tokens"]) and np.all(np.diff(got["sb_off"].astype(np.int64)) >= 0)
    assert np.array_equal(got["counts"], pic["counts"])

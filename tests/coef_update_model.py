"""Python model of the forward coefficient-probability update (csrc/coef_update_core.h): update_coef_probs of the reference
(VPX/vp9_bitstream.c:511-687, TWO_LOOP) with the searches and the sub-exponential code of VPX/vp9_subexp.c, written independently of the C
text -- the branch counts by walking the coefficient tree, the remap table built by split_index as the reference's comment says it was
generated, the bools of an update by running the code and counting -- plus the eob_branch histogram over a token stream, as one run and
block by block, and the callers of the product's host form.  Sums are Python / 64-bit integers: the true ones; `peak` of a decision is
the largest magnitude any sum reached, which says whether the reference's 32-bit sums would have wrapped."""
import ctypes as C
import os

import numpy as np

import boolcode_model as BM
import svt_testlib as T

B = T.B
GOLD = os.path.join(T.GOLDEN_DIR, "coef_update_reference.npz")
EOB_TOKEN = 11
# eb_vp9_coef_tree (VPX/vp9_tokenize.c:57-69): a positive entry is the index of a node pair, -t (and 0) a token
COEF_TREE = (-11, 2, 0, 4, -1, 6, 8, 12, -2, 10, -3, -4, 14, 16, -5, -6, 18, 20, -7, -8, -9, -10)
UPD = 252
MIN_DELP_BITS, COST_SHIFT, TX_TOTAL_MIN = 5, 9, 20


def rec(bit, prob):
    return (bit << 8) | prob


# ---- the token stream ------------------------------------------------------------------------------------------------------------
def unpack(records):
    r = np.asarray(records, np.uint32)
    return (r & 15).astype(np.int64), ((r >> 4) & 0xFFF).astype(np.int64)


def node0_coded(tok, row):
    """per record of ONE run: node 0 is coded unless the record in front is ZERO and the record's band is not 0"""
    band = (row // 6) % 6
    prev_zero = np.concatenate([[False], tok[:-1] == 0])
    return ~(prev_zero & (band != 0))


def eob_branch(records):
    tok, row = unpack(records)
    ok = node0_coded(tok, row) & (row < 576)
    return np.bincount(row[ok], minlength=576)[:576].astype(np.uint32)


def eob_branch_per_block(records, starts):
    """the same histogram with the predecessor test restarted at every block (starts: sorted first records of the blocks)"""
    out = np.zeros(576, np.int64)
    cuts = list(starts) + [len(records)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += eob_branch(records[a:b])
    return out.astype(np.uint32)


def counts_of(records):
    tok, row = unpack(records)
    c = np.zeros((576, 12), np.uint32)
    np.add.at(c, (row, tok), 1)
    return c.reshape(-1)


# ---- tables by their rules ---------------------------------------------------------------------------------------------------------
def split_index(i, n, modulus):
    max1 = (n - 1 - modulus // 2) // modulus + 1
    return i // modulus if i % modulus == modulus // 2 else max1 + i - (i + modulus - modulus // 2) // modulus


MAP_TABLE = [split_index(j, 254, 13) for j in range(254)]


def recenter_nonneg(v, m):
    return v if v > 2 * m else 2 * (v - m) if v >= m else 2 * (m - v) - 1


def remap_prob(v, m):
    v, m = v - 1, m - 1
    i = recenter_nonneg(v, m) - 1 if 2 * m <= 255 else recenter_nonneg(254 - v, 254 - m) - 1
    return MAP_TABLE[i]


def literal(v, bits):
    return [rec((v >> b) & 1, 128) for b in range(bits - 1, -1, -1)]


def term_subexp(word):
    if word < 16:
        return literal(0, 1) + literal(word, 4)
    if word < 32:
        return literal(1, 1) + literal(0, 1) + literal(word - 16, 4)
    if word < 64:
        return literal(1, 1) + literal(1, 1) + literal(0, 1) + literal(word - 32, 5)
    v, m = word - 64, (1 << 8) - 191
    head = literal(1, 1) * 3
    return head + literal(v, 7) if v < m else head + literal(m + ((v - m) >> 1), 7) + literal((v - m) & 1, 1)


UPDATE_BITS = [len(term_subexp(d)) for d in range(254)]


def remap_tables():
    """[(newp - 1) * 255 + oldp - 1] for all pairs: the remap index and the bools of the update (0 on the diagonal)"""
    remap, bits = np.zeros(255 * 255, np.uint8), np.zeros(255 * 255, np.uint8)
    for n in range(1, 256):
        for o in range(1, 256):
            if n != o:
                remap[(n - 1) * 255 + o - 1] = remap_prob(n, o)
                bits[(n - 1) * 255 + o - 1] = UPDATE_BITS[remap_prob(n, o)]
    return remap, bits


_REMAP = None


def _remap_matrix():
    global _REMAP
    if _REMAP is None:
        _REMAP = remap_tables()[1].reshape(255, 255).astype(np.int64)
    return _REMAP


_gold = None


def fixture():
    global _gold
    if _gold is None:
        g = np.load(GOLD)
        _gold = {k: g[k] for k in g.files}
    return _gold


def cost_table():
    return fixture()["prob_cost"].astype(np.int64)


# ---- the decision ------------------------------------------------------------------------------------------------------------------
def branch_counts(counts12, eob):
    """[11][2] through the tree, then node 0's second count from eob_branch (32-bit, as the reference subtracts)"""
    ct = [[0, 0] for _ in range(11)]

    def walk(i):
        side = []
        for k in (0, 1):
            t = COEF_TREE[i + k]
            side.append(int(counts12[-t]) if t <= 0 else walk(t))
        ct[i >> 1] = side
        return (side[0] + side[1]) & 0xFFFFFFFF
    walk(0)
    ct[0][1] = (int(eob) - ct[0][0]) & 0xFFFFFFFF
    return ct


def binary_prob(n0, n1):
    den = (n0 + n1) & 0xFFFFFFFF
    if den == 0:
        return 128
    return min(255, max(1, (n0 * 256 + (den >> 1)) // den))


def entries():
    """(row inside the size, node) of the 396 entries in the reference's order"""
    out = []
    for i in range(2):
        for j in range(2):
            for k in range(6):
                for l in range(3 if k == 0 else 6):
                    for t in range(3):
                        out.append((((i * 2 + j) * 6 + k) * 6 + l, t))
    return out


ENTRIES = entries()


def search(ct, node, oldp, newp, cost, pareto, stats):
    """(savings, best probability); stats["peak"] = the largest |sum| met"""
    upd_cost = int(cost[256 - UPD] - cost[UPD])
    step = -1 if newp > oldp else 1
    cand = np.arange(newp, oldp, step, dtype=np.int64)

    def total(ps):
        ps = np.atleast_1d(ps)
        if node < 2:
            return ct[node][0] * cost[ps] + ct[node][1] * cost[256 - ps]
        b = ct[2][0] * cost[ps] + ct[2][1] * cost[256 - ps]
        for i in range(3, 11):
            q = pareto[ps - 1, i - 3].astype(np.int64)
            b = b + ct[i][0] * cost[q] + ct[i][1] * cost[256 - q]
        return b
    old_b = int(total(np.int64(oldp))[0])
    stats["peak"] = max(stats.get("peak", 0), abs(old_b))
    if old_b <= upd_cost + (MIN_DELP_BITS << COST_SHIFT) or len(cand) == 0:
        return 0, oldp
    new_b = total(cand)
    stats["peak"] = max(stats["peak"], int(np.abs(new_b).max()))
    sav = old_b - new_b - (_remap_matrix()[cand - 1, oldp - 1] << COST_SHIFT) - upd_cost
    k = int(np.argmax(sav))             # the first of equals, in the order the candidates are tried
    return (int(sav[k]), int(cand[k])) if sav[k] > 0 else (0, oldp)


def decide(counts, eob, old_probs, cost=None, pareto=None, prefix=(), suffix=()):
    """counts[6912], eob[576], old_probs[1728] -> dict(bools, probs, updated[4], sent[4], savings[4], peak, arms)"""
    cost = cost_table() if cost is None else np.asarray(cost, np.int64)
    pareto = BM.tables()[0]["pareto"] if pareto is None else pareto
    counts = np.asarray(counts, np.int64).reshape(576, 12)
    eob = np.asarray(eob, np.int64)
    probs = np.array(old_probs, np.uint8).copy()
    old = np.asarray(old_probs, np.int64)
    bools, stats = list(prefix), {}
    updated, sent, savings, arms = [0] * 4, [0] * 4, [0] * 4, set()
    for ts in range(4):
        e144 = eob[144 * ts:144 * ts + 144]
        if int(sum(e144[ij * 36 + l] for ij in range(4) for l in range(6))) <= TX_TOTAL_MIN:
            bools.append(rec(0, 128))
            continue
        res = []
        for row, node in ENTRIES:
            r = 144 * ts + row
            ct = branch_counts(counts[r], eob[r])
            oldp = int(old[3 * r + node])
            s, newp = search(ct, node, oldp, binary_prob(*ct[node]), cost, pareto, stats)
            u = int(s > 0 and newp != oldp)
            res.append((r, node, u, newp, oldp))
            savings[ts] += (s if u else 0) - int(cost[UPD])
            updated[ts] += u
        stats["peak"] = max(stats.get("peak", 0), abs(savings[ts]))
        sent[ts] = int(updated[ts] != 0 and savings[ts] >= 0)
        arms.add("exit_sent" if sent[ts] else "exit_none" if updated[ts] == 0 else "exit_negative")
        bools.append(rec(sent[ts], 128))
        if not sent[ts]:
            continue
        for r, node, u, newp, oldp in res:
            bools.append(rec(u, UPD))
            if u:
                d = remap_prob(newp, oldp)
                arms.add("subexp_16" if d < 16 else "subexp_32" if d < 32 else "subexp_64" if d < 64 else "uniform_short" if d - 64 < 65 else "uniform_long")
                arms.add("newp_above" if newp > oldp else "newp_below")
                bools += term_subexp(d)
                probs[3 * r + node] = newp
    bools += list(suffix)
    return dict(bools=np.array(bools, np.uint16), probs=probs, updated=updated, sent=sent, savings=savings, peak=stats.get("peak", 0), arms=arms)


# ---- the product's host form -------------------------------------------------------------------------------------------------------
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def host_picture(tokens, counts, old_probs=None, prefix=(), suffix=(), tabs=None, device_count=False, max_tokens=None):
    """svt_hip_coef_update_picture: dict(eob, probs, bools, n, segment, result, guard)"""
    lib = B.load()
    tokens = np.ascontiguousarray(tokens, np.uint32)
    counts = np.ascontiguousarray(counts, np.uint32)
    cap = int(lib.svt_hip_coef_update_bools_capacity())
    eob, probs = np.full(576, 0x77777777, np.uint32), np.full(1728, 0xA5, np.uint8)
    bools, n = np.full(cap + 64, 0xA5A5, np.uint16), np.full(1, 0x77777777, np.uint32)
    seg, res = np.zeros(1, B.BOOL_SEGMENT_DTYPE), np.zeros(1, B.CU_RESULT_DTYPE)
    ntok = np.array([len(tokens)], np.uint32)
    old = None if old_probs is None else np.ascontiguousarray(old_probs, np.uint8)
    p = B.CuPicture()
    p.d_tokens = tokens.ctypes.data if len(tokens) else None
    p.d_n_tokens, p.n_tokens = (ntok.ctypes.data, 0) if device_count else (None, len(tokens))
    p.max_tokens = len(tokens) if max_tokens is None else max_tokens
    p.d_counts, p.d_old_probs = counts.ctypes.data, None if old is None else old.ctypes.data
    p.d_eob_branch, p.d_probs, p.d_hdr_bools, p.d_n_hdr_bools = eob.ctypes.data, probs.ctypes.data, bools.ctypes.data, n.ctypes.data
    p.d_segment, p.d_result = seg.ctypes.data, res.ctypes.data
    p.n_prefix, p.n_suffix = len(prefix), len(suffix)
    for i, v in enumerate(prefix):
        p.prefix[i] = v
    for i, v in enumerate(suffix):
        p.suffix[i] = v
    tabs = BM.tables()[1] if tabs is None else tabs
    rc = lib.svt_hip_coef_update_picture(C.byref(p), _vp(tabs))
    assert rc == 0, rc
    return dict(eob=eob, probs=probs, bools=bools[:int(n[0])].copy(), n=int(n[0]), segment=tuple(int(seg[0][k]) for k in ("first", "count", "kind")),
                result=res[0].copy(), guard=bools[cap:])


def tables_with(coef_probs):
    """the C bool tables with other coefficient probabilities"""
    t = BM.tables()[1].copy()
    t["coef_probs"][0] = coef_probs
    return t


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------
def seeded_counts(seed, scale=400, shape=None):
    """coef_counts and a consistent eob_branch (>= the EOB count, <= the row's total) for every row; `shape` tilts the token distribution
    away from the defaults: "zeros" towards ZERO / EOB, "large" towards the categories"""
    rng = np.random.default_rng(seed)
    w = {None: np.array([30, 20, 8, 4, 3, 3, 2, 2, 1, 1, 1, 25.]), "zeros": np.array([200, 6, 1, 1, 0, 0, 0, 0, 0, 0, 0, 90.]),
         "large": np.array([3, 5, 8, 9, 9, 12, 12, 10, 8, 6, 4, 2.])}[shape]
    c = np.zeros((576, 12), np.uint32)
    for r in range(576):
        n = int(rng.integers(0, scale)) if rng.integers(0, 8) else 0
        if n:
            c[r] = rng.multinomial(n, rng.dirichlet(w + 0.05))
    tot = c.sum(axis=1)
    eob = (c[:, 11] + np.floor((tot - c[:, 11]) * rng.random(576))).astype(np.uint32)
    band0 = ((np.arange(576) // 6) % 6) == 0
    eob[band0] = tot[band0]                     # node 0 is always coded in band 0
    return c.reshape(-1), eob


def seeded_probs(seed, ends=False):
    rng = np.random.default_rng(seed)
    p = rng.integers(1, 256, 1728).astype(np.uint8)
    if ends:
        p[rng.integers(0, 1728, 300)] = 1
        p[rng.integers(0, 1728, 300)] = 255
    return p


TOKEN_MIX = dict(default=(45, 20, 8, 4, 3, 3, 2, 2, 1, 1, 1, 10), zeros=(70, 8, 2, 1, 0, 0, 0, 0, 0, 0, 0, 19), large=(4, 8, 10, 10, 10, 12, 12, 10, 8, 6, 4, 6),
                 ones=(10, 70, 4, 2, 1, 1, 0, 0, 0, 0, 0, 12))


def seeded_stream(seed, n=None, groups=None, mix="default", blocks=None, max_len=40):
    """a well-formed token stream: blocks of random length in random (size, plane, ref) groups (0 .. 15, or the given ones), the band from
    the position, a context the band has, tokens drawn from TOKEN_MIX[mix]; a block ends with EOB or, at max_len positions, with a token
    that is not ZERO, and EOB never follows ZERO.  Stops after n records (the last block is then closed) or after `blocks` blocks."""
    rng = np.random.default_rng(seed)
    p = np.array(TOKEN_MIX[mix], float) / sum(TOKEN_MIX[mix])
    out, n_blocks = [], 0
    while (n is None or len(out) < n) and (blocks is None or n_blocks < blocks):
        grp = int(rng.integers(0, 16)) if groups is None else int(rng.choice(groups))
        prev = -1
        for c in range(max_len):
            t = int(rng.choice(12, p=p))
            last = c == max_len - 1 or (n is not None and len(out) == n - 1)
            if t == 11 and prev == 0:
                t = 1
            if last and t == 0:
                t = 2
            band = 0 if c == 0 else 1 if c < 3 else 2 if c < 6 else 3 if c < 10 else 4 if c < 21 else 5
            ctx = int(rng.integers(0, 3 if band == 0 else 6))
            out.append(((int(rng.integers(0, 1 << 16)) if t not in (0, 11) else 0) << 16) | (((grp * 6 + band) * 6 + ctx) << 4) | t)
            prev = t
            if t == 11 or last:
                break
        n_blocks += 1
    return np.array(out, np.uint32)


def block_starts(records):
    """first records of the blocks of a seeded stream: position 0 is band 0"""
    _, row = unpack(records)
    return np.flatnonzero((row // 6) % 6 == 0)


# ---- the chain around the stage, on the host -----------------------------------------------------------------------------------------
def header_parts(fp):
    """svt_hip_frame_header_parts_host: (prefix records, suffix records) of a parameter set (tests/frame_model.py)"""
    import frame_model as FM
    pre, suf = np.zeros(B.CU_PREFIX_MAX, np.uint16), np.zeros(B.CU_SUFFIX_MAX, np.uint16)
    n_pre, n_suf = C.c_uint32(), C.c_uint32()
    s = FM.struct(fp)
    rc = B.load().svt_hip_frame_header_parts_host(C.byref(s), _vp(pre), C.byref(n_pre), _vp(suf), C.byref(n_suf))
    assert rc == 0, rc
    return tuple(int(v) for v in pre[:n_pre.value]), tuple(int(v) for v in suf[:n_suf.value])


def header_coef(fp, bools, capacity=None):
    """svt_hip_frame_header_coef_host: (rc, header bytes, uncompressed bytes, compressed bytes, guard)"""
    import frame_model as FM
    bools = np.ascontiguousarray(bools, np.uint16)
    cap = 64 + int(B.load().svt_hip_boolcode_capacity(len(bools))) if capacity is None else capacity
    buf = np.full(cap + 16, 0xA5, np.uint8)
    ub, cb = C.c_uint32(0), C.c_uint32(0)
    s = FM.struct(fp)
    rc = B.load().svt_hip_frame_header_coef_host(C.byref(s), _vp(bools), len(bools), _vp(buf), cap, C.byref(ub), C.byref(cb))
    return rc, bytes(buf[:ub.value + cb.value]) if rc == 0 else b"", ub.value, cb.value, buf[cap:]


def real_pictures():
    """[(name, kind, picture, frame parameters)]: the three inter pictures of md_inter_reference.npz and a key frame of frame_reference.npz,
    every one coded from the default probabilities with refresh_frame_context 0"""
    import frame_model as FM
    import md_inter_model as DM
    import modes_model as MM
    out = []
    for name, W, H, *_ in DM.GOLDEN:
        pic = DM.golden_picture(name)
        fr = pic["frame"]
        fp = FM.inter(width=W, height=H, reference_mode=fr["reference_mode"], allow_comp_inter_inter=int(fr["reference_mode"] != FM.SINGLE), allow_hp=fr["allow_hp"],
                      ref_frame_sign_bias=fr["sign_bias"], refresh_frame_context=0, frame_parallel_decoding_mode=1)
        out.append((name, "inter", pic, fp))
    name, kind, pname, fp = FM.WHOLE[0]
    assert kind == "modes"
    out.append((name, "key", MM.fixture_picture(pname), dict(fp, refresh_frame_context=0, frame_parallel_decoding_mode=1)))
    return out


def assemble(header, ub, tile):
    """the existing frame assembly (svt_hip_frame_assemble_host): a packet's header field holds SVT_FRAME_HEADER_MAX bytes, too few for a
    compressed header with updates, so the uncompressed header goes there and compressed header || tile is the packet's coded part"""
    coded = np.frombuffer(header[ub:] + tile, np.uint8).copy()
    size, arena, table = np.array([len(coded)], np.uint32), np.full(len(header) + len(tile) + 32, 0xA5, np.uint8), np.zeros(2, B.FRAME_ENTRY_DTYPE)
    pk = B.FramePacket()
    pk.d_tile, pk.d_tile_size, pk.tile_capacity, pk.header_len, pk.trailer_len = coded.ctypes.data, size.ctypes.data, len(coded), ub, 0
    for i in range(ub):
        pk.header[i] = header[i]
    rc = B.load().svt_hip_frame_assemble_host(1, C.byref(pk), _vp(arena), len(arena), _vp(table))
    assert rc == 0 and tuple(table[0]) == (0, ub + len(coded)) and np.all(arena[ub + len(coded):] == 0xA5)
    return bytes(arena[:ub + len(coded)])


_chain_cache = {}


def host_stream(kind, pic):
    """host tokeniser and host mode-info stage of a picture: dict(tokens, counts, tok, bools, segments) (shared, left unchanged)"""
    import modes_inter_model as IM
    import modes_model as MM
    import tokenize_model as TM
    key = id(pic)
    if key not in _chain_cache:
        tok = TM.host_tokenize_picture(pic["lf_mi"], pic["qcoeff"], pic["eob_map"], pic["W"], pic["H"])
        m = MM.host_modes(pic["lf_mi"], pic["eob_map"], tok["tok_off"], pic["W"], pic["H"]) if kind == "key" else IM.host_modes(pic, tok["tok_off"])
        assert m["rc"] == 0
        _chain_cache[key] = dict(tokens=tok["tokens"], counts=tok["counts"], tok=tok, bools=m["bools"], segments=[tuple(int(v) for v in s) for s in m["segments"]], pic=pic)
    return _chain_cache[key]


def host_frame(kind, pic, fp, update=True, old_probs=None):
    """the all-host chain: tokeniser -> the stage -> mode info -> bool coder under the new table -> the two headers -> the frame assembly;
    dict(frame, header, tile, probs, stage)"""
    import frame_model as FM
    s = host_stream(kind, pic)
    if update:
        pre, suf = header_parts(fp)
        st = host_picture(s["tokens"], s["counts"], old_probs=old_probs, prefix=pre, suffix=suf)
        rc, hdr, ub, cb, _ = header_coef(fp, st["bools"])
        assert rc == 0
        probs = st["probs"]
    else:
        st, hdr, ub = None, FM.host_header_bytes(fp), None
        probs = BM.tables()[0]["coef_probs"].reshape(-1) if old_probs is None else old_probs
    tile = BM.product_call(B.load().svt_hip_boolcode_host, s["tokens"], s["bools"], s["segments"], tabs=tables_with(probs))[0]
    frame = assemble(hdr, ub, tile) if update else hdr + tile
    assert frame == hdr + tile
    return dict(frame=frame, header=hdr, tile=tile, probs=probs, stage=st)

"""Python model of the VP9 bool coder, written independently of the C text (csrc/boolcode_core.h, host/boolcode_host.c):
  - token record -> bools by a walk of the coefficient tree as the VP9 specification prints it;
  - serial_write: the plain serial writer (low end, range, bit count, backward carry walk), which also reports its carry events;
  - bigint_write: the output as ONE integer sum, V = sum of split_i << (S - S_(i-1)) over the 1-bools, the form the kernels rest on;
  - chunked_write: the kernels' decomposition (chunk maps over the 128 ranges, chain, 64-bit sums of 32-bit words, fold + generate /
    propagate carries) in plain Python with the chunk and tile sizes as arguments;
  - the raw bool streams and the token-level cases the fixture, the CPU tests and the GPU tests share."""
import ctypes as C
import os

import numpy as np

import svt_testlib as T

B = T.B
GOLD = os.path.join(T.GOLDEN_DIR, "boolcode_reference.npz")
EOB_TOKEN = 11
# the coefficient tree below its three unconstrained nodes (leaves: -token), and the bits of the categories' offsets
CON_TREE = (2, 6, -2, 4, -3, -4, 8, 10, -5, -6, 12, 14, -7, -8, -9, -10)
CAT_BITS = {5: 1, 6: 2, 7: 3, 8: 4, 9: 5, 10: 14}
HALF = 128


def rec(bit, prob):
    return (int(bit) << 8) | int(prob)


def _tree_path(tok):
    """[(node index into the pareto row, bit)] that leads to the leaf -tok"""
    def walk(i, path):
        for bit in (0, 1):
            nxt = CON_TREE[i + bit]
            here = path + [(i >> 1, bit)]
            if nxt == -tok:
                return here
            if nxt > 0:
                r = walk(nxt, here)
                if r:
                    return r
        return None
    return walk(0, [])


def band_of_row(row):
    return (row // 6) % 6


def token_bools(tok, extra, row, skip0, tables):
    """the uint16 bool records of one token record"""
    p = tables["coef_probs"][3 * row:3 * row + 3]
    if tok == EOB_TOKEN:
        return [rec(0, p[0])]
    out = [] if skip0 else [rec(1, p[0])]
    if tok == 0:
        return out + [rec(0, p[1])]
    out.append(rec(1, p[1]))
    if tok == 1:
        return out + [rec(0, p[2]), rec(extra & 1, HALF)]
    out.append(rec(1, p[2]))
    pareto = tables["pareto"][int(p[2]) - 1]
    out += [rec(bit, pareto[node]) for node, bit in _tree_path(tok)]
    if tok >= 5:
        n, v = CAT_BITS[tok], extra >> 1
        out += [rec((v >> (n - 1 - k)) & 1, tables["cat_probs"][tok - 5][k]) for k in range(n)]
    return out + [rec(extra & 1, HALF)]


def unpack(records):
    r = np.asarray(records, np.uint32)
    return (r & 15).astype(np.int64), ((r >> 4) & 0xFFF).astype(np.int64), (r >> 16).astype(np.int64)


def expand(tokens, bools, segments, tables):
    """the bools of a stream in coding order; segments None = all token records"""
    tokens = np.asarray(tokens, np.uint32)
    if segments is None:
        segments = [(0, len(tokens), 0)]
    out = []
    for first, count, kind in segments:
        if kind:
            out += [int(b) for b in bools[first:first + count]]
            continue
        tok, row, extra = unpack(tokens[first:first + count])
        for k in range(count):
            skip0 = k > 0 and tok[k - 1] == 0 and band_of_row(int(row[k])) != 0
            out += token_bools(int(tok[k]), int(extra[k]), int(row[k]), skip0, tables)
    return out


def framed(bools):
    return [rec(0, HALF)] + [int(b) for b in bools] + [rec(0, HALF)] * 32


def _norm(x):
    return 8 - x.bit_length()


def serial_write(bools, stats=None):
    """bytes of the stream; stats (a dict) receives carry_events, flipped (0xff bytes a carry turned to 0, the longest walk), runs (the
    byte range [first, end) of every walk) and marker (was the trailing zero byte added?)"""
    low, rng, count, buf = 0, 255, -24, bytearray()
    events, longest, where = 0, 0, []
    for b in framed(bools):
        split = 1 + (((rng - 1) * (b & 255)) >> 8)
        if b >> 8:
            low += split
            rng -= split
        else:
            rng = split
        shift = _norm(rng)
        rng <<= shift
        count += shift
        if count >= 0:
            offset = shift - count
            if (low << (offset - 1)) & 0x80000000:
                x, run = len(buf) - 1, 0
                while x >= 0 and buf[x] == 0xFF:
                    buf[x] = 0
                    x -= 1
                    run += 1
                buf[x] += 1
                events += 1
                longest = max(longest, run)
                where.append((x + 1, x + 1 + run))
            buf.append((low >> (24 - offset)) & 0xFF)
            low = (low << offset) & 0xFFFFFF
            shift = count
            count -= 8
        low = (low << shift) & 0xFFFFFFFF
    marker = (buf[-1] & 0xE0) == 0xC0
    if marker:
        buf.append(0)
    if stats is not None:
        stats.update(carry_events=events, flipped=longest, runs=where, marker=marker)
    return bytes(buf)


def bigint_write(bools):
    rng, S, terms = 255, 0, []
    for b in framed(bools):
        split = 1 + (((rng - 1) * (b & 255)) >> 8)
        if b >> 8:
            terms.append((split, S))
            rng -= split
        else:
            rng = split
        shift = _norm(rng)
        rng <<= shift
        S += shift
    V = sum(s << (S - p) for s, p in terms)
    nb = (S - 16) // 8
    out = (V >> (S - 8 * nb + 8)).to_bytes(nb, "big")
    return out + (b"\0" if (out[-1] & 0xE0) == 0xC0 else b"")


def chunked_write(bools, K, tile_words=4):
    """the kernels' decomposition: maps, chain, code, carry"""
    sym = framed(bools)
    M = len(sym)
    chunks = [sym[c:c + K] for c in range(0, M, K)]

    def step(r, b):
        split = 1 + (((r - 1) * (b & 255)) >> 8)
        x = r - split if b >> 8 else split
        sh = _norm(x)
        return x << sh, sh, split
    maps = []
    for ch in chunks:
        m = []
        for r0 in range(128, 256):
            r, s = r0, 0
            for b in ch:
                r, sh, _ = step(r, b)
                s += sh
            m.append((r, s))
        maps.append(m)
    r, S, start = 255, 0, []
    for m in maps:
        start.append((r, S))
        r, ds = m[r - 128]
        S += ds
    nb, W = (S - 16) // 8, (S + 8 + 31) // 32 + 1
    acc = [0] * (W + 1)
    for ch, (r, pos) in zip(chunks, start):
        wcur, a0, a1 = pos >> 5, 0, 0
        for b in ch:
            nr, sh, split = step(r, b)
            if b >> 8:
                w = pos >> 5
                if w != wcur:
                    acc[wcur] += a0
                    if w == wcur + 1:
                        a0 = a1
                    else:
                        acc[wcur + 1] += a1
                        a0 = 0
                    a1, wcur = 0, w
                t = split << (56 - (pos & 31))
                assert t < 1 << 64
                a0 += t >> 32
                a1 += t & 0xFFFFFFFF
            r, pos = nr, pos + sh
        acc[wcur] += a0
        acc[wcur + 1] += a1
    assert all(a < 1 << 64 for a in acc)
    words, cin = [0] * W, 0
    for tile in range((W + tile_words - 1) // tile_words - 1, -1, -1):
        ks = [k for k in range(tile * tile_words + tile_words - 1, tile * tile_words - 1, -1) if k < W]   # far end first
        for k in ks:
            v = (acc[k] & 0xFFFFFFFF) + (acc[k + 1] >> 32)
            g, l = v >> 32, v & 0xFFFFFFFF
            assert g <= 1 and not (g and l == 0xFFFFFFFF)
            words[k] = (l + cin) & 0xFFFFFFFF
            cin = g | (int(l == 0xFFFFFFFF) & cin)
    out = b"".join(w.to_bytes(4, "big") for w in words)[:nb]
    return out + (b"\0" if (out[-1] & 0xE0) == 0xC0 else b"")


# ---------------------------------------------------------------------------------------------------
# raw bool streams
# ---------------------------------------------------------------------------------------------------
def random_stream(seed, n):
    """n bools, each bit drawn to match its probability (prob / 256 is the chance of a 0)"""
    rng = np.random.default_rng(1000 + seed)
    p = rng.integers(1, 256, n)
    bit = rng.random(n) >= p / 256.0
    return [rec(b, q) for b, q in zip(bit, p)]


def straddle_stream(n, seed, pad=0):
    """a stream whose low end creeps up to a short dyadic number T for n steps and then crosses it: one carry through a long run of
    0xff bytes.  pad: (128, 0) bools in front (they leave the range at 128 and the low end at 0, so the stream behind them codes the
    same, pad bits later).  Returns (bools, index of the crossing bool)"""
    rng = np.random.default_rng(5000 + 97 * n + seed)
    out = [rec(0, HALF)] * pad
    # exact state: the interval is [L, L + r) in units of 2^-S
    L, r, S = 0, 255, 0

    def put(b):
        nonlocal L, r, S
        split = 1 + (((r - 1) * (b & 255)) >> 8)
        if b >> 8:
            L, r = L + split, r - split
        else:
            r = split
        sh = _norm(r)
        L, r, S = L << sh, r << sh, S + sh
    for b in [rec(0, HALF)] + out:
        put(b)
    # the dyadic number with the shortest expansion strictly inside (L, L + r): T = t / 2^S0
    k = (L + r).bit_length()
    while True:
        t = ((L >> k) + 1) << k
        if L < t < L + r:
            break
        k -= 1
    S0 = S
    steps = 0
    while steps < n:
        p = int(rng.integers(1, 256))
        split = 1 + (((r - 1) * p) >> 8)
        T_now = t << (S - S0)
        if L + split == T_now:
            continue
        b = rec(0 if L + split > T_now else 1, p)
        out.append(b)
        put(b)
        steps += 1
        assert L < (t << (S - S0)) < L + r
    while L < (t << (S - S0)):
        out.append(rec(1, 255))
        put(out[-1])
    return out, len(out) - 1


# raw streams past one pass of the device's scan over tiles of 1024 items (256 tiles a pass): at the pass boundary and two passes + 5
LONG_RAW = (256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, 2 * 256 * 1024 + 5)
CARRY_TILE_BYTES = 1024      # the device's carry scan walks the output 256 32-bit words at a time
_long_cache = {}


def long_raw_stream(n):
    """uint16 records of random_stream(n, n), made once"""
    if n not in _long_cache:
        rng = np.random.default_rng(1000 + n)        # random_stream's draws, without a Python list of n records
        p = rng.integers(1, 256, n)
        bit = rng.random(n) >= p / 256.0
        _long_cache[n] = ((bit.astype(np.uint16) << 8) | p.astype(np.uint16)).astype(np.uint16)
    return _long_cache[n]


def long_straddle(pad=0):
    """(uint16 records, byte range [first, end) of its one carry walk) of straddle_stream(40000, 0, pad): 0xff bytes over more than two whole
    tiles of the carry scan, which only hand the carry on"""
    key = ("straddle", pad)
    if key not in _long_cache:
        st = {}
        s = np.array(straddle_stream(40000, 0, pad)[0], np.uint16)
        serial_write(s, st)
        assert st["carry_events"] == 1
        _long_cache[key] = (s, st["runs"][0])
    return _long_cache[key]


_raw_cache = None


def raw_streams():
    """{name: uint16 array} in the fixture's order"""
    global _raw_cache
    if _raw_cache is not None:
        return _raw_cache
    out = {}
    for n in (0, 1, 2, 7, 8, 9):
        out[f"len{n}"] = random_stream(n, n)
    for p, b in ((255, 0), (1, 1), (255, 1), (128, 1)):
        out[f"const_{p}_{b}"] = [rec(b, p)] * 600
    marker, plain, seed = [], [], 0
    while len(marker) < 3 or len(plain) < 3:     # about one random stream in ten ends in the marker byte
        s = random_stream(seed, 200 + 13 * seed)
        st = {}
        serial_write(s, st)
        ends = st["marker"]
        if ends and len(marker) < 3:
            marker.append(seed)
            out[f"random_marker_{seed}"] = s
        elif not ends and len(plain) < 3:
            plain.append(seed)
            out[f"random_plain_{seed}"] = s
        seed += 1
    for n in (64, 200, 600):
        for seed in range(4):
            out[f"straddle_{n}_{seed}"] = straddle_stream(n, seed)[0]
    _raw_cache = {k: np.array(v, np.uint16) for k, v in out.items()}
    return _raw_cache


# ---------------------------------------------------------------------------------------------------
# token-level cases
# ---------------------------------------------------------------------------------------------------
CAT_BASE = (0, 1, 2, 3, 4, 5, 7, 11, 19, 35, 67)


def _row(ts, ptype, inter, band, ctx):
    return (((ts * 2 + ptype) * 2 + inter) * 6 + band) * 6 + ctx


def token_cases():
    """uint32 token records of well-formed blocks: every token class right behind node 0 and behind a ZERO (node 0 left out), both
    signs, the largest offset of every category (category 6: all 14 bits set), a run of ZEROs, an EOB-only block"""
    out = []

    def put(tok, extra, ts, ptype, inter, c, ctx):
        band = 0 if c == 0 else 1 if c < 3 else 2 if c < 6 else 3
        out.append((extra << 16) | (_row(ts, ptype, inter, band, ctx) << 4) | tok)
    k = 0
    for tok in range(1, 11):
        top = (CAT_BASE[tok + 1] - CAT_BASE[tok] - 1) if tok < 10 else 0x3FFF
        for mag in sorted({0, top}):
            for sign in (0, 1):
                ts, ptype, inter, ctx = k % 4, (k >> 1) & 1, k & 1, k % 3
                k += 1
                extra = ((mag << 1) | sign) & 0xFFFF
                put(tok, extra, ts, ptype, inter, 0, ctx)          # node 0 coded
                put(EOB_TOKEN, 0, ts, ptype, inter, 1, (ctx + 1) % 6)
                put(0, 0, ts, ptype, inter, 0, ctx)                # ZERO, then the token without node 0
                put(tok, extra, ts, ptype, inter, 1, (ctx + 2) % 6)
                put(EOB_TOKEN, 0, ts, ptype, inter, 2, ctx)
    put(EOB_TOKEN, 0, 1, 0, 1, 0, 2)
    for c in range(4):
        put(0, 0, 2, 1, 0, c, c % 3)
    put(1, 1, 2, 1, 0, 4, 5)
    put(EOB_TOKEN, 0, 2, 1, 0, 5, 1)
    return np.array(out, np.uint32)


# ---------------------------------------------------------------------------------------------------
# the fixture and the product's host entry point
# ---------------------------------------------------------------------------------------------------
_gold = None


def fixture():
    global _gold
    if _gold is None:
        g = np.load(GOLD)
        _gold = {k: g[k] for k in g.files}
    return _gold


def tables():
    """the reference's tables as numpy arrays + the same as the C struct"""
    g = fixture()
    t = np.zeros(1, B.BOOL_TABLES_DTYPE)
    t["coef_probs"][0], t["pareto"][0], t["cat_probs"][0] = g["coef_probs"], g["pareto"], g["cat_probs"]
    return dict(coef_probs=g["coef_probs"], pareto=g["pareto"], cat_probs=g["cat_probs"]), t


def fixture_token_streams():
    """the three token streams of tokens_reference.npz as uint32 records, in that fixture's (the entropy coder's) block order"""
    import tokenize_model as TM
    _, _, pics = TM.fixture_pictures()
    out = []
    for p in pics:
        tok, extra, row = (p["tokens"][:, k].astype(np.uint32) for k in range(3))
        out.append(((extra & 0xFFFF) << 16) | (row << 4) | tok)
    return out


def segments_array(segments):
    return np.array([tuple(s) for s in segments], B.BOOL_SEGMENT_DTYPE).reshape(-1)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def product_call(fn, tokens=None, bools=None, segments=None, capacity=None, ctx=None, tabs=None):
    """svt_hip_boolcode_host (ctx None; tabs = the C tables) or svt_hip_boolcode: (bytes, size, guard)"""
    tokens = np.zeros(0, np.uint32) if tokens is None else np.ascontiguousarray(tokens, np.uint32)
    bools = np.zeros(0, np.uint16) if bools is None else np.ascontiguousarray(bools, np.uint16)
    segs = None if segments is None else segments_array(segments)
    worst = len(bools) + B.BOOL_MAX_PER_TOKEN * len(tokens) if segments is None else sum(c * (1 if k else B.BOOL_MAX_PER_TOKEN) for _, c, k in segments)
    cap = int(B.load().svt_hip_boolcode_capacity(worst)) if capacity is None else capacity
    buf = np.full(cap + 64, 0xA5, np.uint8)
    size = C.c_uint32(0x77777777)
    args = (_vp(tokens), len(tokens), _vp(bools), len(bools), segs.ctypes.data_as(C.c_void_p) if segs is not None else None,
            0 if segs is None else len(segs), buf.ctypes.data_as(C.c_void_p), cap, C.byref(size))
    rc = fn(tabs.ctypes.data_as(C.c_void_p), *args) if ctx is None else fn(ctx, *args)
    assert rc == 0, rc
    return bytes(buf[:min(size.value, cap)]), size.value, buf[cap:]


def host_code(tokens=None, bools=None, segments=None, capacity=None):
    return product_call(B.load().svt_hip_boolcode_host, tokens, bools, segments, capacity, tabs=tables()[1])

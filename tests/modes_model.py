"""Python model of the key-frame mode-info syntax, written independently of the C text (csrc/modeinfo_core.h): a plain serial walk
-- SBs in raster order, the quad-tree depth first -- that carries above_seg_context / left_seg_context arrays and above / left block
pointers the way the reference's entropy coding does, and walks the partition tree and the intra mode tree as the VP9 specification
prints them.  It does NOT read a context from the neighbouring grid records: that derivation is what it checks.  Also here: the seeded
pictures of tests/golden/modes_reference.npz, a leaf's token runs from the tokeniser's offsets, and ctypes wrappers of the host form."""
import ctypes as C
import os

import numpy as np

import boolcode_model as BM
import svt_testlib as T
import tokenize_model as TM

B = T.B
GOLD = os.path.join(T.GOLDEN_DIR, "modes_reference.npz")
LEAF_TYPES = (0, 3, 6, 9, 12)                  # sb_type of the square sizes; 0 = an 8x8 unit of four 4x4 blocks
UNITS = {0: 1, 3: 1, 6: 2, 9: 4, 12: 8}        # side in 8x8 units
TX = {0: 0, 3: 1, 6: 2, 9: 3, 12: 3}
SEG_CONTEXT = {0: 15, 3: 14, 6: 12, 9: 8, 12: 0}   # partition_context_lookup of the square sizes
# trees as printed (leaves: -value)
PARTITION_TREE = (0, 2, -1, 4, -2, -3)         # NONE 0, HORZ 1, VERT 2, SPLIT 3
INTRA_MODE_TREE = (0, 2, -9, 4, -1, 6, 8, 12, -2, 10, -4, -5, -3, 14, -8, 16, -6, -7)
# (name, width, height, kind, seed): kind = the one leaf type of the picture, or "random"
PICTURES = tuple((f"sb64_leaf{t}", 64, 64, t, 10 + t) for t in LEAF_TYPES) + (("edge_72x40_a", 72, 40, "random", 21), ("edge_72x40_b", 72, 40, "random", 22),
                                                                                ("sbs_136x136_a", 136, 136, "random", 31), ("sbs_136x136_b", 136, 136, "random", 32))


def rec(bit, prob):
    return (int(bit) << 8) | int(prob)


def tree_path(tree, leaf):
    """[(node, bit)] from the root to the leaf `leaf`; node = index into the probabilities"""
    def walk(i, path):
        for bit in (0, 1):
            nxt = tree[i + bit]
            here = path + [(i >> 1, bit)]
            if nxt == -leaf and (nxt != 0 or (i, bit) == (0, 0)):
                return here
            if nxt > 0:
                r = walk(nxt, here)
                if r:
                    return r
        return None
    return walk(0, [])


def tree_bools(tree, leaf, probs):
    return [rec(bit, probs[node]) for node, bit in tree_path(tree, leaf)]


# ---------------------------------------------------------------------------------------------------
# the seeded pictures
# ---------------------------------------------------------------------------------------------------
def _zorder(x, y):
    v = 0
    for b in range(4):
        v |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
    return v


def eob_offsets(W, H):
    w4, h4 = W // 4, H // 4
    return (0, w4 * h4, w4 * h4 + (w4 // 2) * (h4 // 2), w4 * h4 + 2 * (w4 // 2) * (h4 // 2))


def leaf_tx_blocks(t, r, c):
    """transform blocks of the leaf of type t at unit (r, c): [(plane, x4, y4, tx_size, block index)] in the leaf's coding order"""
    ts = TX[t]
    out = []
    if t in (0, 12):
        out += [(0, 2 * c + ((i & 1) << ts), 2 * r + ((i >> 1) << ts), ts, i) for i in range(4)]
    else:
        out.append((0, 2 * c, 2 * r, ts, 0))
    tu = {0: 0, 3: 0, 6: 1, 9: 2, 12: 3}[t]
    return out + [(1, c, r, tu, 0), (2, c, r, tu, 0)]


def make_picture(W, H, kind, seed):
    """(lf_mi, qcoeff, eob_map): a quad-tree of square leaves with random modes and skip flags, sparse random coefficients in the coded leaves"""
    rng = np.random.default_rng(seed)
    mi_rows, mi_cols = H // 8, W // 8
    lf = np.zeros((mi_rows, mi_cols), B.LF_MODE_INFO_DTYPE)
    q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
    eoff = eob_offsets(W, H)
    emap = np.zeros(eoff[3], np.uint16)
    offs, scans = TM.scan_tables()
    sb_cols = (W + 63) // 64

    def leaf(r, c, t):
        n = UNITS[t]
        modes = [int(m) for m in rng.integers(0, 10, 4)]
        uv, skip = int(rng.integers(0, 10)), int(rng.random() < 0.4)
        lf[r:r + n, c:c + n]["sb_type"], lf[r:r + n, c:c + n]["tx_size"], lf[r:r + n, c:c + n]["skip"], lf[r:r + n, c:c + n]["filter_level"] = t, TX[t], skip, 12
        pad = (modes[2] | modes[3] << 4, modes[0] | modes[1] << 4, uv) if t == 0 else (0, modes[0], uv)
        lf[r:r + n, c:c + n]["pad"] = pad
        if skip:
            return
        blocks = leaf_tx_blocks(t, r, c)
        eobs = [0 if rng.random() < 0.3 else int(min(16 << (2 * ts), 1 + rng.geometric(0.25))) for _, _, _, ts, _ in blocks]
        if not any(eobs):
            eobs[int(rng.integers(0, len(eobs)))] = 1
        for (plane, x4, y4, ts, i), eob in zip(blocks, eobs):
            u = 8 if plane else 16
            tt = TM.INTRA_TX_TYPE[modes[i] if t == 0 else modes[0]] if plane == 0 and ts < 3 else 0
            scan = scans[offs[(ts, tt)]:offs[(ts, tt)] + (16 << (2 * ts))]
            sb = (y4 // u) * sb_cols + x4 // u
            base = sb * B.SB_COEFFS + (0, 4096, 5120)[plane] + _zorder(x4 % u, y4 % u) * 16
            for k in range(eob):
                v = int(rng.choice((1, 1, 1, 2, 2, 3, 4, 5, 9, 20, 70, 300))) if k == eob - 1 or rng.random() < 0.7 else 0
                q[base + int(scan[k])] = -v if rng.random() < 0.5 else v
            emap[eoff[plane] + y4 * (W // 8 if plane else W // 4) + x4] = eob

    def node(r, c, L):
        if r >= mi_rows or c >= mi_cols:
            return
        s = 1 << L
        inside = r + s <= mi_rows and c + s <= mi_cols
        if kind != "random":
            here = inside and UNITS[kind] == s
        else:
            here = inside and (L == 0 or rng.random() < (0.2, 0.3, 0.4, 0.0)[3 - L] + (0.15 if L == 3 else 0))
        if here:
            t = kind if kind != "random" else ((0 if rng.random() < 0.45 else 3) if L == 0 else (6, 9, 12)[L - 1])
            return leaf(r, c, t)
        for dr, dc in ((0, 0), (0, s // 2), (s // 2, 0), (s // 2, s // 2)):
            node(r + dr, c + dc, L - 1)

    for r in range(0, mi_rows, 8):
        for c in range(0, mi_cols, 8):
            node(r, c, 3)
    return lf, q, emap


# ---------------------------------------------------------------------------------------------------
# the serial model
# ---------------------------------------------------------------------------------------------------
class Block:
    """one ModeInfo: what every unit of a leaf points at"""

    def __init__(self, r):
        self.sb_type, self.skip = int(r["sb_type"]), int(r["skip"])
        p = [int(v) for v in r["pad"]]
        self.bmi = [p[1] & 15, p[1] >> 4, p[0] & 15, p[0] >> 4] if self.sb_type == 0 else [p[1]] * 4
        self.mode = self.bmi[3]            # the last quadrant's for four 4x4 blocks
        self.uv_mode = p[2]

    def y_mode(self, k):
        return self.bmi[k]


def serial_walk(lf_mi, W, H, tabs, cover=None):
    """(bool records of the picture in coding order, leaves [(r, c, sb_type, first bool, bools)] in coding order).  cover (a dict) receives
    the partition contexts coded with at least one bool, the skip contexts, and the (above, left) neighbour classes of the luma modes"""
    mi_rows, mi_cols = H // 8, W // 8
    vis = [[None] * mi_cols for _ in range(mi_rows)]
    for r in range(mi_rows):
        for c in range(mi_cols):
            n = UNITS[int(lf_mi[r, c]["sb_type"])]
            r0, c0 = r - r % n, c - c % n
            if vis[r0][c0] is None:
                vis[r0][c0] = Block(lf_mi[r0, c0])
            vis[r][c] = vis[r0][c0]
    above_seg = [0] * (((mi_cols + 7) // 8) * 8)      # cleared once per picture
    left_seg = [0] * 8
    out, leaves = [], []
    cov = dict(partition=set(), skip=set(), pairs=set()) if cover is None else cover
    for k in ("partition", "skip", "pairs"):
        cov.setdefault(k, set())
    klass = lambda m: "missing" if m is None else "4x4" if m.sb_type == 0 else "larger"      # noqa: E731

    first = {}

    def node(r, c, L):
        if r >= mi_rows or c >= mi_cols:
            return
        s, hbs = 1 << L, (1 << L) >> 1
        mi = vis[r][c]
        first.setdefault((r, c), len(out))     # the nodes of one origin are coded back to back, outermost first
        split = UNITS[mi.sb_type] < s or (L == 0 and mi.sb_type == 0)
        ctx = 4 * L + 2 * ((left_seg[r & 7] >> L) & 1) + ((above_seg[c] >> L) & 1)
        probs = tabs["kf_partition_probs"][ctx]
        has_rows, has_cols = r + hbs < mi_rows, c + hbs < mi_cols
        start = len(out)
        if has_rows and has_cols:
            out.extend(tree_bools(PARTITION_TREE, 3 if split else 0, probs))
        elif has_cols:
            assert split
            out.append(rec(1, probs[1]))
        elif has_rows:
            assert split
            out.append(rec(1, probs[2]))
        if len(out) > start:
            cov["partition"].add(ctx)
        if split and L > 0:
            for dr, dc in ((0, 0), (0, hbs), (hbs, 0), (hbs, hbs)):
                node(r + dr, c + dc, L - 1)
            return
        above, left = (vis[r - 1][c] if r > 0 else None), (vis[r][c - 1] if c > 0 else None)
        sctx = (above.skip if above else 0) + (left.skip if left else 0)
        cov["skip"].add(sctx)
        out.append(rec(mi.skip, tabs["skip_probs"][sctx]))
        for b in (range(4) if mi.sb_type == 0 else (0,)):
            a = (above.y_mode(b + 2) if above else 0) if b < 2 else mi.bmi[b - 2]
            l = (left.y_mode(b + 1) if left else 0) if b % 2 == 0 else mi.bmi[b - 1]
            if b == 0:
                cov["pairs"].add((klass(above), klass(left)))
            out.extend(tree_bools(INTRA_MODE_TREE, mi.bmi[b], tabs["kf_y_mode_prob"][a][l]))
        out.extend(tree_bools(INTRA_MODE_TREE, mi.uv_mode, tabs["kf_uv_mode_prob"][mi.mode]))
        leaves.append((r, c, mi.sb_type, first[(r, c)], len(out) - first[(r, c)]))
        # update_partition_context over the leaf's extent
        for i in range(s):
            above_seg[c + i] = SEG_CONTEXT[mi.sb_type]
            left_seg[(r + i) & 7] = SEG_CONTEXT[mi.sb_type]

    for r in range(0, mi_rows, 8):
        left_seg[:] = [0] * 8                       # cleared at the first SB of every SB row
        for c in range(0, mi_cols, 8):
            node(r, c, 3)
    return np.array(out, np.uint16), leaves


def leaf_runs(lf_mi, tok_off, eob_map, W, H):
    """[mi_rows][mi_cols][3][first, count] (int32): the token runs of the leaf whose origin the unit is, from the tokeniser's offsets: every
    transform block that starts inside the leaf's area of a plane, in offset order, which must be one contiguous run"""
    mi_rows, mi_cols = H // 8, W // 8
    eoff = eob_offsets(W, H)
    runs = np.zeros((mi_rows, mi_cols, 3, 2), np.int32)
    for r in range(mi_rows):
        for c in range(mi_cols):
            t = int(lf_mi[r, c]["sb_type"])
            n = UNITS[t]
            if r % n or c % n or int(lf_mi[r, c]["skip"]):
                continue
            for plane in range(3):
                pw4 = W // 8 if plane else W // 4
                side, x0, y0 = (n, c, r) if plane else (2 * n, 2 * c, 2 * r)
                ts = {0: 0, 3: 0, 6: 1, 9: 2, 12: 3}[t] if plane else TX[t]
                blocks = []
                for y4 in range(y0, y0 + side):
                    for x4 in range(x0, x0 + side):
                        off = int(tok_off[eoff[plane] + y4 * pw4 + x4])
                        if off != TM.NO_OFFSET:
                            e, full = int(eob_map[eoff[plane] + y4 * pw4 + x4]), 16 << (2 * ts)
                            blocks.append((off, min(e, full) + (e < full)))
                blocks.sort()
                assert blocks and all(a[0] + a[1] == b[0] for a, b in zip(blocks[:-1], blocks[1:])), (r, c, plane)
                runs[r, c, plane] = blocks[0][0], sum(b[1] for b in blocks)
    return runs


def coding_order_segments(leaves, runs):
    """the tile as a segment list built from the serial walk: per leaf its bools, then its Y, Cb, Cr runs"""
    segs = []
    for r, c, _, pos, n in leaves:
        segs.append((pos, n, 1))
        segs += [(int(runs[r, c, p, 0]), int(runs[r, c, p, 1]), 0) for p in range(3) if runs[r, c, p, 1]]
    return segs


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
    """the reference's four mode tables as numpy arrays + the same as the C struct"""
    g = fixture()
    names = ("kf_y_mode_prob", "kf_uv_mode_prob", "kf_partition_probs", "skip_probs")
    t = np.zeros(1, B.MODES_TABLES_DTYPE)
    for n in names:
        t[n][0] = g[n]
    return {n: g[n] for n in names}, t


_pic_cache = {}


def fixture_picture(name):
    """dict(W, H, lf_mi, qcoeff, eob_map, tile bytes, mode-info bytes) of one picture of the fixture"""
    if name not in _pic_cache:
        g = fixture()
        W, H = (int(v) for v in g[f"size|{name}"])
        lf = g[f"lf_mi|{name}"].view(B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8)
        _pic_cache[name] = dict(W=W, H=H, lf_mi=lf, qcoeff=g[f"qcoeff|{name}"], eob_map=g[f"eob_map|{name}"], tile=bytes(g[f"tile_bytes|{name}"]),
                                modes=bytes(g[f"modes_bytes|{name}"]))
    return _pic_cache[name]


NAMES = [p[0] for p in PICTURES]
_tok_cache = {}


def host_tokens(name):
    """svt_hip_tokenize_picture on a fixture picture (shared, left unchanged)"""
    if name not in _tok_cache:
        p = fixture_picture(name)
        _tok_cache[name] = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], counts=False)
    return _tok_cache[name]


def host_modes(lf_mi, eob_map, tok_off, W, H, capacity=None, tabs=None):
    """svt_hip_modes_kf_picture -> dict(rc, bools[:min(n, capacity)], n_bools, segments, guard)"""
    lib = B.load()
    cap = int(lib.svt_hip_modes_bools_capacity(W, H)) if capacity is None else capacity
    n_seg = int(lib.svt_hip_modes_segments(W, H))
    mi = np.ascontiguousarray(lf_mi)
    em, to = np.ascontiguousarray(eob_map, np.uint16), np.ascontiguousarray(tok_off, np.uint32)
    bools = np.full(cap + 64, 0xA5A5, np.uint16)
    segs = np.full((n_seg + 8) * 3, 0x5A5A5A5A, np.uint32)
    n = np.full(1, 0x77777777, np.uint32)
    p = B.ModesPicture()
    p.d_lf_mi, p.d_eob_map, p.d_tok_off, p.d_bools, p.d_segments, p.d_n_bools, p.capacity = (mi.ctypes.data, em.ctypes.data, to.ctypes.data, bools.ctypes.data,
                                                                                            segs.ctypes.data, n.ctypes.data, cap)
    t = tables()[1] if tabs is None else tabs
    rc = lib.svt_hip_modes_kf_picture(t.ctypes.data_as(C.c_void_p), C.byref(p), W, H, mi.shape[1])
    total = int(n[0])
    got = bools[:min(total, cap)].copy() if total != B.MODES_BAD_GRID else np.zeros(0, np.uint16)
    return dict(rc=rc, bools=got, n_bools=total, segments=segs[:3 * n_seg].view(B.BOOL_SEGMENT_DTYPE).copy(), guard=bools[cap:], seg_guard=segs[3 * n_seg:])


def host_chain(name):
    """host tokeniser -> host mode-info stage -> host bool coder on a fixture picture: (tile bytes, mode-info-only bytes, modes result)"""
    p, tok = fixture_picture(name), host_tokens(name)
    m = host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], p["W"], p["H"])
    assert m["rc"] == 0
    segs = [tuple(int(v) for v in s) for s in m["segments"]]
    tile = BM.host_code(tokens=tok["tokens"], bools=m["bools"], segments=segs)[0]
    only = BM.host_code(bools=m["bools"], segments=[s for s in segs if s[2] == 1])[0]
    return tile, only, m


# ---------------------------------------------------------------------------------------------------
# pictures past the first pass of the scans, and at the ceilings of the staging arrays (regenerated from seeds, shared by the CPU and
# the GPU tests of one process, left unchanged)
# ---------------------------------------------------------------------------------------------------
# (name, width, height, kind, seed): 17 x 17 = 289 SBs (odd, more than 256, partial SBs on both edges); the all-4x4 one has more than
# 256 x 1024 tokens + bools, the bool coder's items
BIG = (("big_random", 1080, 1080, "random", 43), ("big_4x4", 1080, 1080, 0, 44))
_big_cache = {}


def big_pictures():
    """[dict(name, W, H, lf_mi, qcoeff, eob_map)] of BIG"""
    for name, W, H, kind, seed in BIG:
        if name not in _big_cache:
            lf, q, emap = make_picture(W, H, kind, seed)
            _big_cache[name] = dict(name=name, W=W, H=H, lf_mi=lf, qcoeff=q, eob_map=emap)
    return [_big_cache[b[0]] for b in BIG]


def big_host(name):
    """the host forms on a picture of big_pictures(): dict(tok, modes, segs, tile) -- computed once"""
    p = next(p for p in big_pictures() if p["name"] == name)
    if "host" not in p:
        tok = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"])
        m = host_modes(p["lf_mi"], p["eob_map"], tok["tok_off"], p["W"], p["H"])
        assert m["rc"] == 0 and m["n_bools"] != B.MODES_BAD_GRID
        seg = m["segments"]
        segs = list(zip(seg["first"].tolist(), seg["count"].tolist(), seg["kind"].tolist()))
        p["host"] = dict(tok=tok, modes=m, segs=segs, tile=BM.host_code(tokens=tok["tokens"], bools=m["bools"], segments=segs)[0])
    return p["host"]


DENSE_VALUES = (1, 2, 3, 4, 5, 9, 20, 67, 300)      # every class of energy, CAT6 among them
_dense_cache = {}


def dense_picture(W, H, leaf_type, seed, short=False, ones=False, values=DENSE_VALUES):
    """(lf_mi, qcoeff, eob_map) of a picture of leaves of one type in which every unit is coded and every coefficient is non-zero (a
    random value of `values` with a random sign; ones: all 1), eob = n in every transform block: 6144 tokens in every whole SB, and for
    type 0 its 384 transform blocks.  short: every other transform block has eob = n - 1 and a zero at its last scan position -- still n
    records, the last one the EOB token.  W, H: multiples of the leaf's size."""
    key = (W, H, leaf_type, seed, short, ones, tuple(values))
    if key in _dense_cache:
        return _dense_cache[key]
    rng = np.random.default_rng(seed)
    mi_rows, mi_cols, n_u = H // 8, W // 8, UNITS[leaf_type]
    assert mi_rows % n_u == 0 and mi_cols % n_u == 0
    lf = np.zeros((mi_rows, mi_cols), B.LF_MODE_INFO_DTYPE)
    q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
    eoff = eob_offsets(W, H)
    emap = np.zeros(eoff[3], np.uint16)
    offs, scans = TM.scan_tables()
    sb_cols, k = (W + 63) // 64, 0
    lf["sb_type"], lf["tx_size"], lf["filter_level"] = leaf_type, TX[leaf_type], 12
    for r in range(0, mi_rows, n_u):
        for c in range(0, mi_cols, n_u):
            modes = [int(m) for m in rng.integers(0, 10, 4)]
            uv = int(rng.integers(0, 10))
            lf[r:r + n_u, c:c + n_u]["pad"] = (modes[2] | modes[3] << 4, modes[0] | modes[1] << 4, uv) if leaf_type == 0 else (0, modes[0], uv)
            for plane, x4, y4, ts, i in leaf_tx_blocks(leaf_type, r, c):
                n, u = 16 << (2 * ts), 8 if plane else 16
                tt = TM.INTRA_TX_TYPE[modes[i] if leaf_type == 0 else modes[0]] if plane == 0 and ts < 3 else 0
                scan = scans[offs[(ts, tt)]:offs[(ts, tt)] + n].astype(np.int64)
                v = np.ones(n, np.int16) if ones else (rng.choice(values, n) * rng.choice((-1, 1), n)).astype(np.int16)
                eob = n
                if short and k & 1:
                    eob, v[n - 1] = n - 1, 0
                k += 1
                base = ((y4 // u) * sb_cols + x4 // u) * B.SB_COEFFS + (0, 4096, 5120)[plane] + _zorder(x4 % u, y4 % u) * 16
                q[base + scan] = v
                emap[eoff[plane] + y4 * (W // 8 if plane else W // 4) + x4] = eob
    _dense_cache[key] = (lf, q, emap)
    return _dense_cache[key]


# (width, height, leaf type, seed, keyword arguments) of the dense pictures the tests share.  576x64 = 9 SBs: a full run of 8 SBs in one
# workgroup of the tokeniser's emit kernel (49 152 tokens) and a second workgroup; 512x64 = that run alone.  `ones` puts all 32 096
# band-5 luma positions of the run into one bin of the counts (the most a bin can receive: its dword partner, the same row's ZERO
# token, is then empty); `values=(19, 35)` splits the same positions over the two halves of one dword (tokens 8 and 9, one energy class).
DENSE = ((576, 64, 0, 51, {}), (576, 64, 0, 52, dict(short=True)), (576, 64, 12, 53, {}), (576, 64, 12, 54, dict(short=True)),
         (512, 64, 12, 55, dict(ones=True)), (512, 64, 12, 56, dict(values=(19, 35))))

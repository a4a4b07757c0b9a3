"""Python model of the MV-reference derivation (eb_vp9_find_mv_refs of the SVT variant), written independently of the C text
(csrc/mvrefs_core.h): a plain serial restatement over block objects -- every unit of the grid points at its block, as the reference's
mode_info_array does -- with the position table, the two lookup tables, the add / done rule, the restrict flag, the second pass with
its sign inversion and the clamp spelled out.  It keeps no window, packs nothing and finds a block's mode at the block, not at a unit.

Also here: the seeded pictures of tests/golden/mvrefs_reference.npz.  They start from modes_inter_model.make_picture (or, for shapes it
does not draw, from make_grid below) and are then made self-consistent the way an encoder's grids are: the leaves are walked in coding
order, a NEARESTMV / NEARMV / ZEROMV leaf gets the MV the model derives at that point, a NEWMV leaf a random one, and the extension
records get the derived reference MVs and mode contexts.  Variants: the same grid with some leaves' MVs perturbed afterwards, and grids
whose MVs sit at the int16 ceilings.  And ctypes wrappers of the host form."""
import ctypes as C
import os

import numpy as np

import modes_inter_model as IM
import modes_model as MM
import svt_testlib as T
import tokenize_model as TM

B = T.B
GOLD = os.path.join(T.GOLDEN_DIR, "mvrefs_reference.npz")
UNITS, TX = MM.UNITS, MM.TX
NEARESTMV, NEARMV, ZEROMV, NEWMV = IM.NEARESTMV, IM.NEARMV, IM.ZEROMV, IM.NEWMV
# mv_ref_blocks of the square sizes, {row, col} (constants of the format)
POSITIONS = {3: ((-1, 0), (0, -1), (-1, -1), (-2, 0), (0, -2), (-2, -1), (-1, -2), (-2, -2)),
             6: ((-1, 0), (0, -1), (-1, 1), (1, -1), (-1, -1), (-3, 0), (0, -3), (-3, -3)),
             9: ((-1, 1), (1, -1), (-1, 2), (2, -1), (-1, -1), (-3, 0), (0, -3), (-3, -3)),
             12: ((-1, 3), (3, -1), (-1, 4), (4, -1), (-1, -1), (-1, 0), (0, -1), (-1, 6))}
MODE_COUNTER = {NEARESTMV: 0, NEARMV: 0, ZEROMV: 3, NEWMV: 1}        # any intra mode: 9
COUNTER_TO_CONTEXT = (2, 3, 4, 1, 3, None, 0, None, None, 5, 5, None, 5, None, None, None, None, None, 6)
ALL_REFS = 0xE


class Blk:
    """one ModeInfo: what every unit of a block points at"""
    __slots__ = ("r", "c", "t", "n", "inter", "ref", "mv", "mode")

    def __init__(self, r, c, lf, mc, ext):
        self.r, self.c, self.t = r, c, int(lf["sb_type"])
        self.n = UNITS[self.t]
        self.inter = int(lf["is_inter"]) != 0
        f = [int(v) for v in ext["ref_frame"]]
        self.ref = (f[0], f[1] if f[1] > 0 else -1) if self.inter else (0, -1)       # NONE = -1 (and an intra block's second)
        self.mv = [(int(mc["mv_row"][k]), int(mc["mv_col"][k])) for k in range(2)] if self.inter else [(0, 0), (0, 0)]
        self.mode = int(ext["mode"]) if self.inter else 0

    def counter(self):
        return MODE_COUNTER[self.mode] if self.inter else 9


def leaves_of(lf_mi, mi_rows, mi_cols):
    """[(r, c, sb_type)] in coding order: SBs raster, the quad-tree depth first"""
    out = []

    def node(r, c, lv):
        if r >= mi_rows or c >= mi_cols:
            return
        t, s = int(lf_mi[r, c]["sb_type"]), 1 << lv
        if UNITS[t] < s and lv > 0:
            h = s >> 1
            for dr, dc in ((0, 0), (0, h), (h, 0), (h, h)):
                node(r + dr, c + dc, lv - 1)
        else:
            out.append((r, c, t))

    for r in range(0, mi_rows, 8):
        for c in range(0, mi_cols, 8):
            node(r, c, 3)
    return out


def block_grid(pic):
    """(leaves in coding order as Blk, rows of pointers)"""
    mi_rows, mi_cols = pic["H"] // 8, pic["W"] // 8
    grid = [[None] * mi_cols for _ in range(mi_rows)]
    blocks = []
    for r, c, t in leaves_of(pic["lf_mi"], mi_rows, mi_cols):
        b = Blk(r, c, pic["lf_mi"][r, c], pic["mc_mi"][r, c], pic["ext"][r, c])
        blocks.append(b)
        for rr in range(r, r + b.n):
            grid[rr][c:c + b.n] = [b] * b.n
    return blocks, grid


def wrap_neg(v):
    """-v as the reference's build computes it in an int16"""
    return -32768 if v == -32768 else -v


COVER_KEYS = ("supply", "slot1", "dup", "same_mv", "invert", "ret", "clamp", "ctx", "near_inside")


def new_cover():
    return {k: set() for k in COVER_KEYS}


def find_mv_refs(grid, mi_rows, mi_cols, blk, ref, restrict, bias, cov=None):
    """eb_vp9_find_mv_refs of block blk and reference frame ref -> ([mv, mv] clamped, return value, mode context)"""
    cov = new_cover() if cov is None else cov
    r, c, n = blk.r, blk.c, blk.n
    lst, state = [(0, 0), (0, 0)], dict(count=0, done=False)

    def inside(p):
        return 0 <= r + p[0] < mi_rows and 0 <= c + p[1] < mi_cols

    def add(mv, i, where, pas):
        if state["count"]:
            if mv != lst[0]:
                lst[1], state["done"] = mv, True
                cov["slot1"].add(where)
                cov["supply"].add((blk.t, i))
            else:
                cov["dup"].add(pas)
        else:
            lst[0], state["count"] = mv, 1
            cov["supply"].add((blk.t, i))

    counter, any_inside, near = 0, False, 0
    for i, p in enumerate(POSITIONS[blk.t]):
        if not inside(p):
            continue
        cand = grid[r + p[0]][c + p[1]]
        any_inside = True
        if i < 2:
            counter += cand.counter()
            near += 1
        if cand.ref[0] == ref:
            add(cand.mv[0], i, "p1_near" if i < 2 else "p1_far", 1)
        elif cand.ref[1] == ref:
            add(cand.mv[1], i, "p1_near" if i < 2 else "p1_far", 1)
        if state["done"]:
            break
    cov["near_inside"].add(near)
    if not state["done"] and not restrict and any_inside:
        for i, p in enumerate(POSITIONS[blk.t]):
            if not inside(p):
                continue
            cand = grid[r + p[0]][c + p[1]]
            if not cand.inter:
                continue

            def scaled(k):
                flip = bias[cand.ref[k]] != bias[ref]
                cov["invert"].add(int(flip))
                return (wrap_neg(cand.mv[k][0]), wrap_neg(cand.mv[k][1])) if flip else cand.mv[k]
            if cand.ref[0] != ref:
                add(scaled(0), i, "p2_first", 2)
                if state["done"]:
                    break
            if cand.ref[1] > 0 and cand.ref[1] != ref:
                if cand.mv[1] == cand.mv[0]:
                    cov["same_mv"].add(1)
                else:
                    add(scaled(1), i, "p2_second", 2)
                    if state["done"]:
                        break
    ret = 2 if state["done"] else state["count"]
    col_lo, col_hi = -(c * 64) - 128, (mi_cols - n - c) * 64 + 128
    row_lo, row_hi = -(r * 64) - 128, (mi_rows - n - r) * 64 + 128
    for k in range(ret):
        row, col = lst[k]
        for name, hit in (("row_lo", row < row_lo), ("row_hi", row > row_hi), ("col_lo", col < col_lo), ("col_hi", col > col_hi)):
            if hit:
                cov["clamp"].add(name)
        lst[k] = (min(max(row, row_lo), row_hi), min(max(col, col_lo), col_hi))
    ctx = COUNTER_TO_CONTEXT[counter]
    cov["ret"].add((int(bool(restrict)), ret))
    cov["ctx"].add(ctx)
    return lst, ret, ctx


def coverage_complete(cov):
    """what the fixture has to reach, as a list of what is missing"""
    want = dict(supply={(t, i) for t in (3, 6, 9, 12) for i in range(8)}, slot1={"p1_near", "p1_far", "p2_first", "p2_second"}, dup={1, 2}, same_mv={1},
                invert={0, 1}, ret={(f, v) for f in (0, 1) for v in (0, 1, 2)}, clamp={"row_lo", "row_hi", "col_lo", "col_hi"}, ctx=set(range(7)),
                near_inside={0, 1, 2})
    return [(k, sorted(want[k] - set(cov[k]))) for k in want if want[k] - set(cov[k])]


def wanted_mv(mode, lst):
    return lst[0] if mode == NEARESTMV else lst[1] if mode == NEARMV else (0, 0)


def derive_picture(pic, cov=None, ref_mask=ALL_REFS):
    """the stage's outputs as the model states them: dict(cand, ext_out, status)"""
    mi_rows, mi_cols = pic["H"] // 8, pic["W"] // 8
    blocks, grid = block_grid(pic)
    cand = np.zeros((mi_rows, mi_cols), B.MVREF_CAND_DTYPE)
    cand["count"] = 0xFF
    ext_out = np.zeros((mi_rows, mi_cols), B.MI_INTER_EXT_DTYPE)
    ext_out["ref_frame"] = pic["ext"]["ref_frame"]
    contradicting = inter_leaves = 0
    for b in blocks:
        ext_out[b.r, b.c]["mode"] = pic["ext"][b.r, b.c]["mode"]
        if b.t == 0:
            continue
        lists = {}
        for ref in (1, 2, 3):
            lists[ref] = find_mv_refs(grid, mi_rows, mi_cols, b, ref, pic["restrict"], pic["frame"]["sign_bias"], cov)
            if (ref_mask >> ref) & 1:
                lst, ret, ctx = lists[ref]
                k = cand[b.r, b.c]
                k["mv_row"][ref - 1], k["mv_col"][ref - 1] = (lst[0][0], lst[1][0]), (lst[0][1], lst[1][1])
                k["count"][ref - 1] = ret
        cand[b.r, b.c]["mode_context"] = lists[1][2]
        if not b.inter:
            continue
        inter_leaves += 1
        e = ext_out[b.r, b.c]
        e["mode_context"] = lists[1][2]
        bad = False
        for k in range(2 if b.ref[1] > 0 else 1):
            lst = lists[b.ref[k]][0]
            e["ref_mv_row"][k], e["ref_mv_col"][k] = lst[0]
            bad |= b.mode != NEWMV and b.mv[k] != wanted_mv(b.mode, lst)
        contradicting += int(bad)
    return dict(cand=cand, ext_out=ext_out, status=(contradicting, inter_leaves))


# ---------------------------------------------------------------------------------------------------
# the seeded pictures
# ---------------------------------------------------------------------------------------------------
def make_grid(W, H, seed, fr, p_intra, p_leaf):
    """the grids of a picture without coefficients (every leaf skipped): a quad-tree whose node of level lv (3 = 64x64) is a leaf with
    probability p_leaf[lv]; references, modes and MVs as modes_inter_model.make_picture draws them"""
    rng = np.random.default_rng(seed)
    mi_rows, mi_cols = H // 8, W // 8
    lf = np.zeros((mi_rows, mi_cols), B.LF_MODE_INFO_DTYPE)
    mc = np.zeros((mi_rows, mi_cols), B.MC_MODE_INFO_DTYPE)
    ext = np.zeros((mi_rows, mi_cols), B.MI_INTER_EXT_DTYPE)
    mc["ref_list"] = -1
    fix_idx = fr["sign_bias"][fr["comp_fixed_ref"]]

    def leaf(r, c, t):
        n = UNITS[t]
        area = (slice(r, r + n), slice(c, c + n))
        intra = rng.random() < p_intra
        lf[area]["sb_type"], lf[area]["tx_size"], lf[area]["skip"], lf[area]["filter_level"], lf[area]["is_inter"] = t, TX[t], 1, 12, 0 if intra else 1
        mc[area]["bw8"] = mc[area]["bh8"] = n
        if intra:
            lf[area]["pad"] = (0, int(rng.integers(0, 10)), int(rng.integers(0, 10)))
            return
        comp = fr["reference_mode"] == IM.SELECT and rng.random() < 0.45
        refs = [int(rng.integers(1, 4)), 0]
        if comp:
            refs[fix_idx], refs[1 - fix_idx] = fr["comp_fixed_ref"], fr["comp_var_ref"][int(rng.integers(0, 2))]
        m = np.zeros((), B.MC_MODE_INFO_DTYPE)
        m["ref_list"], m["bw8"], m["bh8"] = (0 if refs[0] < IM.ALTREF else 1, 1 if comp else -1), n, n
        mc[area] = m
        ext[area]["ref_frame"] = refs
        ext[r, c]["mode"] = int(rng.choice((NEARESTMV, NEARMV, ZEROMV, NEWMV, NEWMV, NEWMV)))

    def node(r, c, lv):
        if r >= mi_rows or c >= mi_cols:
            return
        s = 1 << lv
        if r + s <= mi_rows and c + s <= mi_cols and (lv == 0 or rng.random() < p_leaf[lv]):
            return leaf(r, c, (3, 6, 9, 12)[lv])
        for dr, dc in ((0, 0), (0, s // 2), (s // 2, 0), (s // 2, s // 2)):
            node(r + dr, c + dc, lv - 1)

    for r in range(0, mi_rows, 8):
        for c in range(0, mi_cols, 8):
            node(r, c, 3)
    q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
    return dict(W=W, H=H, frame=fr, lf_mi=lf, mc_mi=mc, ext=ext, qcoeff=q, eob_map=np.zeros(MM.eob_offsets(W, H)[3], np.uint16))


CEILINGS = ((32767, 32767), (-32768, -32768), (32767, -32768), (-32768, 32767), (-32768, 0), (0, 32767), (32766, -32767), (2, -2))


def make_consistent(pic, restrict, seed, ceilings=False):
    """rewrites pic's MVs and extension records in place (see the module's head); ceilings: a NEWMV leaf's MVs come from CEILINGS"""
    rng = np.random.default_rng(seed)
    pic["restrict"] = restrict
    mi_rows, mi_cols = pic["H"] // 8, pic["W"] // 8
    blocks, grid = block_grid(pic)
    bias = pic["frame"]["sign_bias"]
    for k in ("ref_mv_row", "ref_mv_col", "mode_context"):
        pic["ext"][k] = 0
    for b in blocks:
        if not b.inter:
            continue
        n_ref = 2 if b.ref[1] > 0 else 1
        same = n_ref == 2 and rng.random() < 0.2         # a compound block whose two MVs are equal
        for k in range(n_ref):
            lst, _, ctx = find_mv_refs(grid, mi_rows, mi_cols, b, b.ref[k], restrict, bias)
            if b.mode != NEWMV:
                b.mv[k] = wanted_mv(b.mode, lst)
            elif ceilings:
                b.mv[k] = CEILINGS[int(rng.integers(0, len(CEILINGS)))]
            elif same and k == 1 and all(abs(b.mv[0][i] - lst[0][i]) <= 16382 for i in (0, 1)):
                b.mv[1] = b.mv[0]
            else:                                        # the reference MV plus an even difference drawn by joint and class, inside int16
                joint = int(rng.integers(0, 4))
                mv = []
                for i, bit in ((0, 2), (1, 1)):
                    d = IM.mv_component(rng, int(rng.integers(0, 11)), True) if joint & bit else 0
                    mv.append(lst[0][i] + d if -32768 <= lst[0][i] + d <= 32767 else lst[0][i] - d)
                b.mv[k] = tuple(mv)
            e = pic["ext"][b.r, b.c]
            e["ref_mv_row"][k], e["ref_mv_col"][k] = lst[0]
            e["mode_context"] = ctx
        area = (slice(b.r, b.r + b.n), slice(b.c, b.c + b.n))
        for k in range(n_ref):
            pic["mc_mi"]["mv_row"][area + (k,)], pic["mc_mi"]["mv_col"][area + (k,)] = b.mv[k]
    return pic


def perturb(pic, count, seed):
    """a copy of a consistent picture with the MVs of `count` NEARESTMV / NEARMV / ZEROMV leaves changed afterwards"""
    rng = np.random.default_rng(seed)
    out = dict(pic, mc_mi=pic["mc_mi"].copy())
    blocks, _ = block_grid(pic)
    pool = [b for b in blocks if b.inter and b.mode != NEWMV]
    assert pool
    for i in rng.choice(len(pool), min(count, len(pool)), replace=False):
        b = pool[int(i)]
        area = (slice(b.r, b.r + b.n), slice(b.c, b.c + b.n), int(rng.integers(0, 2 if b.ref[1] > 0 else 1)))
        out["mc_mi"]["mv_row" if rng.random() < 0.5 else "mv_col"][area] += 2 * int(rng.integers(1, 9))
    return out


ZERO_BIAS, ALT_BIAS = (0, 0, 0, 0), (0, 0, 0, 1)
# the four settings every shape comes with: restrict flag, sign biases, reference mode -- each pair of the three factors in all four combinations
SETTINGS = (("a", 0, ZERO_BIAS, IM.SINGLE), ("b", 0, ALT_BIAS, IM.SELECT), ("c", 1, ALT_BIAS, IM.SINGLE), ("d", 1, ZERO_BIAS, IM.SELECT))
# (name, width, height, kind, seed, share of intra leaves): kind as modes_inter_model.make_picture takes it
SHAPES = (("sb64_leaf3", 64, 64, 3, 203, 0.1), ("sb64_leaf6", 64, 64, 6, 206, 0.1), ("sb64_leaf9", 64, 64, 9, 209, 0.0), ("sb64_leaf12", 64, 64, 12, 212, 0.0),
          ("edge_72x40", 72, 40, "random", 221, 0.15), ("mix_136x136", 136, 136, "random", 231, 0.3), ("wide_8192x64", 8192, 64, "random", 241, 0.1))
BIG_LEAVES = {3: 0.5, 2: 0.5, 1: 0.5}


def build_pictures():
    """{name: picture} of the fixture, from seeds.  `consistent` pictures have a reference tile."""
    out = {}
    for name, W, H, kind, seed, p_intra in SHAPES:
        for tag, restrict, bias, mode in SETTINGS:
            fr = IM.frame(reference_mode=mode, sign_bias=bias)
            p = make_consistent(IM.make_picture(W, H, kind, seed + ord(tag), fr, p_intra), restrict, seed)
            out[f"{name}_{tag}"] = dict(p, consistent=1)
    # 64x64 leaves below split SBs, which the trees above hardly draw
    for tag, restrict, bias, mode in SETTINGS:
        fr = IM.frame(reference_mode=mode, sign_bias=bias)
        out[f"big_192x192_{tag}"] = dict(make_consistent(make_grid(192, 192, 250 + ord(tag), fr, 0.1, BIG_LEAVES), restrict, 251), consistent=1)
    # MVs of 32767 and -32768 next to a sign inversion; on the wide picture the column clamp leaves them alone
    fr = IM.frame(reference_mode=IM.SELECT, sign_bias=ALT_BIAS)
    out["ceil_64x64"] = dict(make_consistent(make_grid(64, 64, 261, fr, 0.1, {3: 0.0, 2: 0.0, 1: 0.0}), 0, 262, ceilings=True), consistent=0)
    out["ceil_136x136"] = dict(make_consistent(make_grid(136, 136, 263, fr, 0.15, {3: 0.2, 2: 0.3, 1: 0.4}), 0, 264, ceilings=True), consistent=0)
    out["ceil_8192x64"] = dict(make_consistent(make_grid(8192, 64, 265, IM.frame(sign_bias=ALT_BIAS), 0.1, {3: 0.3, 2: 0.6, 1: 0.6}), 0, 266, ceilings=True), consistent=0)
    out["pert_72x40"] = dict(perturb(out["edge_72x40_b"], 4, 271), consistent=0)
    out["pert_136x136"] = dict(perturb(out["mix_136x136_b"], 9, 272), consistent=0)
    return out


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


def names(consistent=None):
    g = fixture()
    return [str(n) for n in g["names"] if consistent is None or int(g[f"params|{n}"][6]) == consistent]


_pic_cache = {}


def fixture_picture(name):
    """dict(W, H, frame, restrict, consistent, lf_mi, mc_mi, ext, cand, ext_out, status[, qcoeff, eob_map, tile]) of one picture of the
    fixture; cand, ext_out and status are what the reference derived (all three reference frames)"""
    if name not in _pic_cache:
        g = fixture()
        W, H = (int(v) for v in g[f"size|{name}"])
        pp = [int(v) for v in g[f"params|{name}"]]
        shape = (H // 8, W // 8)
        p = dict(W=W, H=H, frame=IM.frame(reference_mode=pp[5], sign_bias=tuple(pp[1:5])), restrict=pp[0], consistent=pp[6],
                 lf_mi=g[f"lf_mi|{name}"].view(B.LF_MODE_INFO_DTYPE).reshape(shape), mc_mi=g[f"mc_mi|{name}"].view(B.MC_MODE_INFO_DTYPE).reshape(shape),
                 ext=g[f"ext|{name}"].view(B.MI_INTER_EXT_DTYPE).reshape(shape), cand=g[f"cand|{name}"].view(B.MVREF_CAND_DTYPE).reshape(shape),
                 ext_out=g[f"ext_out|{name}"].view(B.MI_INTER_EXT_DTYPE).reshape(shape), status=tuple(int(v) for v in g[f"status|{name}"]))
        if p["consistent"]:
            q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
            q[g[f"q_idx|{name}"]] = g[f"q_val|{name}"]
            p.update(qcoeff=q, eob_map=g[f"eob_map|{name}"], tile=bytes(g[f"tile_bytes|{name}"]))
        _pic_cache[name] = p
    return _pic_cache[name]


def mask_cand(cand, ref_mask):
    """the golden candidate records (all three frames) as the stage writes them under ref_mask"""
    out = cand.copy()
    for ref in (1, 2, 3):
        if not (ref_mask >> ref) & 1:
            out["mv_row"][:, :, ref - 1] = 0
            out["mv_col"][:, :, ref - 1] = 0
            out["count"][:, :, ref - 1] = 0xFF
    return out


def fill_picture(p, pic, ref_mask, restrict=None, bias=None):
    p.ref_mask = ref_mask
    p.restrict_ref_mvs = pic["restrict"] if restrict is None else restrict
    for i, v in enumerate(pic["frame"]["sign_bias"] if bias is None else bias):
        p.ref_frame_sign_bias[i] = v


GUARD = 64


def host_mvrefs(pic, ref_mask=ALL_REFS, want_ext=True, want_cand=True, restrict=None, bias=None):
    """svt_hip_mvrefs_picture -> dict(rc, ext_out, cand, status, guards intact); the grids may be wider than the picture (their common
    row length is the mi_stride); the outputs are returned cut to the picture"""
    lib = B.load()
    W, H = pic["W"], pic["H"]
    mi, mc, ex = np.ascontiguousarray(pic["lf_mi"]), np.ascontiguousarray(pic["mc_mi"]), np.ascontiguousarray(pic["ext"])
    assert mi.shape == mc.shape == ex.shape
    rows, stride = mi.shape
    eo = np.full(rows * stride * 12 + GUARD, 0xA5, np.uint8)
    ca = np.full(rows * stride * 32 + GUARD, 0x5A, np.uint8)
    st = np.full(2 + 4, 0x77777777, np.uint32)
    p = B.MvrefsPicture()
    p.d_lf_mi, p.d_mc_mi, p.d_ext, p.d_status = mi.ctypes.data, mc.ctypes.data, ex.ctypes.data, st.ctypes.data
    p.d_ext_out, p.d_cand = eo.ctypes.data if want_ext else None, ca.ctypes.data if want_cand else None
    fill_picture(p, pic, ref_mask, restrict, bias)
    rc = lib.svt_hip_mvrefs_picture(C.byref(p), W, H, stride)
    return dict(rc=rc, ext_out=eo[:-GUARD].view(B.MI_INTER_EXT_DTYPE).reshape(rows, stride)[:, :W // 8].copy(), raw_ext=eo, raw_cand=ca,
                cand=ca[:-GUARD].view(B.MVREF_CAND_DTYPE).reshape(rows, stride)[:, :W // 8].copy(), status=(int(st[0]), int(st[1])),
                guards=bool((eo[-GUARD:] == 0xA5).all() and (ca[-GUARD:] == 0x5A).all() and (st[2:] == 0x77777777).all()))


def with_stride(pic, extra, seed):
    """the picture on grids of mi_cols + extra records a row, random bytes behind every row"""
    out = dict(pic)
    for k in ("lf_mi", "mc_mi", "ext"):
        out[k] = TM.with_stride(pic[k], extra, seed)
    return out


# 17 x 17 = 289 SBs: more than one entry per thread of the status kernel and threads with none; regenerated from its seed
_big = None


def big_picture():
    global _big
    if _big is None:
        fr = IM.frame(reference_mode=IM.SELECT, sign_bias=ALT_BIAS)
        _big = make_consistent(make_grid(1080, 1080, 281, fr, 0.2, {3: 0.15, 2: 0.3, 1: 0.4}), 0, 282)
        _big = perturb(_big, 40, 283)
        _big["host"] = host_mvrefs(_big)
    return _big

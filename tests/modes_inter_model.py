"""Python model of the mode-info syntax of inter pictures, written independently of the C text (csrc/modeinfo_inter_core.h): a plain
serial walk -- SBs in raster order, the quad-tree depth first -- that carries above / left partition-context arrays and above / left
block-pointer arrays, updated after every leaf the way a serial coder updates them, and walks the trees as the VP9 specification
prints them.  It does NOT read a context from the neighbouring grid records: that derivation is what it checks.  Also here: the seeded
pictures of tests/golden/modes_inter_reference.npz and ctypes wrappers of the host form."""
import ctypes as C
import os

import numpy as np

import boolcode_model as BM
import modes_model as MM
import svt_testlib as T
import tokenize_model as TM

B = T.B
GOLD = os.path.join(T.GOLDEN_DIR, "modes_inter_reference.npz")
UNITS, TX, SEG_CONTEXT = MM.UNITS, MM.TX, MM.SEG_CONTEXT
SIZE_GROUP = {0: 0, 3: 1, 6: 2, 9: 3, 12: 3}
INTRA, LAST, GOLDEN, ALTREF = 0, 1, 2, 3
NEARESTMV, NEARMV, ZEROMV, NEWMV = 10, 11, 12, 13
SINGLE, COMPOUND, SELECT = 0, 1, 2
# trees as printed: an entry is the index of the next pair, or ("leaf", value)
L = lambda v: ("leaf", v)                               # noqa: E731
PARTITION_TREE = (L(0), 2, L(1), 4, L(2), L(3))         # NONE, HORZ, VERT, SPLIT
INTRA_MODE_TREE = (L(0), 2, L(9), 4, L(1), 6, 8, 12, L(2), 10, L(4), L(5), L(3), 14, L(8), 16, L(6), L(7))
INTER_MODE_TREE = (L(ZEROMV), 2, L(NEARESTMV), 4, L(NEARMV), L(NEWMV))
MV_JOINT_TREE = (L(0), 2, L(1), 4, L(2), L(3))          # ZERO, HNZVZ (column only), HZVNZ (row only), HNZVNZ
MV_CLASS_TREE = (L(0), 2, L(1), 4, 6, 8, L(2), L(3), 10, 12, L(4), L(5), L(6), 14, 16, 18, L(7), L(8), L(9), L(10))
MV_FP_TREE = (L(0), 2, L(1), 4, L(2), L(3))
TABLE_SHAPES = (("partition_prob", (16, 3)), ("skip_probs", (3,)), ("intra_inter_prob", (4,)), ("comp_inter_prob", (5,)), ("single_ref_prob", (5, 2)),
                ("comp_ref_prob", (5,)), ("y_mode_prob", (4, 9)), ("uv_mode_prob", (10, 9)), ("inter_mode_probs", (7, 3)), ("nmvc", (69,)))


def frame(reference_mode=SINGLE, allow_hp=0, sign_bias=(0, 0, 0, 0)):
    """the frame parameters; comp_fixed_ref / comp_var_ref as eb_vp9_setup_compound_reference_mode derives them from the sign biases"""
    sb = tuple(sign_bias)
    if sb[LAST] == sb[GOLDEN]:
        fixed, var = ALTREF, (LAST, GOLDEN)
    elif sb[LAST] == sb[ALTREF]:
        fixed, var = GOLDEN, (LAST, ALTREF)
    else:
        fixed, var = LAST, (GOLDEN, ALTREF)
    return dict(reference_mode=reference_mode, allow_hp=allow_hp, sign_bias=sb, comp_fixed_ref=fixed, comp_var_ref=var)


B_PICTURE = dict(reference_mode=SELECT, sign_bias=(0, 0, 0, 1))
# (name, width, height, kind, seed, frame, share of intra leaves): kind = the one leaf type of the picture, or "random"
PICTURES = (("sb64_leaf3", 64, 64, 3, 103, frame(), 0.0), ("sb64_leaf6", 64, 64, 6, 106, frame(**B_PICTURE), 0.0), ("sb64_leaf9", 64, 64, 9, 109, frame(), 0.0),
            ("sb64_leaf12", 64, 64, 12, 112, frame(**B_PICTURE), 0.0),
            ("edge_72x40_a", 72, 40, "random", 121, frame(), 0.15), ("edge_72x40_b", 72, 40, "random", 122, frame(**B_PICTURE), 0.15),
            ("mix_136x136_single", 136, 136, "random", 131, frame(), 0.3), ("mix_136x136_select", 136, 136, "random", 132, frame(**B_PICTURE), 0.3),
            ("hp_136x136", 136, 136, "random", 133, frame(allow_hp=1, **B_PICTURE), 0.1))
NAMES = [p[0] for p in PICTURES]


def rec(bit, prob):
    return (int(bit) << 8) | int(prob)


def tree_bools(tree, leaf, probs):
    """the bools from the root to `leaf`, node i >> 1 under probs[i >> 1]"""
    def walk(i, path):
        for bit in (0, 1):
            nxt, here = tree[i + bit], path + [rec(bit, probs[i >> 1])]
            if nxt == ("leaf", leaf):
                return here
            if isinstance(nxt, int):
                r = walk(nxt, here)
                if r:
                    return r
        return None
    return walk(0, [])


# ---------------------------------------------------------------------------------------------------
# the seeded pictures
# ---------------------------------------------------------------------------------------------------
def mv_component(rng, klass, even):
    """a non-zero MV difference of class `klass` (class 0: |v| 1 .. 16, class c: (8 << c) + 1 .. 16 << c, capped at 16383)"""
    lo, hi = (1, 16) if klass == 0 else ((8 << klass) + 1, min(16 << klass, 16383))
    v = int(rng.integers(lo, hi + 1))
    if even and v & 1:
        v += 1 if v < hi else -1
    return -v if rng.random() < 0.5 else v


def make_picture(W, H, kind, seed, fr, p_intra):
    """dict(lf_mi, mc_mi, ext, qcoeff, eob_map): a quad-tree of square leaves; an intra leaf has random modes (8x8 units also as four 4x4
    blocks), an inter leaf a random reference choice the frame allows, mode, mode context, reference MVs and -- NEWMV -- MV differences
    drawn by joint and class; random skip flags, sparse random coefficients in the coded leaves"""
    rng = np.random.default_rng(seed)
    mi_rows, mi_cols = H // 8, W // 8
    lf = np.zeros((mi_rows, mi_cols), B.LF_MODE_INFO_DTYPE)
    mc = np.zeros((mi_rows, mi_cols), B.MC_MODE_INFO_DTYPE)
    ext = np.zeros((mi_rows, mi_cols), B.MI_INTER_EXT_DTYPE)
    mc["ref_list"] = -1
    q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
    eoff = MM.eob_offsets(W, H)
    emap = np.zeros(eoff[3], np.uint16)
    offs, scans = TM.scan_tables()
    sb_cols = (W + 63) // 64
    fix_idx = fr["sign_bias"][fr["comp_fixed_ref"]]

    def leaf(r, c, t, intra):
        n = UNITS[t]
        area = (slice(r, r + n), slice(c, c + n))
        skip = int(rng.random() < 0.4)
        modes = [int(m) for m in rng.integers(0, 10, 4)]
        lf[area]["sb_type"], lf[area]["tx_size"], lf[area]["skip"], lf[area]["filter_level"], lf[area]["is_inter"] = t, TX[t], skip, 12, 0 if intra else 1
        mc[area]["bw8"] = mc[area]["bh8"] = n
        if intra:
            uv = int(rng.integers(0, 10))
            lf[area]["pad"] = (modes[2] | modes[3] << 4, modes[0] | modes[1] << 4, uv) if t == 0 else (0, modes[0], uv)
        else:
            comp = fr["reference_mode"] == COMPOUND or (fr["reference_mode"] == SELECT and rng.random() < 0.45)
            if comp:
                refs = [0, 0]
                refs[fix_idx], refs[1 - fix_idx] = fr["comp_fixed_ref"], fr["comp_var_ref"][int(rng.integers(0, 2))]
            else:
                refs = [int(rng.integers(1, 4)), 0]
            mode = int(rng.choice((NEARESTMV, NEARMV, ZEROMV, NEWMV, NEWMV, NEWMV)))
            e = np.zeros((), B.MI_INTER_EXT_DTYPE)
            m = np.zeros((), B.MC_MODE_INFO_DTYPE)
            e["ref_frame"], e["mode"], e["mode_context"] = refs, mode, int(rng.integers(0, 7))
            m["ref_list"], m["bw8"], m["bh8"] = (0 if refs[0] < ALTREF else 1, 1 if comp else -1), n, n
            for k in range(1 + comp):
                small = fr["allow_hp"] and rng.random() < 0.5
                ref_mv = [int(v) for v in rng.integers(-63, 64, 2)] if small else [int(v) * 2 for v in rng.integers(-1000, 1001, 2)]
                if fr["allow_hp"] and not small and max(abs(v) for v in ref_mv) < 64:
                    ref_mv[0] = 64                                         # exactly at the threshold: no high-precision bit
                usehp = bool(fr["allow_hp"]) and max(abs(v) for v in ref_mv) < 64
                joint = int(rng.integers(0, 4))
                diff = [mv_component(rng, int(rng.integers(0, 11)), not usehp) if joint & b else 0 for b in (2, 1)]
                if mode != NEWMV:
                    diff = [0, 0]
                e["ref_mv_row"][k], e["ref_mv_col"][k] = ref_mv
                m["mv_row"][k], m["mv_col"][k] = ref_mv[0] + diff[0], ref_mv[1] + diff[1]
            mc[area] = m
            ext[area]["ref_frame"] = refs
            ext[r, c] = e                                                   # mode, mode context and reference MVs: at the origin only
        if skip:
            return
        blocks = MM.leaf_tx_blocks(t, r, c)
        eobs = [0 if rng.random() < 0.3 else int(min(16 << (2 * ts), 1 + rng.geometric(0.25))) for _, _, _, ts, _ in blocks]
        if not any(eobs):
            eobs[int(rng.integers(0, len(eobs)))] = 1
        for (plane, x4, y4, ts, i), eob in zip(blocks, eobs):
            u = 8 if plane else 16
            tt = TM.INTRA_TX_TYPE[modes[i] if t == 0 else modes[0]] if intra and plane == 0 and ts < 3 else 0
            scan = scans[offs[(ts, tt)]:offs[(ts, tt)] + (16 << (2 * ts))]
            base = ((y4 // u) * sb_cols + x4 // u) * B.SB_COEFFS + (0, 4096, 5120)[plane] + MM._zorder(x4 % u, y4 % u) * 16
            for k in range(eob):
                v = int(rng.choice((1, 1, 1, 2, 2, 3, 4, 5, 9, 20, 70, 300))) if k == eob - 1 or rng.random() < 0.7 else 0
                q[base + int(scan[k])] = -v if rng.random() < 0.5 else v
            emap[eoff[plane] + y4 * (W // 8 if plane else W // 4) + x4] = eob

    def node(r, c, lv):
        if r >= mi_rows or c >= mi_cols:
            return
        s = 1 << lv
        inside = r + s <= mi_rows and c + s <= mi_cols
        if kind != "random":
            here = inside and UNITS[kind] == s
        else:
            here = inside and (lv == 0 or rng.random() < (0.2, 0.3, 0.4, 0.0)[3 - lv] + (0.15 if lv == 3 else 0))
        if here:
            intra = rng.random() < p_intra
            t = kind if kind != "random" else ((0 if intra and rng.random() < 0.5 else 3) if lv == 0 else (6, 9, 12)[lv - 1])
            return leaf(r, c, t, intra)
        for dr, dc in ((0, 0), (0, s // 2), (s // 2, 0), (s // 2, s // 2)):
            node(r + dr, c + dc, lv - 1)

    for r in range(0, mi_rows, 8):
        for c in range(0, mi_cols, 8):
            node(r, c, 3)
    return dict(W=W, H=H, frame=fr, lf_mi=lf, mc_mi=mc, ext=ext, qcoeff=q, eob_map=emap)


# ---------------------------------------------------------------------------------------------------
# the serial model
# ---------------------------------------------------------------------------------------------------
class Block:
    """one ModeInfo + its MbModeInfoExt: what the above / left pointers of a leaf's successors point at"""

    def __init__(self, lf, mc, ext):
        self.sb_type, self.skip, self.inter = int(lf["sb_type"]), int(lf["skip"]), int(lf["is_inter"]) != 0
        p = [int(v) for v in lf["pad"]]
        self.bmi = [p[1] & 15, p[1] >> 4, p[0] & 15, p[0] >> 4] if self.sb_type == 0 else [p[1]] * 4
        self.uv_mode = p[2]
        self.ref = [int(v) for v in ext["ref_frame"]] if self.inter else [INTRA, 0]
        self.comp = self.ref[1] > 0
        self.mode, self.mode_context = int(ext["mode"]), int(ext["mode_context"])
        self.mv = [(int(mc["mv_row"][k]), int(mc["mv_col"][k])) for k in range(2)]
        self.ref_mv = [(int(ext["ref_mv_row"][k]), int(ext["ref_mv_col"][k])) for k in range(2)]

    def uses(self, ref):
        return self.ref[0] == ref or (self.comp and self.ref[1] == ref)


def ctx_intra_inter(a, l):
    if a and l:
        return 3 if not a.inter and not l.inter else int(not a.inter or not l.inter)
    if a or l:
        return 2 * int(not (a or l).inter)
    return 0


def ctx_comp_flag(a, l, fixed):
    if a and l:
        if not a.comp and not l.comp:
            return int(a.ref[0] == fixed) ^ int(l.ref[0] == fixed)
        if not a.comp:
            return 2 + int(a.ref[0] == fixed or not a.inter)
        if not l.comp:
            return 2 + int(l.ref[0] == fixed or not l.inter)
        return 4
    if a or l:
        e = a or l
        return 3 if e.comp else int(e.ref[0] == fixed)
    return 1


def ctx_single_p1(a, l):
    if a and l:
        if not a.inter and not l.inter:
            return 2
        if not a.inter or not l.inter:
            e = l if not a.inter else a
            return 1 + int(e.uses(LAST)) if e.comp else 4 * int(e.ref[0] == LAST)
        if a.comp and l.comp:
            return 1 + int(a.uses(LAST) or l.uses(LAST))
        if a.comp or l.comp:
            single, comp = (l, a) if a.comp else (a, l)
            return (3 if single.ref[0] == LAST else 0) + int(comp.uses(LAST))
        return 2 * int(a.ref[0] == LAST) + 2 * int(l.ref[0] == LAST)
    if a or l:
        e = a or l
        if not e.inter:
            return 2
        return 1 + int(e.uses(LAST)) if e.comp else 4 * int(e.ref[0] == LAST)
    return 2


def ctx_single_p2(a, l):
    if a and l:
        if not a.inter and not l.inter:
            return 2
        if not a.inter or not l.inter:
            e = l if not a.inter else a
            if e.comp:
                return 1 + 2 * int(e.uses(GOLDEN))
            return 3 if e.ref[0] == LAST else 4 * int(e.ref[0] == GOLDEN)
        if a.comp and l.comp:
            return 3 * int(a.uses(GOLDEN) or l.uses(GOLDEN)) if a.ref == l.ref else 2
        if a.comp or l.comp:
            single, comp = (l, a) if a.comp else (a, l)
            g = int(comp.uses(GOLDEN))
            return 3 + g if single.ref[0] == GOLDEN else g if single.ref[0] == ALTREF else 1 + 2 * g
        if a.ref[0] == LAST and l.ref[0] == LAST:
            return 3
        if a.ref[0] == LAST or l.ref[0] == LAST:
            return 4 * int((l if a.ref[0] == LAST else a).ref[0] == GOLDEN)
        return 2 * int(a.ref[0] == GOLDEN) + 2 * int(l.ref[0] == GOLDEN)
    if a or l:
        e = a or l
        if not e.inter or (e.ref[0] == LAST and not e.comp):
            return 2
        return 3 * int(e.uses(GOLDEN)) if e.comp else 4 * int(e.ref[0] == GOLDEN)
    return 2


def ctx_comp_ref(a, l, fr):
    fixed, (v0, v1) = fr["comp_fixed_ref"], fr["comp_var_ref"]
    var_idx = 1 - fr["sign_bias"][fixed]
    var = lambda b: b.ref[var_idx] if b.comp else b.ref[0]      # noqa: E731
    if a and l:
        if not a.inter and not l.inter:
            return 2
        if not a.inter or not l.inter:
            return 1 + 2 * int(var(l if not a.inter else a) != v1)
        va, vl = var(a), var(l)
        if va == vl and va == v1:
            return 0
        if not a.comp and not l.comp:
            if (va == fixed and vl == v0) or (vl == fixed and va == v0):
                return 4
            return 3 if va == vl else 1
        if a.comp and l.comp:
            return 4 if va == vl else 2
        vc, vs = (va, vl) if a.comp else (vl, va)
        if vc == v1 and vs != v1:
            return 1
        return 2 if vs == v1 and vc != v1 else 4
    if a or l:
        e = a or l
        if not e.inter:
            return 2
        return (4 if e.comp else 3) * int(var(e) != v1)
    return 2


def mv_class_of(z):
    """class of |component| - 1: 0 below 16, then floor(log2(z / 8)), at most 10; and the class's first value"""
    c = 0 if z < 16 else min(10, (z >> 3).bit_length() - 1)
    return c, (8 << c if c else 0)


def mv_bools(diff, usehp, nmvc, cov):
    joints, comps = nmvc[:3], (nmvc[3:36], nmvc[36:69])
    joint = 2 * int(diff[0] != 0) + int(diff[1] != 0)
    cov["joint"].add(joint)
    out = tree_bools(MV_JOINT_TREE, joint, joints)
    for v, p in zip(diff, comps):
        if v == 0:
            continue
        sign, classes, class0, bits, class0_fp, fp, class0_hp, hp = p[0], p[1:11], p[11:12], p[12:22], (p[22:25], p[25:28]), p[28:31], p[31], p[32]
        c, base = mv_class_of(abs(v) - 1)
        o = abs(v) - 1 - base
        d, f, e = o >> 3, (o >> 1) & 3, o & 1
        cov["sign"].add(int(v < 0))
        cov["class"].add(c)
        out.append(rec(v < 0, sign))
        out += tree_bools(MV_CLASS_TREE, c, classes)
        if c == 0:
            cov["class0_int"].add(d)
            out.append(rec(d, class0[0]))
        else:
            out += [rec((d >> i) & 1, bits[i]) for i in range(c)]
        out += tree_bools(MV_FP_TREE, f, class0_fp[d] if c == 0 else fp)
        if usehp:
            out.append(rec(e, class0_hp if c == 0 else hp))
    return out


COVER_KEYS = ("partition", "skip", "intra_inter", "comp_flag", "single_p1", "single_p2", "comp_ref", "mode", "mode_ctx", "joint", "sign", "class", "class0_int", "hp",
              "size_group", "ref_frame")


def serial_walk(pic, tabs, cover=None):
    """(bool records of the picture in coding order, leaves [(r, c, sb_type, first bool, bools)] in coding order).  cover (a dict of sets)
    receives what was coded under which context"""
    lf_mi, mc_mi, ext, fr = pic["lf_mi"], pic["mc_mi"], pic["ext"], pic["frame"]
    mi_rows, mi_cols = pic["H"] // 8, pic["W"] // 8
    cols8 = ((mi_cols + 7) // 8) * 8
    above_seg, left_seg = [0] * cols8, [0] * 8          # partition contexts: above cleared once per picture, left per SB row
    above_blk, left_blk = [None] * cols8, [None] * 8    # the block last coded over a column / a row of the SB row
    out, leaves, first = [], [], {}
    cov = {} if cover is None else cover
    for k in COVER_KEYS:
        cov.setdefault(k, set())

    def node(r, c, lv):
        if r >= mi_rows or c >= mi_cols:
            return
        s, hbs = 1 << lv, (1 << lv) >> 1
        t = int(lf_mi[r, c]["sb_type"])
        first.setdefault((r, c), len(out))
        split = UNITS[t] < s or (lv == 0 and t == 0)
        ctx = 4 * lv + 2 * ((left_seg[r & 7] >> lv) & 1) + ((above_seg[c] >> lv) & 1)
        probs = tabs["partition_prob"][ctx]
        has_rows, has_cols = r + hbs < mi_rows, c + hbs < mi_cols
        if has_rows and has_cols:
            out.extend(tree_bools(PARTITION_TREE, 3 if split else 0, probs))
        elif has_cols:
            out.append(rec(1, probs[1]))
        elif has_rows:
            out.append(rec(1, probs[2]))
        if has_rows or has_cols:
            cov["partition"].add(ctx)
        if split and lv > 0:
            for dr, dc in ((0, 0), (0, hbs), (hbs, 0), (hbs, hbs)):
                node(r + dr, c + dc, lv - 1)
            return
        mi = Block(lf_mi[r, c], mc_mi[r, c], ext[r, c])
        a, l = (above_blk[c] if r > 0 else None), (left_blk[r & 7] if c > 0 else None)
        sctx = (a.skip if a else 0) + (l.skip if l else 0)
        cov["skip"].add(sctx)
        out.append(rec(mi.skip, tabs["skip_probs"][sctx]))
        ictx = ctx_intra_inter(a, l)
        cov["intra_inter"].add(ictx)
        out.append(rec(mi.inter, tabs["intra_inter_prob"][ictx]))
        if not mi.inter:
            cov["size_group"].add(SIZE_GROUP[t])
            for b in (range(4) if t == 0 else (0,)):
                out.extend(tree_bools(INTRA_MODE_TREE, mi.bmi[b], tabs["y_mode_prob"][SIZE_GROUP[t]]))
            out.extend(tree_bools(INTRA_MODE_TREE, mi.uv_mode, tabs["uv_mode_prob"][mi.bmi[3]]))
        else:
            if fr["reference_mode"] == SELECT:
                x = ctx_comp_flag(a, l, fr["comp_fixed_ref"])
                cov["comp_flag"].add(x)
                out.append(rec(mi.comp, tabs["comp_inter_prob"][x]))
            if mi.comp:
                x = ctx_comp_ref(a, l, fr)
                cov["comp_ref"].add(x)
                out.append(rec(mi.ref[1 - fr["sign_bias"][fr["comp_fixed_ref"]]] == fr["comp_var_ref"][1], tabs["comp_ref_prob"][x]))
            else:
                x = ctx_single_p1(a, l)
                cov["single_p1"].add(x)
                cov["ref_frame"].add(mi.ref[0])
                out.append(rec(mi.ref[0] != LAST, tabs["single_ref_prob"][x][0]))
                if mi.ref[0] != LAST:
                    x = ctx_single_p2(a, l)
                    cov["single_p2"].add(x)
                    out.append(rec(mi.ref[0] != GOLDEN, tabs["single_ref_prob"][x][1]))
            cov["mode"].add(mi.mode)
            cov["mode_ctx"].add(mi.mode_context)
            out.extend(tree_bools(INTER_MODE_TREE, mi.mode, tabs["inter_mode_probs"][mi.mode_context]))
            if mi.mode == NEWMV:
                for k in range(1 + mi.comp):
                    usehp = bool(fr["allow_hp"]) and abs(mi.ref_mv[k][0]) < 64 and abs(mi.ref_mv[k][1]) < 64
                    diff = (mi.mv[k][0] - mi.ref_mv[k][0], mi.mv[k][1] - mi.ref_mv[k][1])
                    if fr["allow_hp"] and any(diff):
                        cov["hp"].add(int(usehp))
                    out.extend(mv_bools(diff, usehp, tabs["nmvc"], cov))
        leaves.append((r, c, t, first[(r, c)], len(out) - first[(r, c)]))
        for i in range(s):                              # the leaf is now the last block over its columns and rows
            above_seg[c + i] = left_seg[(r + i) & 7] = SEG_CONTEXT[t]
            above_blk[c + i] = left_blk[(r + i) & 7] = mi

    for r in range(0, mi_rows, 8):
        left_seg[:] = [0] * 8
        for c in range(0, mi_cols, 8):
            node(r, c, 3)
    return np.array(out, np.uint16), leaves


def coverage_complete(cov):
    """what the fixture has to reach (the generator asserts it on the reference's own notes, the tests on the model's)"""
    want = dict(partition=set(range(16)), skip={0, 1, 2}, intra_inter={0, 1, 2, 3}, comp_flag=set(range(5)), single_p1=set(range(5)), single_p2=set(range(5)),
                comp_ref=set(range(5)), mode={10, 11, 12, 13}, mode_ctx=set(range(7)), joint={0, 1, 2, 3}, sign={0, 1}, hp={0, 1}, size_group={0, 1, 2, 3},
                ref_frame={1, 2, 3})
    want["class"], want["class0_int"] = set(range(11)), {0, 1}
    return [(k, sorted(want[k] - set(cov[k]))) for k in want if want[k] - set(cov[k])]


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


def tables_struct(tabs):
    t = np.zeros(1, B.MODES_INTER_TABLES_DTYPE)
    for n, _ in TABLE_SHAPES[:-1]:
        t[n][0] = tabs[n]
    raw = t.view(np.uint8)
    raw[291 - 69:] = tabs["nmvc"]            # mv_joints + mv_comps: nmv_context's layout
    return t


_tabs = None


def tables():
    """the reference's frame-context tables as numpy arrays + the same as the C struct"""
    global _tabs
    if _tabs is None:
        g = fixture()
        tabs = {n: g[n] for n, _ in TABLE_SHAPES}
        _tabs = (tabs, tables_struct(tabs))
    return _tabs


_pic_cache = {}


def fixture_picture(name):
    """dict(W, H, frame, lf_mi, mc_mi, ext, qcoeff, eob_map, tile, modes) of one picture of the fixture"""
    if name not in _pic_cache:
        g = fixture()
        W, H = (int(v) for v in g[f"size|{name}"])
        fp = [int(v) for v in g[f"frame|{name}"]]
        fr = dict(reference_mode=fp[0], allow_hp=fp[1], sign_bias=tuple(fp[2:6]), comp_fixed_ref=fp[6], comp_var_ref=(fp[7], fp[8]))
        shape = (H // 8, W // 8)
        _pic_cache[name] = dict(W=W, H=H, frame=fr, lf_mi=g[f"lf_mi|{name}"].view(B.LF_MODE_INFO_DTYPE).reshape(shape),
                                mc_mi=g[f"mc_mi|{name}"].view(B.MC_MODE_INFO_DTYPE).reshape(shape), ext=g[f"ext|{name}"].view(B.MI_INTER_EXT_DTYPE).reshape(shape),
                                qcoeff=g[f"qcoeff|{name}"], eob_map=g[f"eob_map|{name}"], tile=bytes(g[f"tile_bytes|{name}"]), modes=bytes(g[f"modes_bytes|{name}"]))
    return _pic_cache[name]


_tok_cache = {}


def host_tokens(name):
    """svt_hip_tokenize_picture on a fixture picture (shared, left unchanged)"""
    if name not in _tok_cache:
        p = fixture_picture(name)
        _tok_cache[name] = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], counts=False)
    return _tok_cache[name]


def fill_frame(p, fr):
    p.reference_mode, p.allow_hp, p.comp_fixed_ref = fr["reference_mode"], fr["allow_hp"], fr["comp_fixed_ref"]
    p.comp_var_ref[0], p.comp_var_ref[1] = fr["comp_var_ref"]
    for i in range(4):
        p.ref_frame_sign_bias[i] = fr["sign_bias"][i]


def host_modes(pic, tok_off, capacity=None, tabs=None, frame_override=None):
    """svt_hip_modes_inter_picture -> dict(rc, bools[:min(n, capacity)], n_bools, segments, guard, seg_guard); the grids may be wider
    than the picture (their common row length is the mi_stride)"""
    lib = B.load()
    W, H = pic["W"], pic["H"]
    cap = int(lib.svt_hip_modes_inter_bools_capacity(W, H)) if capacity is None else capacity
    n_seg = int(lib.svt_hip_modes_segments(W, H))
    mi, mc, ex = np.ascontiguousarray(pic["lf_mi"]), np.ascontiguousarray(pic["mc_mi"]), np.ascontiguousarray(pic["ext"])
    assert mi.shape == mc.shape == ex.shape
    em, to = np.ascontiguousarray(pic["eob_map"], np.uint16), np.ascontiguousarray(tok_off, np.uint32)
    bools = np.full(cap + 64, 0xA5A5, np.uint16)
    segs = np.full((n_seg + 8) * 3, 0x5A5A5A5A, np.uint32)
    n = np.full(1, 0x77777777, np.uint32)
    p = B.ModesInterPicture()
    p.d_lf_mi, p.d_mc_mi, p.d_ext, p.d_eob_map, p.d_tok_off = mi.ctypes.data, mc.ctypes.data, ex.ctypes.data, em.ctypes.data, to.ctypes.data
    p.d_bools, p.d_segments, p.d_n_bools, p.capacity = bools.ctypes.data, segs.ctypes.data, n.ctypes.data, cap
    fill_frame(p, frame_override or pic["frame"])
    t = tables()[1] if tabs is None else tabs
    rc = lib.svt_hip_modes_inter_picture(t.ctypes.data_as(C.c_void_p), C.byref(p), W, H, mi.shape[1])
    total = int(n[0])
    got = bools[:min(total, cap)].copy() if total != B.MODES_BAD_GRID else np.zeros(0, np.uint16)
    return dict(rc=rc, bools=got, n_bools=total, segments=segs[:3 * n_seg].view(B.BOOL_SEGMENT_DTYPE).copy(), guard=bools[cap:], seg_guard=segs[3 * n_seg:])


_host_cache = {}


def host_of(name):
    """the host form on a fixture picture (shared, left unchanged)"""
    if name not in _host_cache:
        _host_cache[name] = host_modes(fixture_picture(name), host_tokens(name)["tok_off"])
    return _host_cache[name]


def host_chain(name):
    """host tokeniser -> host mode-info stage -> host bool coder on a fixture picture: (tile bytes, mode-info-only bytes, modes result)"""
    tok, m = host_tokens(name), host_of(name)
    assert m["rc"] == 0
    segs = [tuple(int(v) for v in s) for s in m["segments"]]
    tile = BM.host_code(tokens=tok["tokens"], bools=m["bools"], segments=segs)[0]
    only = BM.host_code(bools=m["bools"], segments=[s for s in segs if s[2] == 1])[0]
    return tile, only, m


# ---------------------------------------------------------------------------------------------------
# pictures past the first pass of the SB scan (regenerated from seeds, shared by the CPU and the GPU tests of one process)
# ---------------------------------------------------------------------------------------------------
# 17 x 17 = 289 SBs: odd, more than 256, partial SBs on both edges
BIG = (("big_select_hp", 1080, 1080, "random", 143, frame(allow_hp=1, **B_PICTURE), 0.2), ("big_single_8x8", 1080, 1080, 3, 144, frame(), 0.0))
_big_cache = {}


def big_pictures():
    for name, W, H, kind, seed, fr, p_intra in BIG:
        if name not in _big_cache:
            _big_cache[name] = dict(name=name, **make_picture(W, H, kind, seed, fr, p_intra))
    return [_big_cache[b[0]] for b in BIG]


def big_host(name):
    """the host forms on a picture of big_pictures(): dict(tok, modes) -- computed once"""
    p = next(p for p in big_pictures() if p["name"] == name)
    if "host" not in p:
        tok = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], counts=False)
        m = host_modes(p, tok["tok_off"])
        assert m["rc"] == 0 and m["n_bools"] != B.MODES_BAD_GRID
        p["host"] = dict(tok=tok, modes=m)
    return p["host"]


def with_stride(pic, extra, seed):
    """the picture on grids of mi_cols + extra records a row, random bytes behind every row"""
    out = dict(pic)
    for k in ("lf_mi", "mc_mi", "ext"):
        out[k] = TM.with_stride(pic[k], extra, seed)
    return out

"""Python model of inter mode labelling (csrc/md_inter_core.h), written independently of the C text: the rule stated over the block
objects and find_mv_refs of tests/mvrefs_model.py -- which tests/golden/mvrefs_reference.npz pins to eb_vp9_find_mv_refs --, a
decoder-side replay that rebuilds every leaf's MVs from (mode, candidates, ref_mv, coded difference) alone, and what defines an
unfaithfully coded leaf here: one the replay gets wrong.  It keeps no window and no scratch grid.

Also here: how a fixture picture of the MV-reference or inter mode-info stage becomes an input of this stage (prepare: ref_frame and
mode erased, ref_list rewritten so that two reference lists can express the picture), seeded pictures whose MVs are candidates, zero,
odd, or far from every candidate, and ctypes wrappers of the host form."""
import ctypes as C
import os

import numpy as np

import modes_inter_model as IM
import mvrefs_model as M
import svt_testlib as T

B = T.B
NEARESTMV, NEARMV, ZEROMV, NEWMV = IM.NEARESTMV, IM.NEARMV, IM.ZEROMV, IM.NEWMV
MV_DIFF_MAX = 16383
BAD = (B.MODES_BAD_GRID,) * 4
GUARD = 64


# ---------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------
def ref_frames(pic):
    """ref_frame[2] of every unit from ref_list and list_ref_frame; intra units {0, 0}"""
    lrf = pic["lrf"]
    out = np.zeros(pic["lf_mi"].shape + (2,), np.uint8)
    inter = pic["lf_mi"]["is_inter"] != 0
    for k in range(2):
        rl = pic["mc_mi"]["ref_list"][..., k]
        out[..., k] = np.where(inter & (rl >= 0), np.where(rl == 0, lrf[0], lrf[1]), 0)
    return out


def choose(mvs, lists):
    """the label of a leaf: mvs[k] its MVs, lists[k] = ([cand 0, cand 1], found) of its k-th reference frame"""
    if all(n >= 1 and mv == lst[0] for mv, (lst, n) in zip(mvs, lists)):
        return NEARESTMV
    if all(n == 2 and mv == lst[1] for mv, (lst, n) in zip(mvs, lists)):
        return NEARMV
    if all(mv == (0, 0) for mv in mvs):
        return ZEROMV
    return NEWMV


def coded_then_decoded(diff, usehp):
    """one MV difference through eb_vp9_encode_mv and a decoder's read_mv: None where no class holds it; where the high-precision bit
    is not coded the decoder takes it as set"""
    out = []
    for d in diff:
        if abs(d) > MV_DIFF_MAX:
            return None
        if d == 0 or usehp:
            out.append(d)
        else:
            mag = ((abs(d) - 1) | 1) + 1
            out.append(-mag if d < 0 else mag)
    return tuple(out)


def use_mv_hp(mv):
    return abs(mv[0]) < 64 and abs(mv[1]) < 64


def label_picture(pic, ref_mask=M.ALL_REFS):
    """pic: dict(W, H, lf_mi, mc_mi, frame, restrict, lrf) of a well-formed picture -> dict(ext_out, cand, status, labels, unfaithful):
    the stage's outputs; labels {(r, c): mode}; unfaithful: the origins of the leaves a decoder would rebuild with other MVs"""
    mi_rows, mi_cols = pic["H"] // 8, pic["W"] // 8
    ext = np.zeros((mi_rows, mi_cols), B.MI_INTER_EXT_DTYPE)
    ext["ref_frame"] = ref_frames(pic)[:, :mi_cols]
    cut = dict(pic, lf_mi=pic["lf_mi"][:, :mi_cols], mc_mi=pic["mc_mi"][:, :mi_cols], ext=ext)
    ext["mode"] = NEWMV                  # (find_mv_refs also counts the neighbours' modes for the context, which is not looked at yet)
    blocks, grid = M.block_grid(cut)
    ext["mode"] = 0
    bias, restrict = pic["frame"]["sign_bias"], pic["restrict"]
    labels = {}
    for b in blocks:
        if not b.inter or b.t == 0:
            continue
        n_ref = 2 if b.ref[1] > 0 else 1
        lists = []
        for k in range(n_ref):
            lst, n, _ = M.find_mv_refs(grid, mi_rows, mi_cols, b, b.ref[k], restrict, bias)
            lists.append((lst, n))
        labels[(b.r, b.c)] = choose(b.mv[:n_ref], lists)
    for (r, c), mode in labels.items():
        ext[r, c]["mode"] = mode
    derived = M.derive_picture(cut, ref_mask=ref_mask)          # mode contexts and ref_mv_* from the labelled grid
    assert derived["status"][0] == 0 and derived["status"][1] == len(labels)
    # the decoder's side: MVs from the records alone
    all_cand = derived["cand"] if ref_mask == M.ALL_REFS else M.derive_picture(cut)["cand"]
    unfaithful = []
    for b in blocks:
        if (b.r, b.c) not in labels:
            continue
        e, k3 = derived["ext_out"][b.r, b.c], all_cand[b.r, b.c]
        rebuilt = []
        for k in range(2 if b.ref[1] > 0 else 1):
            f = int(e["ref_frame"][k]) - 1
            cand = [(int(k3["mv_row"][f][i]), int(k3["mv_col"][f][i])) for i in range(2)]
            ref_mv = (int(e["ref_mv_row"][k]), int(e["ref_mv_col"][k]))
            mode = int(e["mode"])
            if mode == NEWMV:
                diff = coded_then_decoded((b.mv[k][0] - ref_mv[0], b.mv[k][1] - ref_mv[1]), bool(pic["frame"]["allow_hp"]) and use_mv_hp(ref_mv))
                rebuilt.append(None if diff is None else (ref_mv[0] + diff[0], ref_mv[1] + diff[1]))
            else:
                rebuilt.append(cand[0] if mode == NEARESTMV else cand[1] if mode == NEARMV else (0, 0))
        if rebuilt != b.mv[:len(rebuilt)]:
            assert int(e["mode"]) == NEWMV, "only a NEWMV leaf can be rebuilt wrongly"
            unfaithful.append((b.r, b.c))
    n_new = sum(1 for m in labels.values() if m == NEWMV)
    return dict(ext_out=derived["ext_out"], cand=derived["cand"], status=(len(labels), n_new, len(unfaithful), 0), labels=labels, unfaithful=unfaithful)


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def pair_ok(fr, f0, f1):
    fix_idx = int(fr["sign_bias"][fr["comp_fixed_ref"]] != 0)
    refs = (f0, f1)
    return refs[fix_idx] == fr["comp_fixed_ref"] and refs[1 - fix_idx] in fr["comp_var_ref"]


def prepare(pic, lrf=(IM.LAST, IM.ALTREF)):
    """a picture with extension records -> this stage's input: ref_frame and mode erased; ref_list rewritten from the erased ref_frame
    so that the two lists express it (a single block whose frame is not lrf[1] goes to list 0; a compound block gets the order of the
    two lists the frame's compound rule accepts, or becomes a single block of list 0 where there is none)"""
    fr = pic["frame"]
    mc = pic["mc_mi"].copy()
    inter = pic["lf_mi"]["is_inter"] != 0
    f0, f1 = pic["ext"]["ref_frame"][..., 0], pic["ext"]["ref_frame"][..., 1]
    comp = inter & (f1 > 0)
    order = [(a, b) for a, b in ((0, 1), (1, 0)) if pair_ok(fr, lrf[a], lrf[b])]
    rl = np.full(mc.shape + (2,), -1, np.int8)
    rl[..., 0] = np.where(inter, np.where(~comp & (f0 == lrf[1]) & (lrf[0] != lrf[1]), 1, 0), -1)
    if order and fr["reference_mode"] != IM.SINGLE:
        rl[..., 0] = np.where(comp, order[0][0], rl[..., 0])
        rl[..., 1] = np.where(comp, order[0][1], -1)
    mc["ref_list"] = rl
    out = {k: v for k, v in pic.items() if k not in ("ext", "ext_out", "cand", "status", "tile", "modes", "consistent")}
    return dict(out, mc_mi=mc, lrf=tuple(lrf), restrict=pic.get("restrict", 0))


def labelled_ext(pic):
    """the extension records svt_hip_mvrefs_* needs to see the prepared picture as it was meant: ref_frame by the rule, modes 0"""
    ext = np.zeros(pic["lf_mi"].shape, B.MI_INTER_EXT_DTYPE)
    ext["ref_frame"] = ref_frames(pic)
    return ext


ODD = ((1, 0), (0, 1), (-1, 3), (5, -7))
FAR = ((16383, 0), (-16383, 0), (0, 16384), (0, -16384), (16385, 2), (-16382, -16386), (32767, -32768))


def seeded(W, H, seed, fr, restrict=0, lrf=(IM.LAST, IM.ALTREF), p_intra=0.15, p_leaf=None, odd=0.0, far=0.0, kind=None):
    """a seeded input whose MVs are what an encoder's would be -- most leaves carry a candidate of their neighbours, zero, or a candidate
    plus an even difference (mvrefs_model.make_consistent) --, then, with probability `odd` / `far` per NEWMV-meant leaf, an MV that
    differs from the first candidate by an entry of ODD / FAR (kept inside int16)"""
    p_leaf = p_leaf or {3: 0.2, 2: 0.35, 1: 0.5}
    if kind is not None:
        p_leaf = {lv: float(M.UNITS[kind] == 1 << lv) for lv in (1, 2, 3)}
    g = M.make_grid(W, H, seed, fr, p_intra, p_leaf)
    if fr["reference_mode"] == IM.COMPOUND:              # (make_grid draws compound leaves under REFERENCE_MODE_SELECT only)
        refs = [0, 0]
        refs[int(fr["sign_bias"][fr["comp_fixed_ref"]] != 0)], refs[int(fr["sign_bias"][fr["comp_fixed_ref"]] == 0)] = fr["comp_fixed_ref"], fr["comp_var_ref"][0]
        g["ext"]["ref_frame"][g["lf_mi"]["is_inter"] != 0] = refs
    first = prepare(g, lrf)
    g["ext"]["ref_frame"] = ref_frames(dict(first, lf_mi=g["lf_mi"]))       # the grid as the two lists express it, with the modes it was meant to have
    g["mc_mi"] = first["mc_mi"]
    M.make_consistent(g, restrict, seed + 1)
    rng = np.random.default_rng(seed + 2)
    blocks, _ = M.block_grid(g)
    for b in blocks:
        if not b.inter or b.mode != NEWMV:
            continue
        u = rng.random()
        table = ODD if u < odd else FAR if u < odd + far else None
        if table is None:
            continue
        area = (slice(b.r, b.r + b.n), slice(b.c, b.c + b.n))
        e = g["ext"][b.r, b.c]
        for k in range(2 if b.ref[1] > 0 else 1):
            d = table[int(rng.integers(0, len(table)))]
            row, col = int(e["ref_mv_row"][k]) + d[0], int(e["ref_mv_col"][k]) + d[1]
            row, col = (row if -32768 <= row <= 32767 else int(e["ref_mv_row"][k]) - d[0]), (col if -32768 <= col <= 32767 else int(e["ref_mv_col"][k]) - d[1])
            g["mc_mi"]["mv_row"][area + (k,)], g["mc_mi"]["mv_col"][area + (k,)] = row, col
    return prepare(g, lrf)


# ---------------------------------------------------------------------------------------------------
# the pictures of tests/golden/md_inter_reference.npz (written by tests/gen_golden_md_inter.py)
# ---------------------------------------------------------------------------------------------------
GOLD = os.path.join(T.GOLDEN_DIR, "md_inter_reference.npz")
# (name, width, height, seed, frame, restrict, list_ref_frame, share of intra leaves)
GOLDEN = (("edge_72x40_select", 72, 40, 401, IM.frame(reference_mode=IM.SELECT, sign_bias=M.ALT_BIAS), 0, (IM.LAST, IM.ALTREF), 0.15),
          ("mix_136x72_select_hp", 136, 72, 402, IM.frame(reference_mode=IM.SELECT, allow_hp=1, sign_bias=M.ALT_BIAS), 0, (IM.LAST, IM.ALTREF), 0.2),
          ("mix_136x72_single_restrict", 136, 72, 403, IM.frame(sign_bias=(0, 0, 1, 0)), 1, (IM.LAST, IM.GOLDEN), 0.1))


def encoder_like(W, H, seed, fr, restrict, lrf, p_intra, max_diff=600):
    """a picture with coefficients (modes_inter_model.make_picture) whose MVs are drawn the way a hierarchical-B picture's fall: walking
    the leaves in coding order, an inter leaf takes the first candidate of its neighbours, the second, zero, or the first plus a
    difference of at most max_diff eighths per component -- even unless the high-precision bit is coded.  Every label is then codable
    faithfully, and so is the same picture labelled all-NEWMV."""
    g = IM.make_picture(W, H, "random", seed, fr, p_intra)
    first = prepare(g, lrf)
    g["mc_mi"], g["restrict"] = first["mc_mi"], restrict
    g["ext"] = np.zeros_like(g["ext"])
    g["ext"]["ref_frame"] = ref_frames(first)
    g["ext"]["mode"] = NEWMV
    rng = np.random.default_rng(seed + 7)
    mi_rows, mi_cols = H // 8, W // 8
    blocks, grid = M.block_grid(g)
    for b in blocks:
        if not b.inter:
            continue
        what = int(rng.choice(4, p=(0.35, 0.2, 0.15, 0.3)))
        area = (slice(b.r, b.r + b.n), slice(b.c, b.c + b.n))
        for k in range(2 if b.ref[1] > 0 else 1):
            lst, _, _ = M.find_mv_refs(grid, mi_rows, mi_cols, b, b.ref[k], restrict, fr["sign_bias"])
            if what < 3:
                b.mv[k] = (lst[0], lst[1], (0, 0))[what]
            else:
                step = 1 if fr["allow_hp"] and use_mv_hp(lst[0]) else 2
                b.mv[k] = tuple(int(v + step * rng.integers(-(max_diff // step), max_diff // step + 1)) for v in lst[0])
            g["mc_mi"]["mv_row"][area + (k,)], g["mc_mi"]["mv_col"][area + (k,)] = b.mv[k]
    return dict(prepare(g, lrf), restrict=restrict)


def build_golden_pictures():
    return {name: encoder_like(W, H, seed, fr, restrict, lrf, p_intra) for name, W, H, seed, fr, restrict, lrf, p_intra in GOLDEN}


def all_newmv(pic, ext):
    """the labelled records of a picture with every inter leaf relabelled NEWMV: ref_mv_* stay, the mode contexts follow the new modes"""
    cut = dict(pic, ext=ext.copy())
    cut["ext"]["mode"] = np.where((ext["mode"] >= NEARESTMV), NEWMV, ext["mode"])
    return M.derive_picture(cut)["ext_out"]


_gold = None


def golden():
    global _gold
    if _gold is None:
        g = np.load(GOLD)
        _gold = {k: g[k] for k in g.files}
    return _gold


_gold_pics = {}


def golden_picture(name):
    """dict(W, H, frame, restrict, lrf, lf_mi, mc_mi, qcoeff, eob_map, ext, tile, all_newmv_bytes) of one picture of the fixture: ext are
    the records the reference's eb_vp9_find_mv_refs and the four-way comparison gave, tile the bytes the reference wrote for them"""
    if name not in _gold_pics:
        g = golden()
        W, H = (int(v) for v in g[f"size|{name}"])
        pp = [int(v) for v in g[f"params|{name}"]]
        fr = dict(reference_mode=pp[5], allow_hp=pp[6], sign_bias=tuple(pp[1:5]), comp_fixed_ref=pp[9], comp_var_ref=(pp[10], pp[11]))
        shape = (H // 8, W // 8)
        q = np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16)
        q[g[f"q_idx|{name}"]] = g[f"q_val|{name}"]
        _gold_pics[name] = dict(W=W, H=H, frame=fr, restrict=pp[0], lrf=(pp[7], pp[8]), lf_mi=g[f"lf_mi|{name}"].view(B.LF_MODE_INFO_DTYPE).reshape(shape),
                                mc_mi=g[f"mc_mi|{name}"].view(B.MC_MODE_INFO_DTYPE).reshape(shape), qcoeff=q, eob_map=g[f"eob_map|{name}"],
                                ext=g[f"ext|{name}"].view(B.MI_INTER_EXT_DTYPE).reshape(shape), tile=bytes(g[f"tile_bytes|{name}"]),
                                all_newmv_bytes=int(g[f"all_newmv_bytes|{name}"]))
    return _gold_pics[name]


_big = None


def big_picture():
    """17 x 17 = 289 SBs: more than one entry per thread of the status pass and threads with none; regenerated from its seed"""
    global _big
    if _big is None:
        fr = IM.frame(reference_mode=IM.SELECT, sign_bias=M.ALT_BIAS)
        _big = seeded(1080, 1080, 351, fr, p_leaf={3: 0.15, 2: 0.3, 1: 0.4}, odd=0.05, far=0.05)
    return _big


def fixture_inputs():
    """[(name, prepared picture)]: every picture of the two fixtures the issue names, erased"""
    out = []
    for name in M.names():
        out.append((f"mvrefs|{name}", prepare(M.fixture_picture(name))))
    for name in IM.NAMES:
        out.append((f"modes_inter|{name}", prepare(IM.fixture_picture(name))))
    return out


# ---------------------------------------------------------------------------------------------------
# the product's host entry point
# ---------------------------------------------------------------------------------------------------
def fill_picture(p, pic, ref_mask=M.ALL_REFS, **over):
    fr = pic["frame"]
    v = dict(list_ref_frame=pic["lrf"], ref_frame_sign_bias=fr["sign_bias"], restrict_ref_mvs=pic["restrict"], allow_hp=fr["allow_hp"],
             reference_mode=fr["reference_mode"], comp_fixed_ref=fr["comp_fixed_ref"], comp_var_ref=fr["comp_var_ref"], ref_mask=ref_mask)
    v.update(over)
    for k, val in v.items():
        if isinstance(val, (tuple, list)):
            for i, x in enumerate(val):
                getattr(p, k)[i] = x
        else:
            setattr(p, k, val)


def host_md_inter(pic, ref_mask=M.ALL_REFS, want_cand=True, **over):
    """svt_hip_md_inter_modes_picture -> dict(rc, ext_out, cand, status, guards intact); the grids are exactly rows x mi_stride records;
    the outputs are returned cut to the picture (raw_*: with what lies behind every row and the guard)"""
    lib = B.load()
    W, H = pic["W"], pic["H"]
    mi, mc = np.ascontiguousarray(pic["lf_mi"]), np.ascontiguousarray(pic["mc_mi"])
    assert mi.shape == mc.shape
    rows, stride = mi.shape
    eo = np.full(rows * stride * 12 + GUARD, 0xA5, np.uint8)
    ca = np.full(rows * stride * 32 + GUARD, 0x5A, np.uint8)
    st = np.full(4 + 4, 0x77777777, np.uint32)
    p = B.MdInterPicture()
    p.d_lf_mi, p.d_mc_mi, p.d_ext_out, p.d_status = mi.ctypes.data, mc.ctypes.data, eo.ctypes.data, st.ctypes.data
    p.d_cand = ca.ctypes.data if want_cand else None
    fill_picture(p, pic, ref_mask, **over)
    rc = lib.svt_hip_md_inter_modes_picture(C.byref(p), W, H, stride)
    return dict(rc=rc, ext_out=eo[:-GUARD].view(B.MI_INTER_EXT_DTYPE).reshape(rows, stride)[:, :W // 8].copy(), raw_ext=eo, raw_cand=ca,
                full_ext=eo[:-GUARD].view(B.MI_INTER_EXT_DTYPE).reshape(rows, stride).copy(),
                cand=ca[:-GUARD].view(B.MVREF_CAND_DTYPE).reshape(rows, stride)[:, :W // 8].copy(), status=tuple(int(v) for v in st[:4]),
                guards=bool((eo[-GUARD:] == 0xA5).all() and (ca[-GUARD:] == 0x5A).all() and (st[4:] == 0x77777777).all()))


def closure(pic, got, ref_mask=M.ALL_REFS):
    """the existing MV-reference host form over the labelled records -> (its status, whether its d_ext_out equals the stage's byte for byte)"""
    again = M.host_mvrefs(dict(pic, ext=got["full_ext"]), ref_mask=ref_mask)
    assert again["rc"] == 0 and again["guards"]
    return again["status"], bool(np.array_equal(again["ext_out"].view(np.uint8), got["ext_out"].view(np.uint8))), again


def with_stride(pic, extra, seed):
    """the picture on grids of mi_cols + extra records a row, random bytes behind every row"""
    import tokenize_model as TM
    return dict(pic, lf_mi=TM.with_stride(pic["lf_mi"], extra, seed), mc_mi=TM.with_stride(pic["mc_mi"], extra, seed + 1))

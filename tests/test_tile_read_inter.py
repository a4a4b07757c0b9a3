"""CPU: the tile reader on inter pictures (svt_hip_tile_read_host, svt_hip_frame_read_host; svt-vp9_amd/host/frame_read.c) -- the reference's
tiles of tests/golden/md_inter_reference.npz read back to the fixture's three grids, coefficients and eob maps, byte for byte; round trips
through the host writers (labelling -> tokeniser -> inter mode info -> bool coder) on seeded grids with odd and far MVs, encoder-like
grids, MV differences at the ceilings and around the high-precision bit; header plus tile in one call with the decoder's filter-level
rule; refusals; truncated and corrupted tiles with every guard intact, also in a stand-alone program under ASan and UBSan.
What the reader shows about the section 5.10 fixture is pinned below."""
import ctypes as C
import glob
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import boolcode_model as BM
import frame_model as FM
import md_inter_model as D
import modes_inter_model as IM
import modes_model as MM
import mvrefs_model as VM
import svt_testlib as T
import tokenize_model as TM
from test_frame_read import flip, sanitizer_runtime_present
from test_md_inter import SEEDED, seeded, uniform

B = T.B
BT, KT, IT = BM.tables()[1], MM.tables()[1], IM.tables()[1]        # (kept alive: the calls take their addresses)
PAD = 32
FILL = {"lf": 0xEE, "mc": 0xDD, "ex": 0xCC}


def params_of(W, H, stride, fr, restrict, lrf, level=0, **over):
    par = B.TileReadParams()
    par.width, par.height, par.mi_stride = W, H, stride
    par.reference_mode, par.allow_hp, par.restrict_ref_mvs, par.filter_level = fr["reference_mode"], fr["allow_hp"], restrict, level
    for i in range(4):
        par.ref_frame_sign_bias[i] = fr["sign_bias"][i]
    par.list_ref_frame[0], par.list_ref_frame[1] = lrf
    for k, v in over.items():
        setattr(par, k, v)
    return par


class Outputs:
    """every output array between guards; the grids' columns beyond mi_cols are guards too"""

    def __init__(self, W, H, stride):
        self.rows, self.cols, self.stride = H // 8, W // 8, stride
        self.nco, self.nem = T.n_sb(W, H) * B.SB_COEFFS, (W // 4) * (H // 4) * 3 // 2
        n = self.rows * stride
        self.lf, self.mc, self.ex = (np.full(k * (n + 2 * PAD), FILL[f], np.uint8) for k, f in ((8, "lf"), (12, "mc"), (12, "ex")))
        self.q, self.em, self.res = np.full(self.nco + 2 * PAD, 0x5A5A, np.int16), np.full(self.nem + 2 * PAD, 0xA5A5, np.uint16), np.full(8 + 2 * PAD, 0x77777777, np.uint32)

    def pointers(self):
        vp = lambda a, o: C.c_void_p(a.ctypes.data + o)      # noqa: E731
        return [vp(self.lf, 8 * PAD), vp(self.mc, 12 * PAD), vp(self.ex, 12 * PAD), vp(self.q, 2 * PAD), vp(self.em, 2 * PAD), vp(self.res, 4 * PAD)]

    def grids(self):
        n = self.rows * self.stride
        return [a[k * PAD:k * (PAD + n)].view(dt).reshape(self.rows, self.stride) for a, k, dt in
                ((self.lf, 8, B.LF_MODE_INFO_DTYPE), (self.mc, 12, B.MC_MODE_INFO_DTYPE), (self.ex, 12, B.MI_INTER_EXT_DTYPE))]

    def guards(self):
        n, ok = self.rows * self.stride, True
        for a, k, f in ((self.lf, 8, "lf"), (self.mc, 12, "mc"), (self.ex, 12, "ex")):
            body = a[k * PAD:k * (PAD + n)].reshape(self.rows, self.stride * k)
            ok &= bool((a[:k * PAD] == FILL[f]).all() and (a[k * (PAD + n):] == FILL[f]).all() and (body[:, self.cols * k:] == FILL[f]).all())
        return ok and bool((self.q[:PAD] == 0x5A5A).all() and (self.q[PAD + self.nco:] == 0x5A5A).all() and (self.em[:PAD] == 0xA5A5).all() and
                           (self.em[PAD + self.nem:] == 0xA5A5).all() and (self.res[:PAD] == 0x77777777).all() and (self.res[PAD + 8:] == 0x77777777).all())

    def result(self):
        lf, mc, ex = (g[:, :self.cols] for g in self.grids())
        return dict(lf_mi=lf, mc_mi=mc, ext=ex, qcoeff=self.q[PAD:PAD + self.nco], eob_map=self.em[PAD:PAD + self.nem],
                    res=self.res[PAD:PAD + 8].view(B.TILE_READ_RESULT_DTYPE)[0], guards=self.guards())


def read_tile(tile, W, H, fr, restrict=0, lrf=(IM.LAST, IM.ALTREF), level=0, stride=None, **over):
    stride = stride or W // 8
    buf = np.frombuffer(bytes(tile), np.uint8).copy() if len(tile) else np.zeros(1, np.uint8)      # exactly the tile's bytes
    out, par = Outputs(W, H, stride), params_of(W, H, stride, fr, restrict, lrf, level, **over)
    vp = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    rc = B.load().svt_hip_tile_read_host(vp(buf), len(tile), C.byref(par), vp(BT), vp(KT), vp(IT), *out.pointers())
    return rc, out.result()


def same_grids(got, want, what, mvs=None):
    """the three grids, field by field; the prediction grid's fields of an intra unit other than ref_list mean nothing to any stage"""
    assert got["guards"], what
    for f in got["lf_mi"].dtype.names:
        assert np.array_equal(got["lf_mi"][f], want["lf_mi"][f]), (what, "lf_mi", f)
    inter = want["lf_mi"]["is_inter"] != 0
    assert np.array_equal(got["mc_mi"]["ref_list"], want["mc_mi"]["ref_list"]), (what, "ref_list")
    for f in ("mv_row", "mv_col", "bw8", "bh8"):
        assert np.array_equal(got["mc_mi"][f][inter], (want["mc_mi"] if mvs is None or f[:2] != "mv" else mvs)[f][inter]), (what, "mc_mi", f)
    assert got["ext"].tobytes() == np.ascontiguousarray(want["ext"]).tobytes(), (what, [f for f in got["ext"].dtype.names if not np.array_equal(got["ext"][f], want["ext"][f])])


def check_reads_back(tile, p, what, ext=None, mvs=None, stride=None):
    rc, got = read_tile(tile, p["W"], p["H"], p["frame"], p.get("restrict", 0), p.get("lrf", (IM.LAST, IM.ALTREF)), int(p["lf_mi"]["filter_level"][0, 0]), stride)
    assert rc == 0, (what, B.load().svt_hip_last_error())
    same_grids(got, dict(p, ext=p["ext"] if ext is None else ext), what, mvs)
    assert np.array_equal(got["qcoeff"], p["qcoeff"]) and np.array_equal(got["eob_map"], np.asarray(p["eob_map"]).view(np.uint16)), what
    res = got["res"]
    # vpx_reader_find_end: the tile's length, or one less where the last byte is padding the decoder's window never started on
    assert res["tile_bytes"] == len(tile) or (res["tile_bytes"] == len(tile) - 1 and tile[-1] == 0), (what, res)
    assert res["past_end"] == 0 and res["inter_leaves"] > 0, (what, res)
    return got


@pytest.mark.parametrize("name", [g[0] for g in D.GOLDEN])
def test_the_reference_tiles_of_the_labelling_fixture_read_back(name):
    p = D.golden_picture(name)
    got = check_reads_back(p["tile"], p, name)
    lf = p["lf_mi"]
    assert got["res"]["inter_leaves"] == sum(1 for r in range(p["H"] // 8) for c in range(p["W"] // 8)
                                             if lf["is_inter"][r, c] and r % MM.UNITS[int(lf["sb_type"][r, c])] == 0 and c % MM.UNITS[int(lf["sb_type"][r, c])] == 0)


def host_tile(p, ext):
    """tokeniser -> inter mode info -> bool coder on the host; None where the mode-info stage refuses the grid (an MV difference beyond the range)"""
    tok = TM.host_tokenize_picture(p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], counts=False)
    m = IM.host_modes(dict(p, ext=ext), tok["tok_off"])
    assert m["rc"] == 0
    if m["n_bools"] == B.MODES_BAD_GRID:
        return None
    return BM.host_code(tokens=tok["tokens"], bools=m["bools"], segments=[tuple(int(v) for v in s) for s in m["segments"]])[0]


def decoded_mvs(p, ext):
    """the prediction grid as a decoder rebuilds it: a NEWMV leaf's MV is its reference MV plus the difference as coded -- odd differences
    become even where the high-precision bit is not coded (md_inter_model.coded_then_decoded)"""
    mc = p["mc_mi"].copy()
    for r in range(p["H"] // 8):
        for c in range(p["W"] // 8):
            n = MM.UNITS[int(p["lf_mi"]["sb_type"][r, c])]
            o = ext[r - r % n, c - c % n]
            if not p["lf_mi"]["is_inter"][r, c] or o["mode"] != 13:
                continue
            for k in range(2 if ext["ref_frame"][r, c, 1] else 1):
                ref = (int(o["ref_mv_row"][k]), int(o["ref_mv_col"][k]))
                diff = (int(mc["mv_row"][r, c, k]) - ref[0], int(mc["mv_col"][r, c, k]) - ref[1])
                back = D.coded_then_decoded(diff, p["frame"]["allow_hp"] and D.use_mv_hp(ref))
                mc["mv_row"][r, c, k], mc["mv_col"][r, c, k] = ref[0] + back[0], ref[1] + back[1]
    return mc


def with_no_coefficients(p):
    lf = p["lf_mi"].copy()
    lf["skip"] = 1
    return dict(p, lf_mi=lf, qcoeff=np.zeros(T.n_sb(p["W"], p["H"]) * B.SB_COEFFS, np.int16), eob_map=np.zeros((p["W"] // 4) * (p["H"] // 4) * 3 // 2, np.uint16))


def labelled(p):
    got = D.host_md_inter(p, ref_mask=0, want_cand=False)
    assert got["rc"] == 0 and got["status"][0] not in (0, B.MODES_BAD_GRID)
    return got["ext_out"], got["status"]


def decoder_consistent(p):
    """A NEWMV leaf whose difference is not coded faithfully (odd without the high-precision bit) decodes to another MV, and every later leaf
    that takes a candidate from it then derives other records than the encoder's grid gave: that drift is what section 5.13 counts and forbids
    to ship.  For an exact round trip the grid is first brought to what a decoder rebuilds -- each leaf's MVs replaced by their decoded values
    and the picture labelled again -- until nothing changes; odd MVs stay wherever the bit is coded or a candidate supplies them.
    None where a difference beyond +-16383 remains: such a picture is not codable."""
    for _ in range(600):                 # (a change reaches later leaves only: at most one round per leaf)
        ext, status = labelled(p)
        if status[2] == 0:
            return p, ext
        want = p["mc_mi"].copy()
        for r in range(p["H"] // 8):
            for c in range(p["W"] // 8):
                n = MM.UNITS[int(p["lf_mi"]["sb_type"][r, c])]
                o = ext[r - r % n, c - c % n]
                if not p["lf_mi"]["is_inter"][r, c] or o["mode"] != 13:
                    continue
                for k in range(2 if ext["ref_frame"][r, c, 1] else 1):
                    ref = (int(o["ref_mv_row"][k]), int(o["ref_mv_col"][k]))
                    usehp = p["frame"]["allow_hp"] and D.use_mv_hp(ref)
                    top = D.MV_DIFF_MAX if usehp else D.MV_DIFF_MAX - 1           # (without the bit the largest codable magnitude is even)
                    diff = tuple(max(-top, min(top, d)) for d in (int(want["mv_row"][r, c, k]) - ref[0], int(want["mv_col"][r, c, k]) - ref[1]))
                    back = D.coded_then_decoded(diff, usehp)
                    want["mv_row"][r, c, k], want["mv_col"][r, c, k] = ref[0] + back[0], ref[1] + back[1]
        p = dict(p, mc_mi=want)
    return None


@pytest.mark.parametrize("name", [s[0] for s in SEEDED])
def test_round_trip_of_seeded_grids_with_odd_and_far_mvs(name):
    fixed = decoder_consistent(with_no_coefficients(seeded(name)))
    assert fixed is not None
    p, ext = fixed
    tile = host_tile(p, ext)
    assert tile is not None
    check_reads_back(tile, p, name, ext=ext)


@pytest.mark.parametrize("seed,fr,restrict", [(71, IM.frame(**IM.B_PICTURE), 0), (72, IM.frame(allow_hp=1, **IM.B_PICTURE), 1), (73, IM.frame(), 0)])
def test_round_trip_of_encoder_like_grids_with_coefficients(seed, fr, restrict):
    p = D.encoder_like(136, 72, seed, fr, restrict, (IM.LAST, IM.ALTREF), 0.15)
    p, ext = decoder_consistent(p)
    got = check_reads_back(host_tile(p, ext), p, seed, ext=ext)
    assert got["res"]["tokens"] > 0 and got["eob_map"].any()
    check_reads_back(host_tile(p, ext), p, (seed, "stride"), ext=ext, stride=p["W"] // 8 + 5)


@pytest.mark.parametrize("allow_hp", [0, 1])
@pytest.mark.parametrize("mv", [(16383, -16383), (-16383, 16383), (1, -1), (-1, 0), (0, 1), (63, 65)])
def test_mv_differences_at_the_ceilings_and_around_the_high_precision_bit(mv, allow_hp):
    p = uniform(64, 64, IM.frame(allow_hp=allow_hp))
    p["mc_mi"][0, 0]["mv_row"][0], p["mc_mi"][0, 0]["mv_col"][0] = mv        # unit (0, 0) has no candidate: the reference MV is 0, the difference the MV
    p = with_no_coefficients(p)
    ext, _ = labelled(p)
    assert ext["mode"][0, 0] == 13
    want = decoded_mvs(p, ext)
    back = tuple(int(v) for v in (want["mv_row"][0, 0, 0], want["mv_col"][0, 0, 0]))
    faithful = allow_hp == 1 or not (mv[0] | mv[1]) & 1
    assert (back == mv) == faithful and back == tuple(m if faithful or m == 0 else (abs(m) + 1) * (1 if m > 0 else -1) for m in mv)
    tile = host_tile(p, ext)
    if faithful:
        check_reads_back(tile, p, (mv, allow_hp), ext=ext)
    else:      # the leaf decodes to the even MV, and the leaves that take it as a candidate follow it: only the leaf itself is compared
        rc, got = read_tile(tile, 64, 64, p["frame"], level=12)
        assert rc == 0 and got["guards"] and (int(got["mc_mi"]["mv_row"][0, 0, 0]), int(got["mc_mi"]["mv_col"][0, 0, 0])) == back and got["ext"]["mode"][0, 0] == 13


def derivable(p):
    """do the picture's extension records hold what the MV-reference derivation gives for its grids?"""
    got = VM.host_mvrefs(dict(p, restrict=p.get("restrict", 0)), ref_mask=0, want_cand=False)
    return got["rc"] == 0 and got["ext_out"].tobytes() == np.ascontiguousarray(p["ext"]).tobytes()


@pytest.mark.parametrize("name", IM.NAMES)
def test_the_mode_info_fixture_tiles_are_not_decodable_and_why(name):
    """Finding.  The records of tests/golden/modes_inter_reference.npz (ref_mv_*, mode_context) are INPUTS drawn at random for the writer:
    they are not what eb_vp9_find_mv_refs derives from the same grids, so a decoder -- which derives them -- reads the inter mode under
    another context and NEWMV against another reference MV.  The writer's bytes equal the reference's for those inputs and the tile is
    still no decodable stream; the two whole inter frames of frame_reference.npz carry these tiles.  The labelling fixture (above) is the
    one whose records are derived."""
    p = IM.fixture_picture(name)
    assert not derivable(p)
    rc, got = read_tile(p["tile"], p["W"], p["H"], p["frame"], 0, (IM.LAST, IM.ALTREF), int(p["lf_mi"]["filter_level"][0, 0]))
    assert got["guards"]
    assert rc != 0 or got["ext"].tobytes() != np.ascontiguousarray(p["ext"]).tobytes()


def read_frame(frame, W, H, restrict=0, lrf=(IM.LAST, IM.ALTREF), last_ref=FM.DEFAULT_REF_DELTAS, last_mode=(0, 0)):
    buf = np.frombuffer(bytes(frame), np.uint8).copy()
    out, info = Outputs(W, H, W // 8), B.FrameReadInfo()
    vp = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    ptr = out.pointers()
    rc = B.load().svt_hip_frame_read_host(vp(buf), len(buf), (C.c_int8 * 4)(*last_ref), (C.c_int8 * 2)(*last_mode), W // 8, restrict, (C.c_uint8 * 2)(*lrf), vp(BT), vp(KT), vp(IT),
                                           C.byref(info), *ptr)
    return rc, info, out.result()


def test_header_plus_tile_in_one_call_with_the_decoders_filter_level_rule():
    p = D.golden_picture("edge_72x40_select")
    fp = FM.inter(width=72, height=40, reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1), frame_parallel_decoding_mode=1,
                  filter_level=40, mode_ref_delta_enabled=1, mode_ref_delta_update=1, ref_deltas=(2, 0, -1, -3), mode_deltas=(-1, 1), base_qindex=120)
    frame = FM.host_header_bytes(fp) + p["tile"]
    rc, info, got = read_frame(frame, 72, 40)
    assert rc == 0 and info.needs_backward_adaptation == 0 and info.interp_filter == B.READ_FILTER_REGULAR, B.load().svt_hip_last_error()
    # vp9_loop_filter_frame_init: level + ref_deltas[ref_frame[0]] * scale (+ mode_deltas[mode != ZEROMV] * scale for inter), scale = 1 << (level >> 5)
    want = p["lf_mi"].copy()
    for r in range(5):
        for c in range(9):
            n = MM.UNITS[int(want["sb_type"][r, c])]
            f0, mode = int(p["ext"]["ref_frame"][r, c, 0]), int(p["ext"]["mode"][r - r % n, c - c % n])
            want["filter_level"][r, c] = min(63, max(0, 40 + 2 * fp["ref_deltas"][f0] + (2 * fp["mode_deltas"][mode != 12] if f0 else 0)))
    assert len(set(want["filter_level"].ravel().tolist())) >= 3
    same_grids(got, dict(p, lf_mi=want), "frame")
    assert np.array_equal(got["qcoeff"], p["qcoeff"]) and got["res"]["tile_bytes"] == len(p["tile"])
    # a key frame through the same entry
    k = MM.fixture_picture("edge_72x40_a")
    rc, info, got = read_frame(FM.fixture_case("whole_key_a")[1], 72, 40)
    assert rc == 0 and got["guards"] and np.array_equal(got["qcoeff"], k["qcoeff"]) and (got["lf_mi"]["filter_level"] == info.params.filter_level).all()
    assert all(np.array_equal(got["lf_mi"][f], k["lf_mi"][f]) for f in ("sb_type", "tx_size", "skip", "is_inter", "pad"))
    assert (got["mc_mi"].view(np.uint8) == FILL["mc"]).all()                # an intra-only picture's further grids are not touched


def test_refusals():
    lib = B.load()
    p = D.golden_picture("edge_72x40_select")
    args = (p["tile"], 72, 40, p["frame"], 0)

    def refused(rc_got, word, code=B.ERR_UNSUPPORTED):
        rc, got = rc_got
        assert rc == code and got["guards"] and word in lib.svt_hip_last_error(), (rc, lib.svt_hip_last_error())
    refused(read_tile(*args, lrf=(IM.LAST, IM.GOLDEN)), b"no list")                                   # ALTREF is coded, no list stands for it
    refused(read_tile(*args, interp_filter=B.READ_FILTER_SWITCHABLE), b"filter")
    refused(read_tile(*args, interp_filter=B.READ_FILTER_SHARP), b"filter")
    refused(read_tile(*args, lossless=1), b"lossless")
    refused(read_tile(*args, reference_mode=3), b"bad argument", B.ERR_BAD_PARAMETER)
    refused(read_tile(p["tile"], 70, 40, p["frame"], stride=9), b"size", B.ERR_BAD_PARAMETER)
    v = next(VM.fixture_picture(n) for n in VM.names(consistent=1) if (VM.fixture_picture(n)["ext"]["ref_frame"] == IM.GOLDEN).any())
    refused(read_tile(v["tile"], v["W"], v["H"], v["frame"], v["restrict"]), b"no list")               # a GOLDEN block under lists of LAST and ALTREF
    # through the frame entry: reference scaling (found_ref), a switchable filter, lossless, a size that is no multiple of 8
    head = FM.host_header_bytes(FM.inter(width=72, height=40, reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1)))
    rc, _, got = read_frame(flip(head, 30) + p["tile"], 72, 40)
    assert rc == B.ERR_UNSUPPORTED and got["guards"] and b"found_ref" in lib.svt_hip_last_error()
    rc, info, got = read_frame(flip(head, 33 + 32 + 1 + 1) + p["tile"], 72, 40)      # switchable: its probability flags shift the compressed header too
    assert rc != 0 and got["guards"] and (got["lf_mi"].view(np.uint8) == FILL["lf"]).all()
    rc, _, got = read_frame(FM.host_header_bytes(FM.inter(width=72, height=40, base_qindex=0)) + p["tile"], 72, 40)
    assert rc == B.ERR_UNSUPPORTED and got["guards"] and b"lossless" in lib.svt_hip_last_error()
    rc, _, got = read_frame(FM.host_header_bytes(FM.inter(width=70, height=40)) + p["tile"], 72, 40)
    assert rc == B.ERR_UNSUPPORTED and got["guards"] and b"multiple of 8" in lib.svt_hip_last_error()
    rc, _, got = read_frame(FM.show_existing(2), 72, 40)
    assert rc == B.ERR_BAD_PARAMETER and got["guards"]


def test_truncated_and_corrupted_inter_tiles_return_with_guards_intact():
    rng = np.random.default_rng(41)
    p = D.golden_picture("edge_72x40_select")
    tile, codes = p["tile"], (0, B.ERR_BAD_PARAMETER, B.ERR_UNSUPPORTED)
    for n in range(len(tile) + 1):
        rc, got = read_tile(tile[:n], 72, 40, p["frame"])
        assert got["guards"] and rc in codes, n
    for _ in range(200):
        bad = bytearray(tile)
        for _ in range(int(rng.integers(1, 5))):
            bad[int(rng.integers(0, len(bad)))] ^= int(rng.integers(1, 256))
        rc, got = read_tile(bytes(bad), 72, 40, p["frame"])
        assert got["guards"] and rc in codes
        if rc == 0:                       # well-formed, if meaningless
            assert set(got["lf_mi"]["sb_type"].ravel().tolist()) <= {0, 3, 6, 9, 12} and (got["ext"]["ref_frame"] <= 3).all() and (got["mc_mi"]["ref_list"] <= 1).all()
    head = FM.host_header_bytes(FM.inter(width=72, height=40, reference_mode=FM.SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1)))
    frame = head + tile
    for n in range(len(frame) + 1):       # every truncation length of the whole frame through the frame entry
        rc, _, got = read_frame(frame[:n], 72, 40)
        assert got["guards"] and rc in codes and (rc != 0 or n > len(head)), n


def test_inter_tile_reader_under_address_and_ub_sanitizers_in_a_stand_alone_program():
    """the three tiles of the labelling fixture, whole, at every truncation length and under 200 seeded corruptions each; the tile and every
    output array an allocation of exactly its size"""
    pics = [D.golden_picture(g[0]) for g in D.GOLDEN]
    with tempfile.TemporaryDirectory() as td:
        if not sanitizer_runtime_present(td):
            pytest.skip("this compiler links no address / undefined-behaviour sanitizer runtime")
        req, exe = os.path.join(td, "tiles.bin"), os.path.join(td, "inter_read_san")
        with open(req, "wb") as f:
            f.write(BT.tobytes() + KT.tobytes() + IT.tobytes())
            for p in pics:
                par = params_of(p["W"], p["H"], p["W"] // 8, p["frame"], p["restrict"], p["lrf"], 10)
                f.write(struct.pack("<I", len(p["tile"])) + bytes(par) + p["tile"])
        cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-DCHECK_INTER", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{os.path.join(T.ROOT, 'include')}",
               os.path.join(T.ROOT, "tests", "c", "frame_read_check.c")] + sorted(glob.glob(os.path.join(T.ROOT, "svt-vp9_amd", "host", "*.c"))) + ["-lpthread", "-lm", "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe, req], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.split()[:2] == ["calls", str(sum(len(p["tile"]) + 1 + 200 for p in pics))] and int(r.stdout.split()[3]) >= len(pics)

"""CPU: the key-frame tile reader (svt_hip_tile_read_kf_host, svt-vp9_amd/host/frame_read.c) -- the reference's own tiles
(tests/golden/modes_reference.npz, and the two whole key frames of frame_reference.npz through the header reader first) read back to the
fixture pictures' grids, coefficients and eob maps, byte for byte; round trips through the host writers (tokeniser -> mode info -> bool
coder) on pictures the fixtures do not hold; truncated and corrupted tiles return with every guard intact; the same in a stand-alone
program under the address and undefined-behaviour sanitizers."""
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
import modes_model as MM
import svt_testlib as T
import tokenize_model as TM
from test_frame_read import read as read_header
from test_frame_read import sanitizer_runtime_present

B = T.B
RESULT = B.TILE_READ_RESULT_DTYPE
PAD = 32          # guard elements round every output array
BOOL_TABLES, MODES_TABLES = BM.tables()[1], MM.tables()[1]      # (kept alive: the calls below take their addresses)


def read_tile(tile, W, H, level, stride=None):
    """(rc, lf_mi [rows][stride], qcoeff, eob map, result record, guards intact): the tile in an array of exactly its size, every output
    between guards; the grid's columns beyond mi_cols are guards too"""
    stride = stride or W // 8
    rows, cols, nco, nem = H // 8, W // 8, T.n_sb(W, H) * B.SB_COEFFS, (W // 4) * (H // 4) * 3 // 2
    buf = np.frombuffer(bytes(tile), np.uint8).copy() if len(tile) else np.zeros(1, np.uint8)
    lf = np.full(8 * (rows * stride + 2 * PAD), 0xEE, np.uint8)
    q, em, res = np.full(nco + 2 * PAD, 0x5A5A, np.int16), np.full(nem + 2 * PAD, 0xA5A5, np.uint16), np.full(8 + 2 * PAD, 0x77777777, np.uint32)
    vp = lambda a, o=0: C.c_void_p(a.ctypes.data + o)      # noqa: E731
    rc = B.load().svt_hip_tile_read_kf_host(vp(buf), len(tile), W, H, stride, level, vp(BOOL_TABLES), vp(MODES_TABLES), vp(lf, 8 * PAD), vp(q, 2 * PAD), vp(em, 2 * PAD),
                                             vp(res, 4 * PAD))
    grid = lf[8 * PAD:8 * (PAD + rows * stride)].view(B.LF_MODE_INFO_DTYPE).reshape(rows, stride)
    guards = bool((lf[:8 * PAD] == 0xEE).all() and (lf[8 * (PAD + rows * stride):] == 0xEE).all() and (grid[:, cols:].view(np.uint8) == 0xEE).all() and
                  (q[:PAD] == 0x5A5A).all() and (q[PAD + nco:] == 0x5A5A).all() and (em[:PAD] == 0xA5A5).all() and (em[PAD + nem:] == 0xA5A5).all() and
                  (res[:PAD] == 0x77777777).all() and (res[PAD + 8:] == 0x77777777).all())
    return rc, grid[:, :cols], q[PAD:PAD + nco], em[PAD:PAD + nem], res[PAD:PAD + 8].view(RESULT)[0], guards


def check_reads_back(tile, lf_mi, qcoeff, eob_map, W, H, what, stride=None):
    rc, lf, q, em, res, guards = read_tile(tile, W, H, int(lf_mi["filter_level"][0, 0]), stride)
    assert rc == 0 and guards, (what, B.load().svt_hip_last_error())
    assert lf.tobytes() == np.ascontiguousarray(lf_mi).tobytes(), (what, [f for f in lf.dtype.names if not np.array_equal(lf[f], lf_mi[f])])
    assert np.array_equal(q, qcoeff) and np.array_equal(em, np.asarray(eob_map).view(np.uint16)), what
    origins = sum(1 for r in range(H // 8) for c in range(W // 8) if r % MM.UNITS[int(lf_mi["sb_type"][r, c])] == 0 and c % MM.UNITS[int(lf_mi["sb_type"][r, c])] == 0)
    assert res["leaves"] == origins and res["inter_leaves"] == 0 and res["tile_bytes"] == len(tile) and res["past_end"] == 0, (what, res)
    return res


@pytest.mark.parametrize("name", MM.NAMES)
def test_the_reference_tiles_read_back_to_the_fixture_pictures(name):
    p = MM.fixture_picture(name)
    res = check_reads_back(p["tile"], p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], name)
    assert res["tokens"] == len(MM.host_tokens(name)["tokens"])                # EOB tokens included: the tokeniser's count


@pytest.mark.parametrize("case", [w for w in FM.WHOLE if w[1] == "modes"], ids=[w[0] for w in FM.WHOLE if w[1] == "modes"])
def test_whole_key_frames_header_then_tile(case):
    name, _, picture, _ = case
    _, frame, _, _ = FM.fixture_case(name)
    rc, info, _ = read_header(frame)
    assert rc == 0 and info.params.frame_type == FM.KEY and (info.params.width, info.params.height) == (72, 40)
    p = MM.fixture_picture(picture)
    check_reads_back(frame[info.uncompressed_bytes + info.compressed_bytes:], p["lf_mi"], p["qcoeff"], p["eob_map"], info.params.width, info.params.height, name)


def host_tile(lf, q, emap, W, H):
    tok = TM.host_tokenize_picture(lf, q, emap, W, H, counts=False)
    m = MM.host_modes(lf, emap, tok["tok_off"], W, H)
    assert m["rc"] == 0 and m["n_bools"] != B.MODES_BAD_GRID
    return BM.host_code(tokens=tok["tokens"], bools=m["bools"], segments=[tuple(int(v) for v in s) for s in m["segments"]])[0]


# pictures the fixtures do not hold: one unit wide / high, every leaf type alone (all ten modes occur in the seeded draws), partial SBs
SEEDED = [(8, 8, "random", 1), (8, 136, "random", 2), (136, 8, "random", 3), (16, 80, 6, 4), (200, 72, "random", 5), (64, 128, 12, 6), (72, 72, 0, 7), (96, 32, 9, 8)]


@pytest.mark.parametrize("W,H,kind,seed", SEEDED)
def test_round_trip_through_the_host_writers(W, H, kind, seed):
    lf, q, emap = MM.make_picture(W, H, kind, seed)
    check_reads_back(host_tile(lf, q, emap, W, H), lf, q, emap, W, H, (W, H, kind))


def test_round_trip_of_all_ten_modes_and_dense_cat6_blocks():
    modes = set()
    for W, H, kind, seed in SEEDED:
        lf = MM.make_picture(W, H, kind, seed)[0]
        big = lf[lf["sb_type"] != 0]
        modes |= set(big["pad"][:, 1].tolist()) | set(big["pad"][:, 2].tolist())
    assert modes == set(range(10))
    for W, H, t, seed, kw in MM.DENSE[:4]:                                       # every coefficient non-zero, CAT6 values, full and short blocks
        lf, q, emap = MM.dense_picture(W, H, t, seed, **kw)
        assert np.abs(q).max() >= 67
        check_reads_back(host_tile(lf, q, emap, W, H), lf, q, emap, W, H, (W, H, t, kw))
    lf, q, emap = MM.dense_picture(64, 64, 12, 9, values=(67 + 0x3FFF,))        # the largest extra bits of CAT6
    check_reads_back(host_tile(lf, q, emap, 64, 64), lf, q, emap, 64, 64, "cat6 max")


def test_round_trip_of_the_big_pictures():
    for p in MM.big_pictures():
        check_reads_back(MM.big_host(p["name"])["tile"], p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], p["name"])


def test_a_grid_stride_that_is_not_tight():
    p = MM.fixture_picture("edge_72x40_a")
    check_reads_back(p["tile"], p["lf_mi"], p["qcoeff"], p["eob_map"], p["W"], p["H"], "stride 13", stride=13)


def test_truncated_and_corrupted_tiles_return_with_guards_intact():
    rng = np.random.default_rng(31)
    for name in ("edge_72x40_a", "edge_72x40_b"):
        p = MM.fixture_picture(name)
        tile = p["tile"]
        for n in range(len(tile) + 1):
            rc, _, _, _, res, guards = read_tile(tile[:n], 72, 40, 10)
            assert guards and rc in (0, B.ERR_BAD_PARAMETER, B.ERR_UNSUPPORTED), n
            assert n == len(tile) or rc != 0 or res["past_end"] or res["tile_bytes"] <= n
        for _ in range(200):
            bad = bytearray(tile)
            for _ in range(int(rng.integers(1, 5))):
                bad[int(rng.integers(0, len(bad)))] ^= int(rng.integers(1, 256))
            rc, lf, _, _, _, guards = read_tile(bytes(bad), 72, 40, 10)
            assert guards and rc in (0, B.ERR_BAD_PARAMETER, B.ERR_UNSUPPORTED)
            if rc == 0:                                                          # well-formed, if meaningless
                assert set(lf["sb_type"].ravel().tolist()) <= {0, 3, 6, 9, 12} and (lf["pad"][:, :, 2] <= 9).all()
    lib = B.load()
    assert lib.svt_hip_tile_read_kf_host(None, 4, 72, 40, 9, 10, None, None, None, None, None, None) == B.ERR_BAD_PARAMETER
    assert read_tile(b"\x00\x00", 70, 40, 10, stride=9)[0] == B.ERR_BAD_PARAMETER and read_tile(b"\x00", 72, 40, 64)[0] == B.ERR_BAD_PARAMETER
    assert read_tile(b"\x80\x00\x00", 72, 40, 10)[0] == B.ERR_BAD_PARAMETER           # a set marker bit


def build_check(td, sanitize):
    src = os.path.join(T.ROOT, "svt-vp9_amd")
    exe = os.path.join(td, "tile_read_san" if sanitize else "tile_read_plain")
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-DCHECK_TILES"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) + \
          [f"-I{os.path.join(T.ROOT, 'include')}", os.path.join(T.ROOT, "tests", "c", "frame_read_check.c")] + sorted(glob.glob(os.path.join(src, "host", "*.c"))) + ["-lpthread", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_tile_reader_under_address_and_ub_sanitizers_in_a_stand_alone_program():
    """the two 72x40 fixture tiles, whole, at every truncation length and under 200 seeded corruptions each; tile and output arrays are
    allocations of exactly their size.  Where an up-front probe finds that the host compiler links no sanitizer runtime the test is skipped, visibly."""
    tiles = [MM.fixture_picture(n)["tile"] for n in ("edge_72x40_a", "edge_72x40_b")]
    with tempfile.TemporaryDirectory() as td:
        req = os.path.join(td, "tiles.bin")
        with open(req, "wb") as f:
            f.write(BOOL_TABLES.tobytes() + MODES_TABLES.tobytes())
            for t in tiles:
                f.write(struct.pack("<III", len(t), 72, 40) + t)
        if not sanitizer_runtime_present(td):
            pytest.skip("this compiler links no address / undefined-behaviour sanitizer runtime")
        exe = build_check(td, True)
        assert exe, "the sanitized stand-alone program does not build"
        r = subprocess.run([exe, req], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.split()[:2] == ["calls", str(sum(len(t) + 1 + 200 for t in tiles))] and int(r.stdout.split()[3]) >= len(tiles)

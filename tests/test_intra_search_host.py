"""CPU: the host form of the searched intra stand-in (svt_hip_md_intra_search_picture) against a Python restatement of the rule
include/svtvp9_hip.h states, on random open-loop intra search records; its grids pass the library's own grid check; bad arguments
are refused.  The record layout as the C compiler sees it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import intra_search_model as S
import svt_testlib as T

B = T.B


def test_ois_block_layout_matches_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "svtvp9_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d",sizeof(svt_ois_block),'
           'offsetof(svt_ois_block,uv_sad),offsetof(svt_ois_block,mode),offsetof(svt_ois_block,uv_mode),offsetof(svt_ois_block,pad_),SVT_OIS_PER_SB);return 0;}')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", f"{T.ROOT}/include", os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(td, "s")]).split()]
    assert got == [12, 4, 8, 9, 10, B.OIS_PER_SB] and B.OIS_BLOCK_DTYPE.itemsize == 12
    assert [B.OIS_BLOCK_DTYPE.fields[f][1] for f in ("sad", "uv_sad", "mode", "uv_mode", "pad")] == [0, 4, 8, 9, 10]


def grid_accepted(lf, W, H):
    """the library's grid check (svt_hip_tq_blocks_from_grid: sizes, alignment, transforms, blocks inside the picture)"""
    g = B.TqPicGeom()
    g.width, g.height = W, H
    cap = W * H * 3 // 32
    blocks, pos, cnt = np.zeros(cap, dtype=B.TQ_BLOCK_DTYPE), np.zeros(cap, np.uint32), (C.c_int32 * 4)()
    arr = (C.c_void_p * 1)(lf.ctypes.data)
    return B.load().svt_hip_tq_blocks_from_grid(1, arr, lf.shape[1], C.byref(g), blocks.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), cap, cnt)


@pytest.mark.parametrize("W,H,seed,lam", [(640, 360, 1, 300), (1288, 728, 2, 1000), (1920, 1080, 3, 120), (640, 360, 4, 0), (1288, 728, 5, 5000)])
def test_host_form_equals_the_restatement(W, H, seed, lam):
    ois = S.random_ois(seed, W, H)
    level = 5 + seed
    got = S.host_grid(ois, W, H, lam, level)
    want = S.model_grid(ois, W, H, lam, level)
    assert got.tobytes() == want.tobytes(), int(np.sum(got != want))
    assert grid_accepted(got, W, H) >= 0
    kinds = set(np.unique(got["sb_type"]).tolist())
    assert kinds == {0, 3, 6, 9}, kinds                                          # every block size occurs
    assert not got["is_inter"].any() and not got["skip"].any() and (got["filter_level"] == level).all()
    big = got["sb_type"] >= 3
    assert (got["pad"][..., 1][big] <= 9).all() and (got["pad"][..., 0][big] == 0).all()


def test_parents_without_records_or_outside_the_picture_are_never_chosen():
    W, H = 1288, 728
    ois = S.random_ois(7, W, H, none_share=0.5)
    ois["sad"][:, 84:] = 1000                                                   # 4x4 blocks expensive: parents win wherever they may
    ois["sad"][:, 20:84][ois["sad"][:, 20:84] != S.NONE] = 0
    lf = S.host_grid(ois, W, H, 10, 3)
    assert lf.tobytes() == S.model_grid(ois, W, H, 10, 3).tobytes()
    sb_cols = (W + 63) // 64
    for ur, uc in zip(*np.nonzero(lf["sb_type"] >= 6)):
        n8 = 4 if lf["sb_type"][ur, uc] == 9 else 2
        r0, c0 = ur - ur % n8, uc - uc % n8
        assert r0 + n8 <= H // 8 and c0 + n8 <= W // 8
        sb, r, c = (r0 // 8) * sb_cols + c0 // 8, r0 % 8, c0 % 8
        z = S.zord(c // 4, r // 4) if n8 == 4 else 4 + S.zord(c // 2, r // 2)
        assert ois["sad"][sb, z] != S.NONE
    assert grid_accepted(lf, W, H) >= 0


def test_ties_go_to_the_larger_block_and_sums_do_not_wrap():
    W, H, lam = 64, 64, 100
    ois = np.zeros((1, B.OIS_PER_SB), dtype=B.OIS_BLOCK_DTYPE)
    ois["uv_sad"][:, 84:], ois["uv_mode"][:, 84:] = S.NONE, 0xFF
    ois["sad"][0, :20] = S.NONE                                                # no 16x16 / 32x32 records
    grid = lambda l=lam: S.host_grid(ois, W, H, l, 0)
    assert (grid()["sb_type"] == 3).all()                                      # J8 = lam = J(unit of four 4x4): the 8x8 block
    ois["sad"][0, 20:84] = 1
    assert (grid()["sb_type"] == 0).all()                                      # J8 = lam + 1 > lam: four 4x4 blocks
    ois["sad"][0, 20:84], ois["sad"][0, 4:20] = 0, 3 * lam
    assert (grid()["sb_type"] == 6).all()                                      # J16 = 4 lam = four 8x8 at lam: the 16x16 block
    ois["sad"][0, 0:4] = 15 * lam
    assert (grid()["sb_type"] == 9).all()                                      # J32 = 16 lam = four 16x16 at 4 lam: the 32x32 block
    ois["sad"][0, 0:4] = 15 * lam + 1
    assert (grid()["sb_type"] == 6).all()
    # near UINT32_MAX: J32 = 2^33 + 2 < four 16x16 at lam = 2^32 - 1 each -- in 64 bits
    ois["sad"][0, 4:20], ois["sad"][0, 0:4], ois["uv_sad"][0, 0:4] = 0, S.NONE - 1, 5
    lf = grid(0xFFFFFFFF)
    assert (lf["sb_type"] == 9).all() and lf.tobytes() == S.model_grid(ois, W, H, 0xFFFFFFFF, 0).tobytes()


def test_bad_arguments_are_refused():
    lib = B.load()
    W, H = 128, 64
    ois = S.random_ois(1, W, H)
    lf = np.zeros((H // 8, W // 8), dtype=B.LF_MODE_INFO_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda o=vp(ois), w=W, h=H, lvl=10, out=vp(lf), stride=W // 8: lib.svt_hip_md_intra_search_picture(o, w, h, C.c_uint32(100), lvl, out, stride)
    assert call() == 0
    for bad in (dict(o=None), dict(out=None), dict(w=W + 4), dict(h=H - 2), dict(w=0), dict(h=-8), dict(stride=W // 8 - 1), dict(lvl=-1), dict(lvl=64)):
        assert call(**bad) == -1, bad                                          # SVT_HIP_ERR_BAD_PARAMETER
        assert b"md_intra_search" in lib.svt_hip_last_error()
    # the device entries validate their arguments before they touch a device: no context, no records
    planes = B.YuvPlanes()
    assert lib.svt_hip_intra_search_device(None, C.byref(planes), W, H, vp(ois)) == -1
    assert b"intra_search" in lib.svt_hip_last_error()
    assert lib.svt_hip_md_intra_search_device(None, vp(ois), W, H, C.c_uint32(100), 10, vp(lf), W // 8) == -1

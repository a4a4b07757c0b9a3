"""GPU: the intra path where its other tests do not reach (every picture at most 136x72).
  * the intra encode pass (svt_hip_encdec_intra_device) on every case of the recorded reference (tests/golden/intra_reference.npz: what the
    reference's own functions made of thin pictures and of the ends of the q range) -- against the recorded bytes with the loop filter off,
    against the oracle chain with the key-frame flags;
  * thin pictures (cell grids 1x1, 5x1, 1x5, 3x2 ...: the three branches of the wavefront's ticket -> cell mapping, 2 x 2 cell groups cut by
    the picture edge, mi_rows == 1, chroma planes four samples wide) on 1, 2, 5 and the default number of workers, and with a grid wider than
    the picture with random bytes behind every row.  tests/test_intra_wavefront.py checks the mapping itself on the host;
  * the open-loop search (svt_hip_intra_search_device) on pictures without a whole 64x64 SB and on flat, 0 / 255 block and 0 / 255 noise
    content, every SB against the oracle model; the device grid builder on those records against its host form and the model; the chain
    search -> device grid -> intra pass against the oracle chain.
No entry point refuses any of these sizes: svt_hip_encdec_work_create, svt_hip_encdec_intra_device and the two search entries take every
picture whose dimensions are multiples of 8, from 8x8 (test_smallest_picture_is_accepted asserts it)."""
import ctypes as C
import functools

import numpy as np
import pytest

import encdec_model as M
import intra_search_model as S
import svt_testlib as T
from test_gpu_encdec import flags_of, masks_equal
from test_gpu_intra import KEY, check, run_intra
from test_gpu_intra_search import device_grid, device_search

B = T.B
pytestmark = pytest.mark.gpu
CASES = {c[0]: c for c in M.INTRA_GOLDEN_CASES}
NO_LF = dict(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=0, loop_filter=0)


@pytest.fixture(scope="module")
def ctx():
    lib = B.load()
    c = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(c), 0))
    yield c
    lib.svt_hip_ctx_destroy(c)


def thresholds():
    thr = B.LfThresh()
    B.load().svt_hip_lf_thresh_init(C.byref(thr), 0)
    return thr


def chain_equal(ctx, src, mi, q_index, cfg, seed=0):
    """the pass on the grid `mi` (any stride) against the oracle chain: every output, the reconstruction with its border"""
    H, W = src[0].shape
    flags, thr = flags_of(**cfg), thresholds()
    rec_init = M.RefPic(W, H)
    rec_init.buf[:] = np.random.default_rng(seed).integers(0, 256, rec_init.buf.size, dtype=np.uint8)
    rec0 = M.RefPic(W, H)
    rec0.buf[:] = rec_init.buf
    g = run_intra(ctx, src, mi, q_index, flags, thr, rec_init)
    assert g["rc"] == 0                                                  # svt_hip_encdec_work_status: a well-formed grid
    o = M.oracle_intra_chain(src, mi, q_index, flags, thr, recon_init=rec0)
    assert np.array_equal(g["pred"], np.concatenate([p.ravel() for p in o["pred"]])), "prediction"
    assert np.array_equal(g["q"], o["qcoeff"]) and np.array_equal(g["dq"], o["dqcoeff"]), "coefficients"
    assert np.array_equal(g["emap"], o["eob_map"]), "eob map"
    assert np.array_equal(g["lf"]["skip"][:, :W // 8], o["lf_mi"]["skip"][:, :W // 8]), "skip flags"
    if flags.apply_loop_filter:
        assert masks_equal(g["lfm"].view(B.LF_MASK_DTYPE).reshape(o["lfm"].shape), o["lfm"]), "masks"
    assert np.array_equal(g["rec"], o["rec"].buf), ("reconstruction", int(np.sum(g["rec"] != o["rec"].buf)))
    return g, o


def first_difference(name, key, got, want, W, H):
    """case, plane and coordinates of the first differing sample / entry"""
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return None
    i = int(bad[0])
    if key in ("pred", "rec"):
        ny, nc = W * H, W * H // 4
        plane, j, w = (0, i, W) if i < ny else (1, i - ny, W // 2) if i < ny + nc else (2, i - ny - nc, W // 2)
        return f"{name} {key}: {len(bad)} differ, first in plane {plane} at x {j % w} y {j // w}: {int(got[i])} for {int(want[i])}"
    return f"{name} {key}: {len(bad)} differ, first at index {i}: {int(got[i])} for {int(want[i])}"


def test_smallest_picture_is_accepted(ctx):
    lib = B.load()
    work = C.c_void_p()
    assert lib.svt_hip_encdec_work_create(ctx, 1, 8, 8, C.byref(work)) == 0
    lib.svt_hip_encdec_work_destroy(ctx, work)
    assert lib.svt_hip_encdec_work_create(ctx, 1, 8, 4, C.byref(work)) != 0


# ---- 1. the recorded reference ----
@pytest.mark.parametrize("name", list(CASES))
def test_pass_equals_the_recorded_reference(ctx, name):
    """loop filter off: prediction, interior reconstruction, qcoeff, dqcoeff and eob map are the bytes the reference's functions gave"""
    _, W, H, seed, q, kind = CASES[name]
    want = M.intra_golden()[name]
    src, mi = M.intra_golden_inputs(CASES[name])
    assert np.ascontiguousarray(mi).tobytes() == want["mi"].tobytes() and np.array_equal(np.concatenate([p.ravel() for p in src]), want["src"])
    g, _ = chain_equal(ctx, src, mi, q, NO_LF, seed)
    got = dict(pred=g["pred"], rec=np.concatenate([p.ravel() for p in M.RefPic(W, H).interior(g["rec"])]), qcoeff=g["q"], dqcoeff=g["dq"], eob_map=g["emap"])
    for k in M.INTRA_GOLDEN_KEYS:
        assert got[k].shape == want[k].shape
        assert np.array_equal(got[k], want[k]), first_difference(name, k, got[k], want[k], W, H)


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_cases_as_key_frames_equal_the_oracle_chain(ctx, name):
    """the same pictures with deblocking and border (the check() of tests/test_gpu_intra.py, which also asserts svt_hip_encdec_work_status
    == 0); at the ends of the q range the reconstruction is not required to be near the source"""
    _, W, H, seed, q, kind = CASES[name]
    g, o = check(ctx, W, H, seed, q, KEY, sizes=M.INTRA_GOLDEN_SIZES, src=M.intra_content(W, H, seed, kind), quality=name.startswith("thin_"))
    assert g["rc"] == 0
    assert np.array_equal(o["lf_mi"]["sb_type"], M.intra_golden_inputs(CASES[name])[1]["sb_type"])     # the fixture's partition


# ---- 2. thin pictures: worker counts, a wider grid ----
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("name", ["thin_8x8", "thin_8x72", "thin_72x8", "thin_24x40"])
def test_thin_pictures_on_few_workers(ctx, name, n):
    """svt_hip_ctx_set_intra_workgroups caps the number of 64-lane workers: one worker walks the tickets alone, two share a workgroup,
    five fill one workgroup and start a second (the default -- min(2 per CU, 3 per cell) -- runs in the tests above: 3 workers at 8x8)"""
    lib = B.load()
    _, W, H, seed, q, kind = CASES[name]
    src, mi = M.intra_golden_inputs(CASES[name])
    want = M.intra_golden()[name]
    try:
        B.check(lib.svt_hip_ctx_set_intra_workgroups(ctx, n))
        g, _ = chain_equal(ctx, src, mi, q, KEY, seed)
        h, _ = chain_equal(ctx, src, mi, q, NO_LF, seed)
    finally:
        B.check(lib.svt_hip_ctx_set_intra_workgroups(ctx, 0))
    assert np.array_equal(h["q"], want["qcoeff"]) and np.array_equal(h["pred"], want["pred"])
    assert np.array_equal(np.concatenate([p.ravel() for p in M.RefPic(W, H).interior(h["rec"])]), want["rec"])


@pytest.mark.parametrize("name", ["thin_24x40", "thin_8x8"])
def test_thin_picture_with_a_wider_grid(ctx, name):
    """mi_stride = mi_cols + 3, random bytes behind every row of the grid: nothing of them is read"""
    _, W, H, seed, q, kind = CASES[name]
    src, tight = M.intra_golden_inputs(CASES[name])
    mi = np.frombuffer(np.random.default_rng(seed).integers(0, 256, (H // 8) * (W // 8 + 3) * B.LF_MODE_INFO_DTYPE.itemsize, dtype=np.uint8).tobytes(),
                       B.LF_MODE_INFO_DTYPE).reshape(H // 8, W // 8 + 3).copy()
    mi[:, :W // 8] = tight
    g, _ = chain_equal(ctx, src, mi, q, KEY, seed)
    assert g["lf"][:, W // 8:].tobytes() == mi[:, W // 8:].tobytes()                 # ... and nothing written
    want = M.intra_golden()[name]
    assert np.array_equal(g["q"], want["qcoeff"]) and np.array_equal(g["pred"], want["pred"])


# ---- 3., 4. the open-loop search and the grid built from its records ----
SEARCH = [(8, 8, "nat", 0), (8, 72, "nat", 0), (72, 8, "nat", 0), (72, 40, "nat", 0), (136, 72, "nat", 0), (72, 40, "nat", 24),
          (72, 40, "flat", 0), (136, 72, "flat", 0), (72, 40, "blocks", 0), (136, 72, "blocks", 0), (72, 40, "noise", 0), (136, 72, "noise", 0)]


@functools.lru_cache(maxsize=None)
def search_model(W, H, kind):
    """(source, the oracle model's records of every SB): computed once per picture, never written to"""
    src = M.intra_content(W, H, 7, kind)
    want = S.oracle_ois(src)
    want.setflags(write=False)
    return src, want


def flat_share(ois, W, H):
    """share of the records inside the picture whose luma (and, for blocks >= 8x8, chroma) cost is 0 with mode 0"""
    inside = S.inside_mask(W, H)
    r = ois[inside]
    has_uv = r["uv_sad"] != S.NONE
    ok = (r["sad"] == 0) & (r["mode"] == 0) & (~has_uv | ((r["uv_sad"] == 0) & (r["uv_mode"] == 0)))
    return float(ok.mean())


@pytest.mark.parametrize("W,H,kind,stride_pad", SEARCH)
def test_search_records_of_small_and_synthetic_pictures(ctx, W, H, kind, stride_pad):
    src, want = search_model(W, H, kind)
    inside = S.inside_mask(W, H)
    if kind == "flat":
        # every block but the ones at the picture's origin (which see only the 127 / 129 constants) sees the flat value through DC: cost 0,
        # and among the modes that tie at 0 the key sad << 4 | mode must give mode 0.  On the model first.
        assert flat_share(want, W, H) >= 0.9
    _, got = device_search(ctx, src, stride_pad)
    for sb in range(T.n_sb(W, H)):
        assert got[sb].tobytes() == want[sb].tobytes(), (sb, np.nonzero(got[sb] != want[sb])[0][:8].tolist())
    assert (got["sad"][~inside] == S.NONE).all() and (got["sad"][inside] != S.NONE).all()
    if kind == "flat":
        assert flat_share(got, W, H) >= 0.9
    if W < 64 and H < 64:
        assert not inside[:, :4].any()                                               # no 32x32 block, let alone a whole SB


@pytest.mark.parametrize("W,H,kind,stride_pad", [s for s in SEARCH if not s[3]])
def test_device_grid_of_small_and_synthetic_pictures(ctx, W, H, kind, stride_pad):
    lib = B.load()
    src, want = search_model(W, H, kind)
    d_ois, ois = device_search(ctx, src)
    assert ois.tobytes() == want.tobytes()
    for q in (0, 60, 255):
        ac = lib.svt_hip_vp9_ac_step(q)
        lam, level = 4 * ac, lib.svt_hip_lf_level_from_q(ac, 1)
        stride = W // 8 + (3 if q else 0)
        got = device_grid(ctx, d_ois, W, H, lam, level, stride)
        assert got[:, :W // 8].tobytes() == S.host_grid(want, W, H, lam, level, stride)[:, :W // 8].tobytes()
        assert got[:, :W // 8].tobytes() == S.model_grid(want, W, H, lam, level).tobytes()
        assert (got[:, W // 8:].view(np.uint8) == 0x33).all()                        # nothing written beyond the picture's units


# ---- 5. search -> device grid -> intra pass ----
@pytest.mark.parametrize("W,H,kind,q", [(72, 40, "nat", 60), (8, 72, "blocks", 0)])
def test_searched_chain_equals_the_oracle_chain(ctx, W, H, kind, q):
    lib = B.load()
    src, want = search_model(W, H, kind)
    d_ois, ois = device_search(ctx, src)
    ac = lib.svt_hip_vp9_ac_step(q)
    lam, level = 4 * ac, lib.svt_hip_lf_level_from_q(ac, 1)
    mi = device_grid(ctx, d_ois, W, H, lam, level)
    assert mi.tobytes() == S.host_grid(want, W, H, lam, level).tobytes()
    g, o = chain_equal(ctx, src, mi, q, KEY)
    assert o["eob_map"].any()

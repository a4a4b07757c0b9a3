"""CPU: the entropy pass's host half (host/entropy_host.c, rules in csrc/entropy_core.h) -- svt_hip_entropy_picture against the reference's
bytes (the key frames of tests/golden/frame_reference.npz whole; the inter pictures of tests/golden/md_inter_reference.npz as host header
|| the reference's tile), the gate's rules at both sides of every threshold, the limits and the workspace's size, the compound references
and the deliverability report against the recorded values, over-budget pictures, refusals, and the host form under the address and
undefined-behaviour sanitizers in a stand-alone program."""
import ctypes as C
import glob
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import entropy_model as E
import frame_model as FM
import md_inter_model as D
import modes_inter_model as IM
import svt_testlib as T
from test_frame_read import sanitizer_runtime_present

B = T.B
BAD, OVER = B.MODES_BAD_GRID, B.BOOL_SIZE_OVERFLOW
KEYS = [w for w in FM.WHOLE if w[1] == "modes"]
INTER = [g[0] for g in D.GOLDEN]


def test_exports_and_sizes():
    lib = B.load()
    for s in ("svt_hip_entropy_batch_device", "svt_hip_entropy_picture", "svt_hip_entropy_work_create", "svt_hip_entropy_deliverable"):
        assert hasattr(lib, s) and s in B.EXPORTS, s
    src = ('#include <stdio.h>\n#include "svtvp9_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu",sizeof(svt_entropy_picture),sizeof(svt_entropy_result),'
           'sizeof(svt_entropy_limits),sizeof(svt_entropy_buffers),sizeof(svt_entropy_host_detail));return 0;}')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", f"{T.ROOT}/include", os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(td, "s")]).split()]
    assert sizes == [C.sizeof(B.EntropyPicture), B.ENTROPY_RESULT_DTYPE.itemsize, C.sizeof(B.EntropyLimits), C.sizeof(B.EntropyBuffers), C.sizeof(B.EntropyHostDetail)]


@pytest.mark.parametrize("case", KEYS, ids=[w[0] for w in KEYS])
def test_key_pictures_equal_the_reference_frames(case):
    name, _, picture, fp = case
    got = E.host_entropy(E.key_picture(picture), fp, counts=True)
    want = bytes(FM.fixture()[f"frame|{name}"])
    assert got["rc"] == 0 and got["packet"] == want and got["size"] == len(want)
    r = got["result"]
    assert r["flags"] == 0 and r["tile_bytes"] == len(want) - got["header_bytes"] and r["tokens"] > 0 and r["mode_bools"] > 0
    assert (r["inter_leaves"], r["newmv_leaves"], r["unfaithful_leaves"]) == (0, 0, 0)
    assert got["stream_bools"] > r["mode_bools"] and int(got["counts"].sum()) == r["tokens"]
    # the four show-existing bytes of a packet flagged EB_BUFFERFLAG_SHOW_EXT
    trailer = b"".join(FM.show_existing(s) for s in (0, 3, 7, 3))
    assert E.host_entropy(E.key_picture(picture), fp, trailer=trailer)["packet"] == want + trailer


@pytest.mark.parametrize("name", INTER)
def test_inter_pictures_equal_host_header_and_the_reference_tile(name):
    p, fp, want = E.golden_inter(name)
    got = E.host_entropy(p, fp)
    assert got["rc"] == 0 and got["packet"] == want
    r = got["result"]
    assert r["flags"] == 0 and r["unfaithful_leaves"] == 0 and r["inter_leaves"] > 0 and r["tile_bytes"] == len(p["tile"])
    labels = D.host_md_inter(p, ref_mask=0, want_cand=False)
    assert (r["inter_leaves"], r["newmv_leaves"], r["unfaithful_leaves"]) == labels["status"][:3]


# (what, total, max_tokens, n_bools, capacity, status, size, max_tile_bytes) -> flags; phase A's part of them
OK4 = (5, 2, 0, 0)
GATE = (
    ("total = max_tokens", 100, 100, 50, 60, OK4, 30, 40, 0),
    ("total = max_tokens + 1", 101, 100, 50, 60, OK4, 30, 40, B.ENT_TOKENS_OVER),
    ("bools = capacity", 100, 100, 60, 60, OK4, 30, 40, 0),
    ("bools = capacity + 1", 100, 100, 61, 60, OK4, 30, 40, B.ENT_MODE_BOOLS_OVER),
    ("status word 2 is 0, key picture", 100, 100, 60, 60, None, 30, 40, 0),
    ("status word 2 is 1", 100, 100, 60, 60, (5, 2, 1, 0), 30, 40, B.ENT_UNFAITHFUL_MV),
    ("bad grid in n_bools", 100, 100, BAD, 60, OK4, 30, 40, B.ENT_BAD_GRID),
    ("bad grid in n_bools, key picture", 100, 100, BAD, 60, None, 30, 40, B.ENT_BAD_GRID),
    ("bad grid in status word 0", 100, 100, 50, 60, (BAD, 2, 0, 0), 30, 40, B.ENT_BAD_GRID),
    ("bad grid in status word 1", 100, 100, 50, 60, (5, BAD, 0, 0), 30, 40, B.ENT_BAD_GRID),
    ("bad grid in status word 2", 100, 100, 50, 60, (5, 2, BAD, 0), 30, 40, B.ENT_BAD_GRID),
    ("bad grid in status word 3", 100, 100, 50, 60, (5, 2, 0, BAD), 30, 40, B.ENT_BAD_GRID),
    ("bad grid everywhere", 100, 100, BAD, 60, (BAD,) * 4, 30, 40, B.ENT_BAD_GRID),
    ("size = capacity", 100, 100, 50, 60, OK4, 40, 40, 0),
    ("size = capacity + 1", 100, 100, 50, 60, OK4, 41, 40, B.ENT_TILE_OVER),
    ("the bool coder's overflow", 100, 100, 50, 60, OK4, OVER, 40, B.ENT_STREAM_OVER),
    ("two phase-A reasons", 101, 100, 61, 60, (5, 2, 3, 0), 30, 40, B.ENT_TOKENS_OVER | B.ENT_MODE_BOOLS_OVER | B.ENT_UNFAITHFUL_MV),
    ("phase A hides phase B", 101, 100, 50, 60, OK4, OVER, 40, B.ENT_TOKENS_OVER),
    ("everything zero", 0, 0, 0, 0, (0, 0, 0, 0), 0, 0, 0),
)
PHASE_B = B.ENT_STREAM_OVER | B.ENT_TILE_OVER


@pytest.mark.parametrize("case", GATE, ids=[g[0] for g in GATE])
def test_gate_rules(case):
    what, total, max_tokens, n_bools, cap, status, size, max_tile, flags = case
    a, got, out, r = E.gate(total, max_tokens, n_bools, cap, status, size, max_tile)
    assert got == flags and a == flags & ~PHASE_B, what
    assert out == (OVER if flags else size) and r["tile_bytes"] == (0 if flags else size)
    assert r["tokens"] == total and r["mode_bools"] == n_bools and r["pad"] == 0
    counted = status is not None and BAD not in status
    assert (r["inter_leaves"], r["newmv_leaves"], r["unfaithful_leaves"]) == (tuple(status[:3]) if counted else (0, 0, 0))


@pytest.mark.parametrize("size", [(72, 40), (136, 72), (3840, 2160), (8, 8), (4096, 4096)])
def test_limits_worst_equals_the_capacity_functions(size):
    lib = B.load()
    W, H = size
    lim = E.limits(W, H, 16)
    tokens = lib.svt_hip_tokenize_capacity(W, H)
    bools = lib.svt_hip_boolcode_bools_capacity(tokens) + lib.svt_hip_modes_inter_bools_capacity(W, H)
    assert (lim.max_pics, lim.max_tokens, lim.max_bools, lim.max_tile_bytes) == (16, tokens, bools, lib.svt_hip_boolcode_capacity(bools))
    assert lib.svt_hip_modes_inter_bools_capacity(W, H) >= lib.svt_hip_modes_bools_capacity(W, H)
    bad = E.limits(60, 40, 1)
    assert (bad.max_pics, bad.max_tokens, bad.max_bools, bad.max_tile_bytes) == (0, 0, 0, 0)


def test_work_bytes_formula_monotony_and_refusals():
    lib = B.load()

    def nbytes(W=136, H=72, stride=17, **kw):
        lim = E.limits(W, H, 1, **kw)
        return int(lib.svt_hip_entropy_work_bytes(W, H, stride, C.byref(lim)))
    base = dict(max_pics=2, max_tokens=1000, max_bools=30000, max_tile_bytes=5000)
    up = lambda n: (n + 15) // 16 * 16      # noqa: E731
    per_picture = up(4 * 34 * 18 * 3 // 2) + up(4 * (3 * 2 + 1)) + up(4 * 1000) + up(12 * 9 * 17) + up(2 * 17 * 9 * 111) + up(12 * 6 * 256) + up(5000) + 64
    assert nbytes(**base) == 2 * per_picture
    for field, step in (("max_pics", 1), ("max_tokens", 4), ("max_tile_bytes", 16)):
        assert nbytes(**dict(base, **{field: base[field] + step})) > nbytes(**base), field
        assert nbytes(**dict(base, **{field: base[field] + 10 * step})) > nbytes(**dict(base, **{field: base[field] + step})), field
    # max_bools sizes the context's bool-coder scratch, not the slab: it may not shrink it
    assert nbytes(**dict(base, max_bools=60000)) >= nbytes(**base)
    assert nbytes(stride=24, **base) > nbytes(**base)
    assert nbytes(**dict(base, max_pics=0)) == 0 and nbytes(**dict(base, max_pics=33)) == 0 and nbytes(stride=16, **base) == 0 and nbytes(W=60, **base) == 0
    # the bool coder's 32-bit bit positions: 7 * (max_bools + 33) < 2^32
    edge = (1 << 32) // 7 - 33
    assert 7 * (edge + 33) < 1 << 32 <= 7 * (edge + 34)
    assert nbytes(**dict(base, max_bools=edge)) > 0 and nbytes(**dict(base, max_bools=edge + 1)) == 0
    assert lib.svt_hip_entropy_work_bytes(136, 72, 17, None) == 0
    # the worst case of the workload's picture is refused by that rule at no size this project codes, and is large
    lim = E.limits(3840, 2160, 1)
    assert int(lib.svt_hip_entropy_work_bytes(3840, 2160, 480, C.byref(lim))) > 300 << 20


def recorded_compound_refs():
    out = []
    for name in IM.NAMES:
        fr = IM.fixture_picture(name)["frame"]
        out.append((fr["sign_bias"], fr["comp_fixed_ref"], fr["comp_var_ref"]))
    for name in INTER:
        fr = D.golden_picture(name)["frame"]
        out.append((fr["sign_bias"], fr["comp_fixed_ref"], fr["comp_var_ref"]))
    return out


def test_compound_refs_match_the_recorded_values():
    lib = B.load()
    seen = set()
    for bias, fixed, var in recorded_compound_refs():
        sb, f, v = (C.c_uint8 * 4)(*bias), C.c_uint8(0), (C.c_uint8 * 2)()
        lib.svt_hip_compound_refs_from_sign_bias(sb, C.byref(f), v)
        assert (f.value, tuple(v)) == (fixed, tuple(var)), bias
        seen.add(tuple(bias))
    assert len(seen) >= 3
    for bias in ((0, 1, 0, 0), (0, 1, 1, 0), (0, 0, 1, 1), (1, 1, 1, 1)):      # the rule over the biases the fixtures do not hold
        sb, f, v = (C.c_uint8 * 4)(*bias), C.c_uint8(0), (C.c_uint8 * 2)()
        lib.svt_hip_compound_refs_from_sign_bias(sb, C.byref(f), v)
        fr = IM.frame(sign_bias=bias)
        assert (f.value, tuple(v)) == (fr["comp_fixed_ref"], tuple(fr["comp_var_ref"]))


def test_deliverable_reports_what_a_decoder_needs():
    lib = B.load()
    cases = dict(FM.CASES)
    rep = lambda p: int(lib.svt_hip_entropy_deliverable(C.byref(FM.struct(p))))      # noqa: E731
    assert rep(cases["q0"]) & B.ENT_LOSSLESS and not rep(cases["q255"]) & B.ENT_LOSSLESS
    assert rep(dict(cases["q0"], uv_ac_delta_q=1)) & B.ENT_LOSSLESS == 0
    assert rep(cases["inter_single"]) == B.ENT_NEEDS_BACKWARD_ADAPTATION
    assert rep(cases["inter_context_flags"]) == 0 and rep(cases["inter_error_resilient"]) == 0
    both = B.ENT_COMP_FLAG_MISMATCH | B.ENT_REFERENCE_MODE_UNREAD
    assert rep(FM.worst_params()[1]) & both == both
    assert rep(FM.worst_params()[0]) & both == 0                                      # an intra-only picture codes neither
    assert rep(cases["inter_select_altref_bias"]) & both == 0
    assert rep(cases["inter_single_comp_allowed"]) & both == B.ENT_COMP_FLAG_MISMATCH
    assert rep(dict(cases["inter_select_altref_bias"], allow_comp_inter_inter=0)) & both == B.ENT_COMP_FLAG_MISMATCH
    # the reader's own report agrees on every case it can parse
    for name, p in FM.CASES:
        info = B.FrameReadInfo()
        frame = FM.host_header_bytes(p)
        buf = np.frombuffer(frame, np.uint8).copy()
        lr, lm = (C.c_int8 * 4)(*p["last_ref_deltas"]), (C.c_int8 * 2)(*p["last_mode_deltas"])
        if lib.svt_hip_frame_read_header_host(buf.ctypes.data, len(frame), lr, lm, C.byref(info)) == 0:
            assert bool(rep(p) & B.ENT_NEEDS_BACKWARD_ADAPTATION) == bool(info.needs_backward_adaptation), name
            assert bool(rep(p) & B.ENT_LOSSLESS) == bool(info.lossless), name


def budgets(got, **delta):
    r = got["result"]
    v = dict(max_tokens=r["tokens"], max_bools=got["stream_bools"], max_tile_bytes=r["tile_bytes"])
    for k, d in delta.items():
        v[k] += d
    return v


@pytest.mark.parametrize("name", ["key:edge_72x40_b", "mix_136x72_select_hp"])
def test_over_budget_pictures_are_withheld_and_exact_budgets_ship(name):
    if name.startswith("key:"):
        p, fp = E.key_picture(name[4:]), next(w[3] for w in KEYS if w[2] == name[4:])
    else:
        p, fp, _ = E.golden_inter(name)
    W, H = p["W"], p["H"]
    full = E.host_entropy(p, fp)
    exact = E.host_entropy(p, fp, E.limits(W, H, **budgets(full)))
    assert exact["rc"] == 0 and exact["packet"] == full["packet"] and exact["result"] == full["result"]
    empty = len(E.empty_stream_bytes())
    for field, flag, phase_a in (("max_tokens", B.ENT_TOKENS_OVER, True), ("max_bools", B.ENT_STREAM_OVER, False), ("max_tile_bytes", B.ENT_TILE_OVER, False)):
        got = E.host_entropy(p, fp, E.limits(W, H, **budgets(full, **{field: -1})))
        r = got["result"]
        assert got["rc"] == 0 and got["packet"] is None and got["size"] == B.FRAME_SIZE_NONE and r["flags"] == flag, field
        assert r["tile_bytes"] == 0 and r["tokens"] == full["result"]["tokens"] and r["mode_bools"] == full["result"]["mode_bools"]
        assert got["coded_size"] == (empty if phase_a else OVER if field == "max_bools" else full["result"]["tile_bytes"])


def test_malformed_and_unfaithful_pictures_are_withheld():
    from test_md_inter import put, uniform
    p, fp, _ = E.golden_inter("mix_136x72_single_restrict")
    bad = dict(p, lf_mi=p["lf_mi"].copy())
    bad["lf_mi"]["sb_type"][0, 0] = 1
    got = E.host_entropy(bad, fp)
    assert got["rc"] == 0 and got["packet"] is None and got["result"]["flags"] == B.ENT_BAD_GRID and got["result"]["mode_bools"] == BAD
    key = E.key_picture("edge_72x40_a")
    bad = dict(key, lf_mi=key["lf_mi"].copy())
    bad["lf_mi"]["sb_type"][0, 0] = 1
    assert E.host_entropy(bad, KEYS[0][3])["result"]["flags"] == B.ENT_BAD_GRID
    odd = E.zero_coefficients(uniform(136, 72, IM.frame()))
    put(odd, (0, 1), (8, 8)), put(odd, (1, 1), (9, 8))
    got = E.host_entropy(odd, E.inter_params(odd))
    assert got["packet"] is None and got["result"]["flags"] == B.ENT_UNFAITHFUL_MV and got["result"]["unfaithful_leaves"] == 1
    assert got["coded_size"] == len(E.empty_stream_bytes())
    hp = E.host_entropy(odd, E.inter_params(dict(odd, frame=IM.frame(allow_hp=1))))
    assert hp["result"]["flags"] == 0 and hp["packet"] is not None and hp["result"]["newmv_leaves"] >= 1


def test_host_form_refusals():
    p, fp, _ = E.golden_inter("edge_72x40_select")
    key = E.key_picture("edge_72x40_a")
    kp = KEYS[0][3]
    assert E.host_entropy(p, fp, trailer=b"12345")["rc"] == -1
    assert E.host_entropy(dict(p, lrf=(0, 3)), fp)["rc"] == -1 and E.host_entropy(dict(p, lrf=(1, 4)), fp)["rc"] == -1
    assert E.host_entropy(dict(p, mc_mi=None), fp)["rc"] == -1                     # an inter picture without its prediction grid
    assert E.host_entropy(dict(key, mc_mi=p["mc_mi"]), kp)["rc"] == -1              # a key picture with one
    assert E.host_entropy(p, dict(fp, color_space=7))["rc"] == -1 and E.host_entropy(p, dict(fp, y_dc_delta_q=16))["rc"] == -1
    assert E.host_entropy(p, dict(fp, width=60, render_width=60))["rc"] == -1 and E.host_entropy(p, dict(fp, height=8200, render_height=8200))["rc"] == -1
    assert E.host_entropy(p, fp, E.limits(72, 40, max_bools=(1 << 32) // 7))["rc"] == -1
    assert E.host_entropy(key, kp)["rc"] == 0 and E.host_entropy(p, fp)["rc"] == 0


# ---- the host form under the sanitizers, in a stand-alone program --------------------------------------------------------------------
def request(cases):
    """[(picture, frame parameters, limits, trailer)] -> the bytes tests/c/entropy_check.c reads"""
    tb, tm, ti = E.tables()
    out = [struct.pack("<I", len(cases)), tb.tobytes(), tm.tobytes(), ti.tobytes()]
    for p, fp, lim, trailer in cases:
        lf = np.ascontiguousarray(p["lf_mi"])
        mc = np.ascontiguousarray(p["mc_mi"]) if p.get("mc_mi") is not None else None
        q, em = np.ascontiguousarray(p["qcoeff"], np.int16), np.ascontiguousarray(p["eob_map"], np.uint16)
        s = E.fill_struct(B.EntropyPicture(), (None, None, None, None), fp, p.get("lrf", (1, 3)), p.get("restrict", 0), trailer)
        out.append(struct.pack("<iIIII", lf.shape[1], lim.max_tokens, lim.max_bools, lim.max_tile_bytes, 0 if mc is None else mc.nbytes))
        out.append(bytes(s))
        out.append(struct.pack("<III", lf.nbytes, q.nbytes, em.nbytes))
        out += [lf.tobytes(), mc.tobytes() if mc is not None else b"", q.tobytes(), em.tobytes()]
    return b"".join(out)


def test_host_form_under_address_and_ub_sanitizers_in_a_stand_alone_program():
    """the fixture pictures and the over-budget, malformed and unfaithful cases, every input in an allocation of exactly its bytes; the
    program prints size, flags and a checksum of every packet, compared here with the library's.  Skipped, visibly, where the host
    compiler links no sanitizer runtime."""
    from test_md_inter import put, uniform
    cases = []
    for _, _, picture, fp in KEYS:
        p = E.key_picture(picture)
        cases.append((p, fp, E.limits(p["W"], p["H"]), b"\x88\x8b"))
    for name in INTER:
        p, fp, _ = E.golden_inter(name)
        full = E.host_entropy(p, fp)
        cases.append((p, fp, E.limits(p["W"], p["H"]), b""))
        cases.append((p, fp, E.limits(p["W"], p["H"], **budgets(full)), b""))
        for field in ("max_tokens", "max_bools", "max_tile_bytes"):
            cases.append((p, fp, E.limits(p["W"], p["H"], **budgets(full, **{field: -1})), b""))
        cases.append((p, fp, E.limits(p["W"], p["H"], max_tokens=0, max_bools=0, max_tile_bytes=0), b""))
    # a rectangular sb_type on a key picture (on an inter picture the labelling's svt_mdi_label_unit shifts by the level -1 of such a type before
    # it refuses it: a finding of this test in md_inter_core.h, whose text this file's subject does not own)
    p = E.key_picture("edge_72x40_a")
    bad = dict(p, lf_mi=p["lf_mi"].copy())
    bad["lf_mi"]["sb_type"][1, 1] = 2
    cases.append((bad, KEYS[0][3], E.limits(p["W"], p["H"]), b""))
    odd = E.zero_coefficients(uniform(136, 72, IM.frame()))
    put(odd, (0, 1), (8, 8)), put(odd, (1, 1), (9, 8))
    cases.append((odd, E.inter_params(odd), E.limits(136, 72), b""))
    wide = D.with_stride(D.golden_picture("mix_136x72_select_hp"), 7, 3)
    cases.append((wide, E.golden_inter("mix_136x72_select_hp")[1], E.limits(136, 72), b""))
    want = []
    for p, fp, lim, trailer in cases:
        got = E.host_entropy(p, fp, lim, trailer=trailer)
        assert got["rc"] == 0
        want.append((got["size"], got["result"]["flags"], sum(got["packet"] or b"") & 0xFFFFFFFF))
    assert {w[1] for w in want} >= {0, B.ENT_BAD_GRID, B.ENT_TOKENS_OVER, B.ENT_UNFAITHFUL_MV, B.ENT_STREAM_OVER, B.ENT_TILE_OVER}
    with tempfile.TemporaryDirectory() as td:
        if not sanitizer_runtime_present(td):
            pytest.skip("this compiler links no address / undefined-behaviour sanitizer runtime")
        req = os.path.join(td, "cases.bin")
        with open(req, "wb") as f:
            f.write(request(cases))
        exe = os.path.join(td, "entropy_san")
        src = os.path.join(T.ROOT, "svt-vp9_amd")
        cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{os.path.join(T.ROOT, 'include')}",
               os.path.join(T.ROOT, "tests", "c", "entropy_check.c")] + sorted(glob.glob(os.path.join(src, "host", "*.c"))) + ["-lpthread", "-lm", "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe, req], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = [tuple(int(v) for v in line.split()) for line in r.stdout.strip().splitlines()]
        assert got == want

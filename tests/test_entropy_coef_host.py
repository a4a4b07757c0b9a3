"""CPU: the entropy pass's coefficient-update mode on the host (svt_hip_entropy_picture_coef, host/entropy_host.c): the four real-stream
pictures of tests/golden/coef_update_reference.npz against the all-host chain and the recorded frames; a picture without coefficients;
the second slab's size and the invariant that lets the compressed header never withhold a picture; the refresh_frame_context refusal;
read-back through svt_hip_frame_read_coef_host; the form under the sanitizers in a stand-alone program."""
import ctypes as C
import glob
import os
import subprocess
import tempfile

import numpy as np
import pytest

import coef_update_model as CM
import entropy_coef_model as EC
import entropy_model as E
import frame_model as FM
import md_inter_model as D
import svt_testlib as T

B = T.B
DEFAULT = CM.BM.tables()[0]["coef_probs"].reshape(-1)
RECORDED = (("385", 385, 353), ("376", 376, 343), ("716", 716, 608), ("490", 490, 435))        # bytes without and with updates, as the fixture records them


@pytest.mark.parametrize("k", range(4))
def test_fixture_pictures_equal_the_all_host_chain_and_the_recorded_frames(k):
    name, kind, pic, fp, entry = EC.fixture_cases()[k]
    want = CM.host_frame(kind, pic, fp, update=True)
    got = EC.host_entropy_coef(entry, fp, counts=bool(k & 1))
    g = CM.fixture()
    assert got["rc"] == 0 and got["packet"] == want["frame"] == bytes(g[f"frame_with|{name}"])
    assert (len(bytes(g[f"frame_without|{name}"])), len(got["packet"])) == RECORDED[k][1:]
    assert np.array_equal(got["probs"], want["probs"]) and got["update"].tobytes() == want["stage"]["result"].tobytes()
    assert sum(int(v) for v in got["update"]["sent"]) >= 1 and got["result"]["flags"] == 0
    plain = E.host_entropy(entry, fp)
    assert plain["packet"] == bytes(g[f"frame_without|{name}"]) and got["result"]["tokens"] == plain["result"]["tokens"]
    assert got["header_bytes"] + got["result"]["tile_bytes"] == len(got["packet"])
    # a trailer rides behind the tile
    assert EC.host_entropy_coef(entry, fp, trailer=b"\x88\x8b\x8f")["packet"] == got["packet"] + b"\x88\x8b\x8f"


def test_a_picture_without_coefficients_sends_nothing_and_equals_the_plain_form():
    p = E.zero_coefficients(D.golden_picture("mix_136x72_select_hp"))
    fp = E.inter_params(p, **EC.NO_REFRESH)
    got, plain = EC.host_entropy_coef(p, fp), E.host_entropy(p, fp)
    assert got["rc"] == 0 and got["packet"] == plain["packet"] and got["result"] == plain["result"]
    assert [int(v) for v in got["update"]["sent"]] == [0] * 4 and np.array_equal(got["probs"], DEFAULT)


def test_second_slab_size_is_the_stated_sum():
    lib = B.load()
    a16 = lambda n: (n + 15) // 16 * 16      # noqa: E731
    bools = int(lib.svt_hip_coef_update_bools_capacity())
    per = a16(4 * B.TOK_COUNTS) + a16(2304) + a16(1728) + a16(2 * bools) + a16(int(lib.svt_hip_boolcode_capacity(bools))) + a16(72) + 64
    for n in (1, 5, 32):
        lim = E.limits(136, 72, n)
        assert int(lib.svt_hip_entropy_coef_update_bytes(C.byref(lim))) == per * n
    assert int(lib.svt_hip_entropy_coef_update_bytes(C.byref(E.limits(136, 72, 0)))) == 0 and int(lib.svt_hip_entropy_coef_update_bytes(C.byref(E.limits(136, 72, 33)))) == 0
    assert int(lib.svt_hip_entropy_coef_update_bytes(None)) == 0
    # the first slab keeps its documented sum: the mode adds nothing to it
    lim = E.limits(136, 72, 3)
    assert int(lib.svt_hip_entropy_work_bytes(136, 72, 17, C.byref(lim))) % 3 == 0


def test_the_compressed_header_cannot_overflow_first_part_size():
    """at most 19 228 records whatever the picture; their coded bytes are below 2^16: no picture is withheld for its header"""
    lib = B.load()
    bools = int(lib.svt_hip_coef_update_bools_capacity())
    assert bools == B.CU_PREFIX_MAX + 4 * (1 + 396 * 12) + B.CU_SUFFIX_MAX == 19228
    assert EC.hdr_capacity() == (7 * (bools + 33) + 7) // 8 + 2 == 16856 <= 0xFFFF
    # and a stream of that many worst-case records stays inside it: every bool a 1 at probability 1 shifts the most bits
    from boolcode_model import host_code, rec
    coded = host_code(bools=np.full(bools, rec(1, 1), np.uint16), segments=[(0, bools, 1)])[0]
    assert 0 < len(coded) <= EC.hdr_capacity()


def test_a_picture_that_refreshes_the_frame_context_is_refused():
    name, kind, pic, fp, entry = EC.fixture_cases()[0]
    assert EC.host_entropy_coef(entry, dict(fp, refresh_frame_context=1, frame_parallel_decoding_mode=1))["rc"] == B.ERR_BAD_PARAMETER
    assert EC.host_entropy_coef(entry, dict(fp, refresh_frame_context=1, frame_parallel_decoding_mode=0))["rc"] == B.ERR_BAD_PARAMETER
    assert E.host_entropy(entry, dict(fp, refresh_frame_context=1))["rc"] == 0                      # the plain form takes it, as before
    ok = EC.host_entropy_coef(entry, dict(fp, error_resilient_mode=1, refresh_frame_context=1))     # not coded under error resilience: nothing is kept
    assert ok["rc"] == 0 and ok["packet"] is not None
    assert EC.host_entropy_coef(entry, fp, trailer_len=5)["rc"] == B.ERR_BAD_PARAMETER              # and what the plain form refuses


@pytest.mark.parametrize("k", range(4))
def test_packets_read_back_to_the_grids_coefficients_and_the_updated_table(k):
    name, kind, pic, fp, entry = EC.fixture_cases()[k]
    got = EC.host_entropy_coef(entry, fp)
    W, H = pic["W"], pic["H"]
    rc, info, back, table, untouched = EC.read_frame_coef(got["packet"], W, H, restrict=pic.get("restrict", 0), lrf=pic.get("lrf", (1, 3)))
    assert rc == 0 and untouched and back["guards"], B.load().svt_hip_last_error()
    assert np.array_equal(table, got["probs"]) and not np.array_equal(table, DEFAULT)
    assert info.uncompressed_bytes + info.compressed_bytes == got["header_bytes"] and back["res"]["past_end"] == 0
    assert np.array_equal(back["qcoeff"], pic["qcoeff"]) and np.array_equal(back["eob_map"], np.asarray(pic["eob_map"]).view(np.uint16))
    assert all(np.array_equal(back["lf_mi"][f], pic["lf_mi"][f]) for f in ("sb_type", "tx_size", "skip", "is_inter"))
    if kind == "inter":
        assert back["mc_mi"].tobytes() == np.ascontiguousarray(pic["mc_mi"]).tobytes()
    # the plain reader keeps refusing the update
    from test_tile_read_inter import read_frame
    assert read_frame(got["packet"], W, H, restrict=pic.get("restrict", 0), lrf=pic.get("lrf", (1, 3)))[0] == B.ERR_UNSUPPORTED


def test_host_form_under_address_and_ub_sanitizers_in_a_stand_alone_program():
    """the fixture pictures, budgets at and one below their counts, a picture without coefficients: every input in an allocation of exactly
    its bytes, the counts the caller's or the form's own in turn; size, flags, checksum and sizes sent compared with the library's.  Skipped,
    visibly, where the host compiler links no sanitizer runtime."""
    from test_entropy_host import budgets, request, sanitizer_runtime_present
    cases = []
    for name, kind, pic, fp, entry in EC.fixture_cases():
        full = EC.host_entropy_coef(entry, fp)
        W, H = entry["W"], entry["H"]
        cases += [(entry, fp, E.limits(W, H), b"\x88"), (entry, fp, E.limits(W, H, **budgets(full)), b"")]
        for field in ("max_tokens", "max_bools", "max_tile_bytes"):
            cases.append((entry, fp, E.limits(W, H, **budgets(full, **{field: -1})), b""))
    p = E.zero_coefficients(D.golden_picture("mix_136x72_select_hp"))
    cases.append((p, E.inter_params(p, **EC.NO_REFRESH), E.limits(136, 72), b""))
    want = []
    for i, (p, fp, lim, trailer) in enumerate(cases):
        got = EC.host_entropy_coef(p, fp, lim, trailer=trailer, counts=bool(i & 1))
        assert got["rc"] == 0
        want.append((got["size"], got["result"]["flags"], (sum(got["packet"] or b"") + int(got["probs"].sum())) & 0xFFFFFFFF, sum(int(v) for v in got["update"]["sent"])))
    assert {w[1] for w in want} >= {0, B.ENT_TOKENS_OVER, B.ENT_STREAM_OVER, B.ENT_TILE_OVER} and {w[3] for w in want} >= {0, 1}
    with tempfile.TemporaryDirectory() as td:
        if not sanitizer_runtime_present(td):
            pytest.skip("this compiler links no address / undefined-behaviour sanitizer runtime")
        req = os.path.join(td, "cases.bin")
        with open(req, "wb") as f:
            f.write(request(cases))
        exe = os.path.join(td, "entropy_coef_san")
        src = os.path.join(T.ROOT, "svt-vp9_amd")
        cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{os.path.join(T.ROOT, 'include')}",
               os.path.join(T.ROOT, "tests", "c", "entropy_coef_check.c")] + sorted(glob.glob(os.path.join(src, "host", "*.c"))) + ["-lpthread", "-lm", "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe, req], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = [tuple(int(v) for v in line.split()) for line in r.stdout.strip().splitlines()]
        assert got == want


def test_the_timing_tools_compile():
    """tools/entropy_time.py gained the mode's switches and tools/coef_update_bytes.py imports it: both must at least be valid Python"""
    for name in ("entropy_time.py", "coef_update_bytes.py"):
        path = os.path.join(T.ROOT, "tools", name)
        with open(path) as f:
            compile(f.read(), path, "exec")

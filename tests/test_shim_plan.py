"""The encoder library's group planner (svt-vp9_amd/shim/shim_plan.c) on a CPU: the structure of a group -- decode order, references,
temporal layers, waves, deep-stream eligibility -- is integer logic and is driven here through tests/c/shim_plan_check.c, over
levels in {3, 4}, pending in 1 .. 2^levels, cut_by_intra in {0, 1} and (first, prev_base) in {(1, 0), (17, 16), (1, -1)}.
Three judges: the plans the planner's predecessor made (tests/golden/shim_plan_parent.npz, recorded as DESIGN.md section 7 describes),
the full groups written out below, and invariants every plan must keep."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import svt_testlib as T

CASES = [(levels, pending, cut, first, prev) for levels in (3, 4) for pending in range(1, (1 << levels) + 1) for cut in (0, 1)
         for first, prev in ((1, 0), (17, 16), (1, -1))]
PIC_FIELDS = ("number", "ref0", "ref1", "layer", "levels", "n_lists", "used_as_ref", "wave")


@functools.lru_cache(maxsize=None)
def plans():
    """every case through ONE run of the stand-alone program: {case: None (refused) or dict(pics (n, 8), waves (n_waves, 2), first, last, oldest)}"""
    amd = os.path.join(T.ROOT, "svt-vp9_amd")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "shim_plan_check")
        cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-Wall", f"-I{os.path.join(T.ROOT, 'include')}", f"-I{os.path.join(amd, 'shim')}", os.path.join(T.ROOT, "tests", "c", "shim_plan_check.c"),
               os.path.join(amd, "shim", "shim_plan.c"), os.path.join(amd, "host", "gop_shard.c"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        args = [str(v) for (levels, pending, cut, first, prev) in CASES for v in (first, pending, levels, cut, prev)]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines, out, at = r.stdout.splitlines(), {}, 0
    for case in CASES:
        h = lines[at].split()
        at += 1
        if h == ["plan", "error"]:
            out[case] = None
            continue
        assert h[:2] == ["plan", "n"], h
        n, nw = int(h[2]), int(h[4])
        pics = np.array([[int(v) for v in ln.split()[1:]] for ln in lines[at:at + n]], np.int64).reshape(n, 8)
        assert all(ln.split()[0] == "pic" for ln in lines[at:at + n])
        at += n
        waves = np.array([[int(v) for v in ln.split()[2:]] for ln in lines[at:at + nw]], np.int64).reshape(nw, 2)
        assert [ln.split()[:2] for ln in lines[at:at + nw]] == [["wave", str(w)] for w in range(nw)]
        at += nw
        out[case] = dict(pics=pics, waves=waves, first=int(h[6]), last=int(h[8]), oldest=int(h[10]))
    assert at == len(lines)
    return out


def col(p, name):
    return p["pics"][:, PIC_FIELDS.index(name)]


def test_every_plan_equals_the_recorded_plans_of_the_previous_planner():
    z = np.load(os.path.join(T.ROOT, "tests", "golden", "shim_plan_parent.npz"))
    assert [tuple(int(v) for v in c) for c in z["cases"]] == CASES
    got = plans()
    for k, case in enumerate(CASES):
        n, nw, first, last, oldest = (int(v) for v in z["meta"][k])
        p = got[case]
        if n < 0:                                                  # svt_hip_minigop_split refuses pending + 1 > 2^levels pictures
            assert p is None, case
            continue
        assert p is not None, case
        assert (len(p["pics"]), len(p["waves"]), p["first"], p["last"], p["oldest"]) == (n, nw, first, last, oldest), case
        assert np.array_equal(p["pics"], z["pics"][k][:n]), case
        assert np.array_equal(p["waves"], z["waves"][k][:nw]), case


def test_full_groups_written_out():
    p = plans()[(3, 8, 0, 1, 0)]
    assert col(p, "number").tolist() == [8, 4, 2, 1, 3, 6, 5, 7]
    assert col(p, "layer").tolist() == [0, 1, 2, 3, 3, 2, 3, 3]
    refs = {int(n): (int(a), int(b)) for n, a, b in zip(col(p, "number"), col(p, "ref0"), col(p, "ref1"))}
    assert refs == {8: (0, 0), 4: (0, 8), 2: (0, 4), 1: (0, 2), 3: (2, 4), 6: (4, 8), 5: (4, 6), 7: (6, 8)}
    assert np.array_equal(col(p, "wave"), col(p, "layer"))
    assert np.array_equal(col(p, "used_as_ref"), (col(p, "layer") < 3).astype(np.int64))
    assert p["waves"][:, 0].tolist() == [0, 1, 2, 3] and p["waves"][:, 1].tolist() == [0, 0, 1, 1]
    p = plans()[(4, 16, 0, 1, 0)]
    assert p["waves"][:, 0].tolist() == [0, 1, 2, 3, 4] and p["waves"][:, 1].tolist() == [0, 0, 0, 1, 1]
    assert int(np.isin(col(p, "wave"), np.flatnonzero(p["waves"][:, 1])).sum()) == 12 and len(p["pics"]) == 16


@pytest.mark.parametrize("levels", [3, 4])
def test_invariants_of_every_plan(levels):
    for case in [c for c in CASES if c[0] == levels]:
        _, pending, cut, first, prev = case
        p = plans()[case]
        parts = T.product_minigop_split(pending + cut, levels, cut) if pending + cut <= (1 << levels) else None
        assert (p is None) == (parts is None), case
        if p is None:
            continue
        number, wave, layer = col(p, "number"), col(p, "wave"), col(p, "layer")
        assert sorted(number.tolist()) == list(range(first, first + pending)), case               # each picture exactly once
        wave_of = dict(zip(number.tolist(), wave.tolist()))
        chain_heads = set()                                                                       # the first picture of a P chain predicts from its display
        for i in range(len(number)):                                                              # predecessor: prev_base in every state the library reaches (the
            if col(p, "n_lists")[i] == 1 and number[i] == first:                                  # recorded (1, -1) cases keep the predecessor's q - 1 rule)
                chain_heads.add(int(number[i]))
        for i in range(len(number)):
            refs = [int(col(p, "ref0")[i])] + ([int(col(p, "ref1")[i])] if col(p, "n_lists")[i] == 2 else [])
            assert (col(p, "ref1")[i] == -1) == (col(p, "n_lists")[i] == 1), case
            for r in refs:
                assert r == prev or (r in wave_of and wave_of[r] < wave[i]) or (int(number[i]) in chain_heads and r == first - 1), (case, int(number[i]), r)
        for w in range(len(p["waves"])):                                                          # one layer per wave, and it is the wave's
            assert set(layer[wave == w].tolist()) == {int(p["waves"][w, 0])}, (case, w)
        assert len(p["waves"]) <= len(number), case
        nonneg = [int(r) for r in np.concatenate([col(p, "ref0"), col(p, "ref1")]) if r >= 0]
        assert p["oldest"] == min([first] + nonneg) and p["first"] == first and p["last"] == first + pending - 1, case
        # cut_by_intra changes only what svt_hip_minigop_split changes: the plan follows from the split's parts alone
        want, prev_k, nw = [], prev, 0
        for idx, (start, length, lv, ra) in enumerate(parts):
            length -= 1 if cut and idx == len(parts) - 1 else 0
            if length < 1:
                continue
            p0, base = first + start, first + start + length - 1
            if ra and prev_k >= 0:
                want.append((base, prev_k, prev_k, 0, lv, 2, 1, nw))

                def hierarchy(lo, hi, lay):
                    if hi - lo < 2:
                        return
                    mid = (lo + hi) // 2
                    want.append((mid, lo, hi, lay, lv, 2, int(lay < lv), nw + lay))
                    hierarchy(lo, mid, lay + 1)
                    hierarchy(mid, hi, lay + 1)
                hierarchy(prev_k, base, 1)
                nw += lv + 1
            else:
                for q in range(p0, base + 1):
                    want.append((q, q - 1, -1, 0, lv, 1, 1, nw))
                    nw += 1
            prev_k = base
        assert p["pics"].tolist() == [list(w) for w in want] and len(p["waves"]) == nw, case

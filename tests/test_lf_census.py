"""The deblocking oracle's census (oracle/oracle.h) over the extremes list: the list must keep reaching every branch it was chosen for,
and counting must not change a sample."""
import numpy as np
import pytest

import svt_testlib as T

# a condition on the list, not a measurement: every class at least this often (svt_testlib.LF_EXTREMES_CASES)
MIN_COUNT = 10


@pytest.fixture(scope="module")
def census():
    """[(case tuple, planes with the census on, counts)] over the list"""
    return [(c,) + T.oracle_lf_frame_census(T.make_lf_extremes_case(*c)) for c in T.LF_EXTREMES_CASES]


def test_lf_extremes_list_shape():
    cases = T.LF_EXTREMES_CASES
    assert len(cases) <= 8 and len(set(cases)) == len(cases)
    assert all(w <= 264 and h <= 200 and w % 8 == 0 and h % 8 == 0 for _, w, h, _, _ in cases)
    sharp = {c[3] for c in cases}
    assert 0 in sharp and 7 in sharp and sharp & {1, 2, 3, 4, 5, 6}
    assert {(104, 40), (40, 104)} <= {(c[1], c[2]) for c in cases}
    assert {c[4] for c in cases} == {0, 1}


def test_lf_extremes_census_reaches_every_class(census):
    """per sample position: every class >= MIN_COUNT on the vertical-walk pictures and on the horizontal-walk pictures separately;
    per edge and per SB: >= MIN_COUNT over the list"""
    by_axis = {a: {k: sum(cnt[k] for c, _, cnt in census if c[4] == a) for k in T.LF_CENSUS} for a in (0, 1)}
    print({k: (by_axis[0][k], by_axis[1][k]) for k in T.LF_CENSUS})
    short = []
    for k in T.LF_CENSUS:
        if k in T.LF_CENSUS_PER_POSITION:
            short += [(k, a, by_axis[a][k]) for a in (0, 1) if by_axis[a][k] < MIN_COUNT]
        elif by_axis[0][k] + by_axis[1][k] < MIN_COUNT:
            short.append((k, "both", by_axis[0][k] + by_axis[1][k]))
    assert not short, short


def test_lf_ragged_branches_within_one_sb_row_and_column(census):
    """the thin and ragged pictures of tests/test_gpu_lf.py take adjust_mask's rows / cols == 5 and == 1 branches inside a single SB
    row (104x40, 72x8) and a single SB column (40x104, 8x72)"""
    got = {(c[1], c[2]): cnt for c, _, cnt in census}
    for size, keys in (((104, 40), ("ROWS_5", "COLS_5")), ((40, 104), ("ROWS_5", "COLS_5")), ((72, 8), ("ROWS_1", "COLS_1")), ((8, 72), ("ROWS_1", "COLS_1"))):
        assert all(got[size][k] >= 1 for k in keys), (size, {k: got[size][k] for k in keys})


def test_lf_census_leaves_the_samples_alone(census):
    for c, planes, cnt in census:
        case = T.make_lf_extremes_case(*c)
        assert all(np.array_equal(a, b) for a, b in zip(planes, T.oracle_lf_frame(case))), c
        assert sum(cnt.values()) > 0
    # and off means off: nothing is counted after the census call has returned
    _, again = T.oracle_lf_frame_census(T.make_lf_extremes_case(*T.LF_EXTREMES_CASES[0]))
    assert again == census[0][2]

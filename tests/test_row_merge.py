"""What the two device merges share (csrc/row_merge.h: the class of a row, the stable partition by class, the cut),
through both of them with nms == 0, where nothing else runs: cp_merge_detections against oracle merge_outputs and
cp_merge_detections_mask against its host statement, bit for bit, and the two against each other -- the same counts and
the same rows, in another order inside a class (the mask merge sorts a class by score).  The row counts are no
multiple of 4 and lie on both sides of a wave: the cut takes four slots per thread in one merge and one in the other.
Scores have eight levels, so ties sit at the cut."""
import functools

import numpy as np
import pytest

import test_mask_nms as mask
import test_merge_device as literal
from test_mask_nms import host

C, NCOLS, CANVAS = 8, 13, 64
SHAPES = [(1, 1), (1, 5), (3, 21), (5, 13), (7, 37), (1, 1023)]
KEPT_AT_THE_CUT = {(1, 5): (1, 2), (3, 21): (21, 24), (5, 13): (21, 29), (7, 37): (86, 91), (1, 1023): (341, 461)}
CASES = [(S, K, S * K) for S, K in SHAPES] + [(S, K, KEPT_AT_THE_CUT[S, K][0]) for S, K in SHAPES[1:]]
cases = pytest.mark.parametrize("case", CASES, ids=["%dx%d-%d" % c for c in CASES])


@functools.lru_cache(maxsize=None)
def rows_for(S, K):
    R = S * K
    rng = np.random.RandomState(1000 * S + K)
    rows = np.zeros((R, NCOLS), np.float32)
    rows[:, 0:2] = rng.uniform(0, 40, (R, 2))
    rows[:, 2:4] = rows[:, 0:2] + rng.uniform(1, 20, (R, 2))
    rows[:, 4] = np.round(rng.uniform(0.05, 1, R) * 8) / 8
    rows[:, 5] = rng.randint(0, C, R)
    if R >= 8:
        rows[:3, 5] = [-1, 8, 2.5]                                       # no class: dropped
    rows[:, 6:12] = rng.uniform(0, 60, (R, 6))
    rows[:, 12] = np.arange(R)                                            # the rows are distinct
    rows = rows.reshape(S, K, NCOLS)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def references(case):
    """(literal table, counts), (mask table, counts) of the two host statements; made once, never modified."""
    S, K, mpi = case
    rows, R = rows_for(S, K), S * K
    lit = literal._merge_reference(rows, C, mpi, 0)
    msk = host.mask_nms(rows, C, np.zeros(R, np.int32), np.zeros((R, R), np.int32), mpi, threshold=-np.inf)
    for a in lit + msk:
        a.setflags(write=False)
    return lit, msk


def _multiset(table):
    return sorted(r.tobytes() for r in np.ascontiguousarray(table).view(np.uint32))


def assert_same_rows(lit, msk):
    """Equal counts and equal multisets of rows, class by class."""
    (lt, lc), (mt, mc) = lit, msk
    assert lc.tolist() == mc.tolist()
    at = 0
    for n in lc[1:]:
        assert _multiset(lt[at:at + n]) == _multiset(mt[at:at + n])
        at += n
    assert at == lc[0] == len(lt) == len(mt)


def test_shapes_are_what_the_cut_can_get_wrong():
    assert [S * K for S, K in SHAPES] == [1, 5, 63, 65, 259, 1023]
    assert all(S * K % 4 for S, K in SHAPES) and max(S * K for S, K in SHAPES) <= 1024
    assert all(KEPT_AT_THE_CUT[S, K][0] == max(1, S * K // 3) for S, K in SHAPES[1:])


@cases
def test_host_statements_agree_and_the_cut_cases_cut_with_ties(case):
    S, K, mpi = case
    lit, msk = references(case)
    assert_same_rows(lit, msk)
    dropped = 3 if S * K >= 8 else 0
    if mpi == S * K:
        assert lit[1][0] == S * K - dropped
    else:
        assert lit[1][0] > mpi and (mpi, lit[1][0]) == KEPT_AT_THE_CUT[S, K]


@pytest.mark.gpu
@cases
def test_literal_merge_without_nms_matches_the_oracle_bitwise(case):
    S, K, mpi = case
    want, want_counts = references(case)[0]
    got, counts = literal._merge_device(np.array(rows_for(S, K)), C, mpi, 0)
    assert counts.tolist() == want_counts.tolist()
    assert literal._same_bits(got, want)


def _mask_device(case):
    S, K, mpi = case
    return mask._merge_device(rows_for(S, K), C, CANVAS, CANVAS, (mpi, 0.5, 0.5, 0.001, 2), nms=0)


@pytest.mark.gpu
@cases
def test_mask_merge_without_nms_matches_the_host_statement_bitwise(case):
    want, want_counts = references(case)[1]
    got, counts = _mask_device(case)                                      # (nothing written beyond counts[0] rows)
    assert counts.tolist() == want_counts.tolist()
    assert mask._same_bits(got, want), mask._report(got, want)
    again, counts2 = _mask_device(case)
    assert mask._same_bits(again, got) and counts2.tolist() == counts.tolist()


@pytest.mark.gpu
@cases
def test_the_two_device_merges_keep_the_same_rows(case):
    S, K, mpi = case
    assert_same_rows(literal._merge_device(np.array(rows_for(S, K)), C, mpi, 0), _mask_device(case))

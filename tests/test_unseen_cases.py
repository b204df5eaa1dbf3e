"""The preconditions of the als_recommend_unseen cases (tests/unseen_cases.py), checked with the oracle alone:
the GPU tests (tests/test_gpu_recommend_unseen.py) rely on them to know which tier served which row."""
import numpy as np
import pytest

from tests import query_cases as QC
from tests import unseen_cases as UC


def _well_formed(case):
    n_dst = len(case["dst_ids"])
    assert np.all(np.diff(case["src_ids"].astype(np.int64)) > 0) and np.all(np.diff(case["dst_ids"].astype(np.int64)) > 0)
    assert all(len(e) > 0 and np.all(np.diff(e) > 0) and e[0] >= 0 and e[-1] < n_dst for e in case["E"])
    assert np.array_equal(np.unique(np.concatenate(case["E"])), np.arange(n_dst))  # the ratings name every dst id
    assert np.isfinite(case["U"]).all() and np.isfinite(case["V"]).all()


@pytest.mark.parametrize("rank", UC.RANKS)
def test_ladder_rows_fall_where_designed(rank):
    case = UC.ladder(rank)
    _well_formed(case)
    n_src, n_dst = len(case["src_ids"]), len(case["dst_ids"])
    assert n_dst == 700 and set(UC.ladder_m(n_dst)) <= set(case["m"].tolist())
    s = UC.survivors(case, UC.DEPTH)
    assert np.array_equal(s, UC.DEPTH - np.minimum(case["m"], UC.DEPTH))  # the extras lie outside every list
    t2 = UC.tier2_rows(case, UC.DEPTH, UC.K)
    assert np.array_equal(t2, UC.designed_tier2(case)) and 0 < len(t2) < n_src
    assert (s == UC.K).any() and (s == UC.K - 1).any()
    left = n_dst - np.array([len(e) for e in case["E"]])
    assert (left == 0).sum() == 1 and ((left > 0) & (left < UC.K)).any()  # all padding, and short lists
    for depth in (UC.K, 48):
        assert np.array_equal(UC.tier2_rows(case, depth, UC.K), UC.designed_tier2(case, depth, UC.K))


def test_expected_fast_equals_expected_on_a_sample():
    case = UC.passes()
    _well_formed(case)
    rows = np.concatenate([np.arange(0, len(case["src_ids"]), 97)[:40], [1, 2, 65535, 65536, len(case["src_ids"]) - 1]])
    fast = UC.expected_fast(case, UC.K)
    assert QC.same((fast[0][rows], fast[1][rows]), UC.expected(case, UC.K, rows))
    t2 = UC.tier2_rows(case, UC.DEPTH, UC.K)
    assert 0 < len(t2) < len(case["src_ids"]) and (t2 < 65536).any() and (t2 >= 65536).any()  # in both passes
    small = UC.ladder(3)
    assert QC.same(UC.expected_fast(small, UC.K), UC.expected(small, UC.K))


def test_sizes_cases():
    for k in (1, 30, 64):
        for n in UC.SIZES:
            n_dst = UC.size(n, k)
            if n_dst < 1:
                continue
            case = UC.sizes(n_dst, k)
            _well_formed(case)
            left = n_dst - np.array([len(e) for e in case["E"]])
            assert left[-1] == 0
            if n_dst > k + 1:
                assert left[:3].tolist() == [k - 1, k, k + 1]
            if n_dst <= UC.DEPTH:
                assert len(UC.tier2_rows(case, UC.DEPTH, k)) == 0
    assert len(UC.tier2_rows(UC.sizes(513, 30), UC.DEPTH, 30)) > 0


def test_tie_cases_put_ties_on_the_boundaries():
    case = UC.tie_groups()
    _well_formed(case)
    s = UC.scores(case)
    order = UC.ranking(case)
    tie_score = s[0, case["tie"][0]]
    assert (s[0, case["tie"]] == tie_score).all()
    assert s[0, order[0][UC.DEPTH - 1]] == tie_score == s[0, order[0][UC.DEPTH]]  # across place depth, unfiltered
    across_k = 0
    for i in range(len(case["src_ids"]) - 1):
        kept = order[i][~np.isin(order[i], case["E"][i])]
        across_k += int(s[i, kept[UC.K - 1]] == tie_score == s[i, kept[UC.K]])
        assert np.isin(case["tie"], case["E"][i]).any() or i == 0
    assert across_k >= 8
    assert len(UC.tier2_rows(case, UC.DEPTH, 64)) > 1
    mt = UC.mass_tie()
    _well_formed(mt)
    n_known = sorted(len(e) for e in mt["E"])
    assert n_known[-3:] == [250, 300, len(mt["dst_ids"])] and len(UC.tier2_rows(mt, UC.DEPTH, UC.K)) >= 3
    zn = UC.zeros_and_negatives()
    _well_formed(zn)
    sz = UC.scores(zn)
    assert (sz[:4] == 0).all() and (sz[4:] <= 0).all() and ((sz[4:] == 0).sum(axis=1) == len(zn["zero"])).all()


def test_pruning_case_sends_every_row_to_the_exact_scan():
    case = UC.pruning()
    _well_formed(case)
    assert len(UC.tier2_rows(case, UC.DEPTH, UC.K)) == len(case["src_ids"])
    assert all(len(e) == UC.PRUNE_KNOWN for e in case["E"][:-1])

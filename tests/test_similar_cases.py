"""The preconditions of tests/similar_cases.py, on the CPU: what the GPU tests of als_similar take for granted
about their own cases holds by the numpy definition, before any device is asked."""
import numpy as np
import pytest

from oracle import spark_als as O
from tests import similar_cases as SC


def _case(name):
    return getattr(SC, name)()


def test_unit_image_follows_the_definition_step_by_step():
    case = SC.random_case(257, 30, 5)
    F = case["F"]
    U, ok = SC.unit_image(F)
    assert ok.all()
    for r in (0, 100, 256):
        s = np.float32(0.0)
        for c in range(F.shape[1]):
            s = np.float32(s + np.float32(F[r, c] * F[r, c]))
        root = np.sqrt(s, dtype=np.float32)
        assert np.array_equal(SC.bits(U[r]), SC.bits(np.array([np.float32(v / root) for v in F[r]], np.float32)))


def test_power_of_two_scaling_keeps_the_unit_row_and_copies_tie():
    case = SC.tie_case()
    U, ok = SC.unit_image(case["F"])
    blk = case["block"]
    assert ok.all() and blk.size > case["k"] and blk[0] < SC.SLICE_ROWS <= blk[-1]
    assert all(np.array_equal(SC.bits(U[b]), SC.bits(U[blk[0]])) for b in blk)      # bit-equal unit rows
    norms = np.linalg.norm(case["F"][blk].astype(np.float64), axis=1)
    assert norms.max() / norms.min() == 2.0 ** 18                                    # scaled by 2^-9 .. 2^9
    src, ids, sc = SC.expected(case)
    bid = case["ids"][blk]
    k = case["k"]
    assert ids[0].tolist() == bid[:k].tolist()                                       # an outside row: the lowest ids
    assert ids[1].tolist() == bid[1:k + 1].tolist()                                  # the first member leaves itself out
    mid = [b for b in bid if b != src[2]][:k]
    assert ids[2].tolist() == mid and src[2] not in ids[2]
    for row in sc:
        assert np.unique(SC.bits(row)).size == 1                                      # the whole list ties
    # a row against a copy of itself scores f2j_sdot(u, u), whatever that is: it need not be 1.0f
    assert np.array_equal(SC.bits(sc[1][:1]), SC.bits(O.f2j_sdot(U[blk[:1]], U[blk[:1]])))


def test_edge_rows_find_their_copies_in_another_slice():
    case = SC.edge_copy_case()
    src, ids, sc = SC.expected(case)
    for j, (q, c) in enumerate(case["pairs"].items()):
        assert q // SC.SLICE_ROWS != c // SC.SLICE_ROWS and q % SC.SLICE_ROWS in (0, SC.SLICE_ROWS - 1, 999 % SC.SLICE_ROWS)
        assert src[j] == case["ids"][q] and ids[j][0] == case["ids"][c] and src[j] not in ids[j]
        assert sc[j][0] > 0.9999 and (sc[j][1:] < 0.99).all()  # the copy leads by far more than rounding


@pytest.mark.parametrize("rank", (1, 5, 64))
def test_rows_without_a_direction_are_flagged_by_the_numpy_rule(rank):
    rows = SC.no_direction_rows(rank)
    U, ok = SC.unit_image(rows)
    assert rows.shape[0] == 7 and not ok.any() and np.isnan(U).all()
    with np.errstate(all="ignore"):
        s = O.f2j_sdot(rows, rows)
    assert s[0] == 0 and s[1] == 0 and np.isnan(s[2]) and np.isinf(s[3]) and np.isinf(s[4]) and np.isinf(s[5]) and s[6] == 0
    assert np.isfinite(rows[5]).all() and (rows[6] > 0).all()  # overflow and underflow of s, not of the row


def test_cases_without_direction():
    case = SC.no_direction_case()
    U, ok = SC.unit_image(case["F"])
    assert np.array_equal(np.flatnonzero(~ok), case["at"])
    src, ids, sc = SC.expected(case)
    bad = case["ids"][case["at"]]
    assert not np.isin(ids, bad).any()
    assert (ids[case["at"]] == -1).all() and np.isnan(sc[case["at"]]).all()
    assert (ids[ok] != -1).all()
    case = SC.all_without_direction_case()
    assert not SC.unit_image(case["F"])[1].any()
    _, ids, sc = SC.expected(case)
    assert (ids == -1).all() and np.isnan(sc).all()
    case = SC.k_plus_one_directions_case()
    U, ok = SC.unit_image(case["F"])
    assert ok.sum() == case["k"] + 1 and np.array_equal(np.flatnonzero(ok), case["good"])
    _, ids, sc = SC.expected(case)
    assert (ids[ok] != -1).all() and (ids[~ok] == -1).all()


def test_subset_case_holds_what_it_says():
    case = SC.subset_case()
    sub, ids = case["subset"], case["ids"]
    assert SC.I32_MIN in ids and SC.I32_MAX in ids and SC.I32_MIN in sub and SC.I32_MAX in sub
    assert np.isin(case["unknown"], sub).all() and not np.isin(case["unknown"], ids).any()
    assert np.sum(sub == ids[3]) == 3 and not np.array_equal(sub, np.sort(sub))
    src, out, sc = SC.expected(case)
    assert np.array_equal(src, sub)
    unk = np.isin(sub, case["unknown"])
    assert (out[unk] == -1).all() and (out[~unk] != -1).all()
    three = np.flatnonzero(sub == ids[3])
    assert all(SC.same((out[j], sc[j]), (out[three[0]], sc[three[0]])) for j in three)


@pytest.mark.parametrize("rank", SC.RANKS)
def test_definition_is_within_its_bound_of_the_fp64_cosine(rank):
    case = SC.random_case(300, 30, rank)
    F = case["F"]
    U, ok = SC.unit_image(F)
    assert ok.all()
    cos32 = O.f2j_sdot(U[:, None, :], U[None, :, :]).astype(np.float64)
    err = np.max(np.abs(cos32 - SC.fp64_cosine(F)))
    bound = (rank + 4) * 2.0 ** -24
    print(f"rank {rank}: worst |cos - fp64 cosine| = {err:.3e}, {err / bound:.2f} of the bound")
    assert err <= bound
    norms = np.linalg.norm(F.astype(np.float64), axis=1)
    assert norms.max() / norms.min() > 1e10  # many decades


def _unambiguous(case):
    """Every expected list is strictly ordered by (score desc, id asc), holds no id twice, never the row itself,
    and is as long as the rows left allow."""
    src, ids, sc = SC.expected(case)
    _, ok = SC.unit_image(case["F"])
    all_ids = np.asarray(case["ids"], np.int32)
    for j in range(src.size):
        n = int(np.sum(~np.isnan(sc[j])))
        r = np.searchsorted(all_ids, src[j])
        known = r < all_ids.size and all_ids[r] == src[j] and ok[r]
        assert n == (min(case["k"], int(ok.sum()) - 1) if known else 0)
        assert (ids[j][n:] == -1).all() and np.isnan(sc[j][n:]).all()
        li, ls = ids[j][:n], sc[j][:n]
        assert np.unique(li).size == n and src[j] not in li[:n]
        for a in range(n - 1):
            assert ls[a] > ls[a + 1] or (ls[a] == ls[a + 1] and li[a] < li[a + 1])


@pytest.mark.parametrize("name", SC.CASES)
def test_named_cases_are_unambiguous(name):
    _unambiguous(_case(name))


@pytest.mark.parametrize("n", SC.SIZES)
def test_size_cases_are_unambiguous(n):
    for k in SC.KS:
        _unambiguous(SC.random_case(SC.size(n, k), k, 6))


def test_one_row_is_all_padding_and_k_plus_one_rows_fill_the_list():
    _, ids, sc = SC.expected(SC.random_case(1, 30, 6))
    assert (ids == -1).all() and np.isnan(sc).all()
    _, ids, _ = SC.expected(SC.random_case(31, 30, 6))
    assert (ids != -1).all()
    _, ids, _ = SC.expected(SC.random_case(30, 30, 6))
    assert (ids[:, :29] != -1).all() and (ids[:, 29] == -1).all()

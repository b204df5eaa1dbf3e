"""CPU checks of the fold-in test data (tests/foldin_cases.py): the generators hold what the GPU tests
rely on, and `expected` is the half-sweep of the same rows."""
import numpy as np
import pytest

from oracle import spark_als as O
from tests import foldin_cases as FC
from tests import ladder as LD


def test_every_ladder_degree_is_an_item_row():
    row, src, r = FC.ladder_items("varying")
    B = FC.data("varying")[3]
    ids, ptr, col, val, deg = FC.fold_csr(row, src, r, B.user_ids)
    assert ids.size == 2 * len(LD.LADDER) == 52
    assert sorted(deg.tolist()) == sorted(LD.LADDER + LD.LADDER)
    assert not np.isin(ids, B.item_ids).any()  # shifted off the model's ids
    assert max(LD.LADDER) > 2 * FC.FOLD_TILE + 1 and min(LD.LADDER) == 1


@pytest.mark.parametrize("mode", FC.MODES)
def test_expected_equals_the_half_sweep_of_the_full_data(mode):
    """Folding the ladder's own item rows in is the item half of a sweep over the whole data set."""
    implicit, alpha, reg = LD.MODES[mode]
    user, item, r, B = FC.data(mode)
    k = 50
    Y = FC.src_factors(k, len(B.user_ids), seed=1)
    ids, deg, X = FC.expected(Y, B.user_ids, item, user, r, reg=reg, alpha=alpha, implicit=implicit)
    V = O.half_sweep(Y, B.i_ptr, B.i_col, B.i_val, reg=reg, alpha=alpha, implicit=implicit)
    assert np.array_equal(ids, B.item_ids) and np.array_equal(deg, np.diff(B.i_ptr))
    assert np.array_equal(X, V)
    if mode == "mixed":  # the rows without a positive rating
        assert (~X.any(axis=1)).sum() >= 4


def test_mirror_direction_has_one_row_per_user():
    for mode in FC.MODES:
        ids, deg, X = FC.ladder_expected(mode, 50, 0)
        B = FC.data(mode)[3]
        assert np.array_equal(ids.astype(np.int64) - FC.ID_SHIFT, B.user_ids) and np.array_equal(deg, np.diff(B.u_ptr))
        assert np.isfinite(X).all()


def test_tile_edge_rows_have_their_degrees():
    B = FC.data("varying")[3]
    want = FC.tile_degrees(128)
    row, src, r = FC.degree_rows(want, B.user_ids)
    ids, ptr, col, val, deg = FC.fold_csr(row, src, r, B.user_ids)
    assert deg.tolist() == want == [31, 32, 33, 65, 127, 128, 129]
    assert all(np.all(np.diff(col[ptr[j]:ptr[j + 1]]) > 0) for j in range(ids.size))  # ascending, no copies


def test_contract_case_holds_its_edges():
    B = FC.data("varying")[3]
    row, src, r = FC.contract_case(B.user_ids)
    ids, ptr, col, val, deg = FC.fold_csr(row, src, r, B.user_ids)
    assert ids[0] == FC.I32_MIN and ids[-1] == FC.I32_MAX and -1 in ids
    by_id = dict(zip(ids.tolist(), deg.tolist()))
    assert by_id[77] == 0 and int(np.sum(row == 77)) == 3            # a row of unknown sources only
    assert by_id[78] == 6 and int(np.sum(row == 78)) == 11           # unknown sources mixed in
    for rid, copies in ((100, 2), (101, 3), (102, 64)):
        j = int(np.searchsorted(ids, rid))
        c = col[ptr[j]:ptr[j + 1]]
        assert by_id[rid] == copies + 4 and int(np.sum(c == 7)) == copies  # src_ids[7] is row 7
    assert np.all(np.diff(ids) > 0)
    r2, s2, v2 = FC.without_duplicates(row, src, r)
    key = (r2.astype(np.int64) << 32) | (s2.astype(np.int64) & 0xFFFFFFFF)
    assert np.unique(key).size == key.size and np.array_equal(np.unique(r2), ids)
    ids_e, deg_e, X = FC.expected(FC.src_factors(128, len(B.user_ids)), B.user_ids, row, src, r, reg=0.5, alpha=10.0,
                                  implicit=True)
    assert np.array_equal(deg_e, deg) and not X[ids_e == 77].any() and np.isfinite(X).all()


def test_unknown_sources_are_unknown():
    B = FC.data("varying")[3]
    assert not np.isin(FC.unknown_sources(B.user_ids, 8), B.user_ids).any()


@pytest.mark.parametrize("implicit", [True, False])
def test_only_the_singular_case_is_not_positive_definite(implicit):
    src_ids, Y, row, src, r = FC.singular_case()
    with pytest.raises(O.NotPositiveDefinite):
        FC.expected(Y, src_ids, row, src, r, reg=0.0, alpha=1.0, implicit=implicit)
    ids, deg, X = FC.expected(Y, src_ids, row, src, r, reg=0.5, alpha=1.0, implicit=implicit)
    assert deg.tolist() == [1] and np.isfinite(X).all()

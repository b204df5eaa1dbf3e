"""CPU checks of the als_explain test data (tests/explain_cases.py): the preconditions the GPU tests
(tests/test_gpu_explain.py) rely on, and the Python layer's refusals, which need no GPU.

Measured here over the ladder cases (new items at ranks 1 .. 256 and new users at ranks 50 and 128, three
modes, the targets of explain_cases.ladder_case): the two fp64 routes of the reference differ by at most
5.6e-12·scale (stars_signed at rank 256; 1.2e-12 on the other modes there, 1.9e-13 or less below rank 256); the smallest gap among the first 11
contributions of a pair on `varying` at ranks >= 50 is 8.5e-8·scale; the score identity against the oracle's
fp32 fold-in row uses at most 0.86 of its bound (rank 1; 0.38 from rank 50 on).  Each test prints its figure."""
import numpy as np
import pytest

from tests import explain_cases as XC
from tests import foldin_cases as FC

LADDER = [(mode, k, 1) for k in XC.RANKS for mode in XC.MODES] + [(mode, k, 0) for k in (50, 128) for mode in XC.MODES]


def _id(c):
    return f"{c[0]}-k{c[1]}-{'items' if c[2] == 1 else 'users'}"


def _scales(ref):
    return [float(np.max(np.abs(f[1]))) if f is not None and f[1].size else 0.0 for f in ref.full]


@pytest.mark.parametrize("case", LADDER, ids=_id)
def test_two_routes_of_the_reference_agree(case):
    a, b = XC.ladder_expected(*case), XC.ladder_expected(*case, route="solve")
    worst = 0.0
    for fa, fb, s in zip(a.full, b.full, _scales(a)):
        assert np.array_equal(fa[0], fb[0])
        if fa[1].size:
            d = float(np.max(np.abs(fa[1] - fb[1])))
            assert d <= 1e-11 * s
            worst = max(worst, d / s if s > 0 else 0.0)
    print(f"EXPLAIN routes {_id(case)}: worst {worst:.3e}")


@pytest.mark.parametrize("case", [c for c in LADDER if c[0] == "varying" and c[1] >= 50], ids=_id)
def test_varying_lists_have_no_near_ties(case):
    """The GPU test compares the ids of these lists exactly: the first 11 contributions of every pair are
    further apart than any admissible error."""
    ref = XC.ladder_expected(*case)
    gap = np.inf
    for (src, e), s in zip(ref.full, _scales(ref)):
        top = np.sort(e)[::-1][:11]
        if top.size > 1:
            g = float(np.min(-np.diff(top))) / s
            assert g > 1e-8
            gap = min(gap, g)
    print(f"EXPLAIN gaps {_id(case)}: smallest {gap:.3e}")


@pytest.mark.parametrize("case", [("mixed", 50, 1), ("stars_signed", 50, 1), ("varying", 1, 1)], ids=_id)
def test_exact_ties_are_present(case):
    """Zero contributions of w = 0 ratings (mixed: ratings <= 0; stars_signed: ratings of 0) and, at rank 1,
    equal src rows: rules 1-3 of check_pair meet exact ties."""
    ref = XC.ladder_expected(*case)
    tied = zeros = 0
    for src, e in ref.full:
        v = np.sort(e)
        tied += int(np.sum(v[1:] == v[:-1]))
        zeros += int(np.sum(e == 0.0))
    assert tied > 0
    if case[1] > 1:
        assert zeros > 0
    # the reference's own lists pass the rule, ties and all
    XC.check_all((ref.total, ref.ids, ref.val), ref, 10, what=_id(case))


@pytest.mark.parametrize("case", LADDER, ids=_id)
def test_total_is_the_score_of_the_oracles_fold_in_row(case):
    mode, k, side = case
    src_ids, Y, t, (pr, pt), kw = XC.ladder_case(mode, k, side)
    ref = XC.ladder_expected(*case)
    ids, deg, X = FC.ladder_expected(mode, k, side)
    x = X[np.searchsorted(ids, pr)].astype(np.float64)
    yt = np.asarray(Y, np.float64)[np.searchsorted(src_ids, pt)]
    prod = x * yt
    score, mag = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    worst = 0.0
    for p in range(pr.size):
        bound = 2.0 ** -24 * mag[p] + 1e-10 * float(np.sum(np.abs(ref.full[p][1])))
        d = abs(ref.total[p] - score[p])
        assert d <= bound
        worst = max(worst, d / bound if bound > 0 else 0.0)
    print(f"EXPLAIN identity {_id(case)}: worst ratio to the bound {worst:.3f}")


def test_the_cases_hold_their_edges():
    B = FC.data("varying")[3]
    src_ids = B.user_ids
    # the ladder: a target among the row's own sources, a negative contribution among the first m, m above the degree
    _, Y, t, (pr, pt), kw = XC.ladder_case("varying", 50, 1)
    ref = XC.ladder_expected("varying", 50, 1)
    own = sum(int(pt[p] in ref.full[p][0]) for p in range(pr.size))
    assert own >= 52 and own < pr.size
    assert any(np.any(ref.val[p] < 0) for p in range(pr.size))
    assert any(np.isnan(ref.val[p]).any() and ref.full[p][1].size > 0 for p in range(pr.size))
    # the contract case: a degree-0 row, an unknown target, an unknown row, copies, a pair given twice
    row, src, r = FC.contract_case(src_ids)
    cr, ct = XC.contract_pairs(src_ids)
    Y = FC.src_factors(128, len(src_ids), seed=1)
    ref = XC.expected(Y, src_ids, row, src, r, cr, ct, 10, reg=0.5, alpha=10.0, implicit=True)
    p77 = np.nonzero(cr == 77)[0]
    assert p77.size >= 3 and np.all(ref.total[p77] == 0.0) and not np.signbit(ref.total[p77]).any()
    assert all(ref.full[p][1].size == 0 and np.isnan(ref.val[p]).all() for p in p77)
    unknown = [p for p in range(cr.size) if ref.full[p] is None]
    assert len(unknown) == 3 and np.isnan(ref.total[unknown]).all()
    assert sorted(int(cr[p]) for p in unknown) == [-1, XC.UNKNOWN_ROW, XC.UNKNOWN_ROW]
    assert {int(FC.I32_MIN), -1, int(FC.I32_MAX)} <= set(cr.tolist())
    p102 = [p for p in range(cr.size) if cr[p] == 102 and ct[p] == src_ids[7]]
    assert p102 and int(np.sum(ref.full[p102[0]][0] == src_ids[7])) == 64
    assert int(np.sum(ref.ids[p102[0]] == src_ids[7])) == 10  # the 64 copies fill the list: a target of its own
    assert cr[-1] == cr[0] and ct[-1] == ct[0] and np.array_equal(ref.val[-1], ref.val[0], equal_nan=True)
    XC.check_all((ref.total, ref.ids, ref.val), ref, 10, what="contract")


def test_tie_case_is_bit_equal_in_the_reference():
    B = FC.data("varying")[3]
    src_ids = B.user_ids
    Y = XC.tie_factors(FC.src_factors(128, len(src_ids), seed=1))
    t, (pr, pt) = XC.tie_case(src_ids)
    ref = XC.expected(Y, src_ids, *t, pr, pt, 20, reg=0.5, alpha=10.0, implicit=True)
    a, b = src_ids[3], src_ids[11]
    for p in range(pr.size):
        src, e = ref.full[p]
        ea, eb = e[src == a], e[src == b]
        assert ea.size == 1 and eb.size == 1 and ea[0] == eb[0] and ea[0] != 0.0
        ia, ib = int(np.nonzero(ref.ids[p] == a)[0][0]), int(np.nonzero(ref.ids[p] == b)[0][0])
        assert ib == ia + 1  # equal values: the lower id first


def test_check_pair_refuses_what_it_should():
    ref = XC.ladder_expected("varying", 50, 1)
    p = next(p for p in range(ref.total.size) if ref.full[p][1].size > 12)
    ok = (ref.total[p], ref.ids[p].copy(), ref.val[p].copy())
    XC.check_pair(*ok, ref.full[p], 10)
    swapped = (ok[0], ok[1][[1, 0] + list(range(2, 10))], ok[2][[1, 0] + list(range(2, 10))])
    off = (ok[0], ok[1], ok[2] * (1 + 1e-8))
    src, e = ref.full[p]
    o = np.lexsort((src, -e))
    dropped = (ok[0], np.concatenate([ok[1][1:], src[o[10:11]]]), np.concatenate([ok[2][1:], e[o[10:11]]]))
    for bad in (swapped, off, dropped, (ok[0] * (1 + 1e-8) + 1e-9, ok[1], ok[2])):
        with pytest.raises(AssertionError):
            XC.check_pair(*bad, ref.full[p], 10)


# ---- the Python layer's refusals: no GPU needed ------------------------------------------------------------

def _model(loaded, **params):
    from albedo_amd import ALS, ALSModel
    m = ALSModel.__new__(ALSModel)
    m._p = dict(ALS(**params)._p)
    m._loaded = loaded
    return m


def test_explain_np_on_a_loaded_model_needs_its_parameters():
    e = np.zeros(0, np.int32)
    with pytest.raises(ValueError, match="regParam"):
        _model(True).explain_np(e, e, np.zeros(0, np.float32), e, e)
    with pytest.raises(ValueError, match="dataset"):
        import pandas as pd
        _model(True).explain(pd.DataFrame({"user": [1], "item": [2]}), regParam=0.1, alpha=1.0, implicitPrefs=True)


def test_explain_np_refuses_a_nonnegative_model():
    e = np.zeros(0, np.int32)
    m = _model(False, regParam=0.5, alpha=10.0, implicitPrefs=True, nonnegative=True)
    with pytest.raises(ValueError, match="not linear"):
        m.explain_np(e, e, np.zeros(0, np.float32), e, e)

"""The cases of tests/query_cases.py hold what the GPU tests rely on (no GPU needed): tie widths, which
exclusions hit the unexcluded top-k, distinct scores where a case needs them, short lists where a case says
so, and the expected answer itself against the Python oracle."""
import numpy as np

from oracle import spark_als as O
from tests import query_cases as QC


def _scores(case, i, rows=None):
    s = QC.scores(case["q"][i:i + 1], case["F"])[0]
    return s if rows is None else s[rows]


def test_expected_agrees_with_the_python_oracle():
    case = QC.random_case(257, 5, 30, 6)
    got = QC.expected(case)
    for i in range(5):
        keep = QC.kept_rows(case, i)
        assert 0 < (~keep).sum() < 40
        want = O.recommend_for_all([0], case["q"][i:i + 1], case["dst_ids"][keep], case["F"][keep], 30)
        assert QC.same((got[0][i:i + 1], got[1][i:i + 1]), want)
    # the exclusions matter: every query loses members of its unexcluded top-k
    plain = QC.expected(dict(case, excl=None))
    assert all(np.isin(plain[0][i], case["excl"][i]).sum() >= 10 for i in range(5))
    assert not any(np.isin(got[0][i], case["excl"][i]).any() for i in range(5))


def test_sizes_cover_the_edges():
    for k in QC.KS:
        sizes = [QC.size(n, k) for n in QC.SIZES]
        assert sizes[:4] == [1, k - 1, k, k + 1] and sizes[4:] == [255, 256, 257, 1000]
    assert QC.SLICE_ROWS == 256
    c = QC.random_case(5, 3, 30, 6)  # fewer rows than k: short lists, dense, padded
    ids, sc = QC.expected(c)
    n = (ids != -1).sum(axis=1)
    assert np.all(n <= 5) and np.all(np.isnan(sc) == (np.arange(30)[None, :] >= n[:, None]))


def test_boundary_tie():
    c = QC.boundary_tie_case()
    k, rep, better, ids = c["k"], c["rep"], c["better"], c["dst_ids"]
    s = _scores(c, 0)
    assert np.all(s[rep] == s[rep[0]]) and rep.size == 3 * k          # the tie is 3k wide, exactly
    assert np.all(s[better] == 2 * s[rep[0]])
    others = np.setdiff1d(np.arange(ids.size), np.concatenate([rep, better]))
    assert s[others].max() < s[rep[0]]
    assert (rep < QC.SLICE_ROWS).sum() == 4 and (rep >= QC.SLICE_ROWS).sum() == 3 * k - 4  # both slices
    e_ids, e_sc = QC.expected(c)
    assert e_ids[0].tolist() == ids[rep[:k]].tolist()                  # the lowest ids, from both slices
    assert e_ids[1].tolist() == ids[better].tolist() + ids[rep[:k - 4]].tolist()
    assert e_ids[2].tolist() == ids[better].tolist() + ids[np.delete(rep, 2)[:k - 4]].tolist()
    assert np.isin(c["excl"][2], e_ids[1]).all()                       # the excluded one was a kept member


def test_zeros_and_signs():
    c = QC.zero_and_sign_case()
    ids, zero, k = c["dst_ids"], c["zero"], c["k"]
    s0, s1 = _scores(c, 0), _scores(c, 1)
    assert np.all(QC.bits(s0) == 0)                                    # +0.0, though products are -0.0
    assert np.signbit(c["F"][zero[:3], 0]).all()
    assert np.all(s1[zero] == 0) and np.all(np.delete(s1, zero) < 0)
    e_ids, e_sc = QC.expected(c)
    assert e_ids[0].tolist() == ids[:k].tolist()
    assert e_ids[1][:6].tolist() == ids[zero].tolist() and np.all(e_sc[1][6:] < 0)
    assert (zero < QC.SLICE_ROWS).any() and (zero >= QC.SLICE_ROWS).any()


def test_nonfinite():
    c = QC.nonfinite_case()
    ids = c["dst_ids"]
    s0, s1 = _scores(c, 0), _scores(c, 1)
    assert np.isnan(s0[10]) and s0[20] == np.inf and s0[280] == -np.inf
    assert np.isnan(s1[[10, 20, 280]]).all() and np.isnan(s1).sum() == 3
    e_ids, e_sc = QC.expected(c)
    assert e_ids[0][0] == ids[20] and e_sc[0][0] == np.inf and not np.isin(ids[[10, 280]], e_ids[0]).any()
    assert not np.isin(ids[[10, 20, 280]], e_ids[1]).any() and not np.isnan(e_sc[:2]).any()
    assert e_ids[2].tolist() == [ids[20], ids[100], ids[280], -1, -1, -1]  # -inf listed last, then padding
    assert e_sc[2][2] == -np.inf and np.isnan(e_sc[2][3:]).all()


def test_exclusion_contract():
    c = QC.exclusion_case()
    ids, k, top, ex = c["dst_ids"], c["k"], c["unexcluded_top"], c["excl"]
    s = _scores(c, 0)
    assert np.unique(s).size == s.size                                 # no two listed scores are equal
    assert ids[0] == QC.I32_MIN and ids[-1] == QC.I32_MAX
    assert set(top[0][:2].tolist()) == {QC.I32_MIN, QC.I32_MAX}        # the edge ids lead the plain list
    e_ids, e_sc = QC.expected(c)
    assert ex[1].size == 0 and ex[0].size and ex[2].size              # an empty range between non-empty ones
    assert not np.isin(ex[0], top[0]).any() and e_ids[0].tolist() == top[0].tolist() == e_ids[1].tolist()
    assert np.isin(top[2], ex[2]).all() and not np.isin(e_ids[2], top[2]).any() and (e_ids[2] != -1).all()
    assert np.all(e_ids[3] == -1) and np.isnan(e_sc[3]).all()          # every row excluded
    assert (e_ids[4] != -1).sum() == k - 1 and e_ids[4][-1] == -1      # short list
    assert np.unique(ex[5]).size < ex[5].size and (~np.isin(ex[5], ids)).sum() >= 3  # copies and unknown ids
    assert np.isin(top[5][:3], ex[5]).all() and not np.isin(e_ids[5], ex[5]).any()
    assert not np.isin([QC.I32_MIN, QC.I32_MAX], e_ids[6]).any() and e_ids[6].tolist() != top[6].tolist()
    assert sorted(ex[7].tolist()) == sorted(ex[5].tolist()) and ex[7].tolist() != ex[5].tolist()
    assert e_ids[7].tolist() == e_ids[5].tolist()
    sh = QC.shuffled(c)
    assert any(a.tolist() != b.tolist() for a, b in zip(sh["excl"], ex))
    assert QC.same(QC.expected(sh), (e_ids, e_sc))


def test_own_factor_leads():
    c = QC.own_factor_case()
    s = _scores(c, 0)
    lead = c["lead"]
    assert s[lead] > 8.9 and np.delete(s, lead).max() < 3.01           # 9 against at most 3
    assert QC.expected(c)[0][0][0] == c["dst_ids"][lead]


def test_excl_csr():
    ptr, ids = QC.excl_csr([[3, 1], [], [2]])
    assert ptr.tolist() == [0, 2, 2, 3] and ids.tolist() == [3, 1, 2] and ptr.dtype == np.int64 and ids.dtype == np.int32

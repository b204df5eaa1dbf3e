"""CPU oracle checks: known answers from Spark's own test suites, LAPACK, scipy, the C restatement
and the committed golden fixtures (the oracle is test infrastructure; see oracle/__init__.py)."""
import os

import numpy as np
import pytest
import scipy.optimize

from oracle import cbind
from oracle import spark_als as O
from tests.conftest import GOLDEN


def test_ndcg_known_answers():
    # mllib RankingMetricsSuite (Spark 2.2.0): the three-user fixture and its published values
    pairs = [([1, 6, 2, 7, 8, 3, 9, 10, 4, 5], [1, 2, 3, 4, 5]),
             ([4, 1, 5, 6, 2, 7, 3, 8, 9, 10], [1, 2, 3]),
             ([1, 2, 3, 4, 5], [])]
    assert O.ndcg_at(pairs, 3) == pytest.approx(1.0 / 3, abs=1e-8)
    assert O.ndcg_at(pairs, 5) == pytest.approx(0.328788, abs=1e-6)
    assert O.ndcg_at(pairs, 10) == pytest.approx(0.487913, abs=1e-6)
    assert O.ndcg_at(pairs, 15) == pytest.approx(0.487913, abs=1e-6)
    with pytest.raises(ValueError):
        O.ndcg_at(pairs, 0)


def test_product_ndcg_matches_oracle():
    from albedo_amd import evaluation as E
    rng = np.random.default_rng(0)
    pairs = [(list(rng.permutation(50)[:30]), list(rng.permutation(50)[: rng.integers(0, 40)])) for _ in range(40)]
    for k in (1, 5, 30):
        assert E.ndcg_at(pairs, k) == pytest.approx(O.ndcg_at(pairs, k), abs=1e-12)


def test_cholesky_is_lapack_dppsv():
    rng = np.random.default_rng(1)
    for k in (1, 8, 50):
        M = rng.standard_normal((k + 3, k))
        A = M.T @ M
        b = rng.standard_normal(k)
        x = O.cholesky_solve(A, b, 0.3)
        ref = np.linalg.solve(A + 0.3 * np.eye(k), b)
        assert np.allclose(x, ref.astype(np.float32), rtol=1e-5, atol=1e-6)
    with pytest.raises(O.NotPositiveDefinite):
        O.cholesky_solve(np.zeros((4, 4)), np.ones(4), 0.0)


def test_nnls_reaches_scipy_optimum():
    rng = np.random.default_rng(2)
    for n in (4, 16, 32):
        M = rng.standard_normal((3 * n, n))
        y = rng.standard_normal(3 * n)
        A, b = M.T @ M, M.T @ y
        x = O.nnls(A, b)
        ref, _ = scipy.optimize.nnls(M, y)
        assert np.all(x >= 0)
        assert np.allclose(x, ref, rtol=1e-6, atol=1e-6)


def test_f2j_sdot_is_sequential_float32():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 23)).astype(np.float32)
    y = rng.standard_normal((5, 23)).astype(np.float32)
    got = O.f2j_sdot(x, y)
    for r in range(5):
        acc = np.float32(0)
        for i in range(23):
            acc = np.float32(acc + np.float32(x[r, i] * y[r, i]))
        assert got[r] == acc


def test_bounded_priority_queue_matches_sorted_topk():
    rng = np.random.default_rng(4)
    scores = rng.integers(0, 20, size=200).astype(np.float32)  # many ties
    ids = np.arange(200)
    q = O.BoundedPriorityQueue(10, key=lambda e: e[1])
    for i in ids:  # ascending id order: first seen = lower id
        q.add((int(i), float(scores[i])))
    kept = sorted(q.items(), key=lambda e: (-e[1], e[0]))
    order = np.lexsort((ids, -scores))[:10]
    assert [e[0] for e in kept] == list(order)


def test_numpy_oracle_matches_c_oracle():
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(300, 120, 3000, seed=5))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    rng = np.random.default_rng(5)
    for implicit in (True, False):
        Y = rng.standard_normal((len(B.user_ids), 12)).astype(np.float32)
        a = O.half_sweep(Y, B.i_ptr, B.i_col, B.i_val, reg=0.5, alpha=40.0, implicit=implicit)
        b = cbind.half_sweep(Y, B.i_ptr, B.i_col, B.i_val, reg=0.5, alpha=40.0, implicit=implicit)
        assert np.allclose(a, b, rtol=1e-6, atol=1e-7)
    assert np.allclose(cbind.gram(Y), O.gram(Y), rtol=1e-12)


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def test_oracle_reproduces_golden_f1_f2():
    f = _load("f1_half_sweep.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    for k in (8, 16):
        V = O.half_sweep(f[f"U0_k{k}"], B.i_ptr, B.i_col, B.i_val, reg=0.5, alpha=40.0)
        assert np.array_equal(V, f[f"V_k{k}"])
    f = _load("f2_three_sweeps.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    U, V = O.fit(B, rank=16, max_iter=3, reg=0.5, alpha=40.0, init_user=f["U0"], init_item=f["V0"])
    assert np.array_equal(U, f["U"]) and np.array_equal(V, f["V"])


def test_oracle_reproduces_golden_topk():
    f = _load("f4_topk_ties.npz")
    ids, sc = O.recommend_for_all(f["uid"], f["uf"], f["iid"], f["itf"], 30)
    assert np.array_equal(ids, f["ids30"]) and np.array_equal(sc, f["sc30"])


def test_into_user_items_rank_keeps_ties():
    from albedo_amd import evaluation as E
    user = np.array([1, 1, 1, 1, 2, 2])
    item = np.array([10, 11, 12, 13, 20, 21])
    key = np.array([5.0, 7.0, 7.0, 1.0, 3.0, 3.0])
    a = O.into_user_items(user, item, key, 1)
    b = E.into_user_items(user, item, key, 1)
    assert a == b == {1: [11, 12], 2: [20, 21]}


def test_synthetic_generator_shape():
    from albedo_amd.synthetic import SynthSpec, generate, user_degrees
    spec = SynthSpec(2000, 400, 30000, seed=9)
    d = generate(spec)
    key = d["user"].astype(np.int64) * (1 << 31) + d["item"]
    assert np.unique(key).size == key.size  # unique (user, repo) pairs, like app/models.py:166-167
    assert user_degrees(spec).sum() == spec.nnz
    assert key.size >= 0.99 * spec.nnz
    assert np.all(d["rating"] == 1.0)


def test_c_topk_oracle_matches_numpy_oracle_and_golden():
    """The C/OpenMP scorer (full-size parity checks) equals the numpy restatement bit for bit:
    golden F4 (engineered ties), a catalogue that is not a multiple of the 64-row block, duplicate
    rows (equal scores, id tie-break), k above the catalogue size."""
    f = _load("f4_topk_ties.npz")
    for num in (30, 60):
        ids, sc = cbind.recommend(f["uf"], f["iid"], f["itf"], num)
        assert np.array_equal(ids, f[f"ids{num}"]) and np.array_equal(sc.view(np.uint32), f[f"sc{num}"].view(np.uint32))
    rng = np.random.default_rng(3)
    n_i, k = 1000, 37
    iid = rng.permutation(np.arange(n_i, dtype=np.int32) * 7 - 300)
    itf = (rng.standard_normal((n_i, k)) * rng.lognormal(0, 1, (n_i, 1))).astype(np.float32)
    itf[500:540] = itf[:40]
    uf = rng.standard_normal((45, k)).astype(np.float32)
    for num in (1, 30, 64):
        a = O.recommend_for_all(np.arange(45), uf, iid, itf, num)
        b = cbind.recommend(uf, iid, itf, num, threads=3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    a = O.recommend_for_all(np.arange(5), uf[:5], iid[:20], itf[:20], 30)
    b = cbind.recommend(uf[:5], iid[:20], itf[:20], 30)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][:, :20], b[1][:, :20]) and np.all(np.isnan(b[1][:, 20:]))


def test_c_nnls_matches_numpy_nnls_on_f5():
    """The C/OpenMP NNLSSolver restatement (oracle/c/als_cpu.c, the c5 bench's cpu_baseline) equals the
    numpy restatement of NNLS.scala (oracle/spark_als.py:nnls) on the F5 golden rows: the committed
    item half-sweep V1 from U0, and the user half-sweep from V1, row by row."""
    f = _load("f5_nnls.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    U0 = f["U0"].astype(np.float32)
    V, it = cbind.solve_rows_nnls(U0, O.gram(U0), B.i_ptr, B.i_col, B.i_val, reg=0.5, alpha=40.0, threads=4)
    assert np.all(V >= 0) and np.all(it > 0)
    assert np.allclose(V, f["V1"], rtol=1e-6, atol=1e-7)
    U, _ = cbind.solve_rows_nnls(V, O.gram(V), B.u_ptr, B.u_col, B.u_val, reg=0.5, alpha=40.0, threads=3)
    U_ref = O.half_sweep(V, B.u_ptr, B.u_col, B.u_val, reg=0.5, alpha=40.0, nonnegative=True)
    assert np.allclose(U, U_ref, rtol=1e-6, atol=1e-7)
    assert np.mean((U == 0) == (U_ref == 0)) == 1.0


# ---- rating modes: non-unit, signed and zero ratings (tests/test_gpu_rating_modes.py relies on these) ----

def _signed_small_set():
    """A small set with non-unit, negative and exactly-zero ratings, and rows without a positive one."""
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(300, 120, 3000, seed=6))
    rng = np.random.default_rng(6)
    r = rng.choice([0.25, 0.5, 1.0, 2.0, 3.0, 5.0], d["user"].size)
    r[rng.random(r.size) < 0.15] = 0.0
    r = np.where(rng.random(r.size) < 0.25, -r, r) + 0.0
    nonpos = np.isin(d["item"], np.unique(d["item"])[:3])
    r[nonpos] = -np.abs(r[nonpos]) + 0.0
    B = O.make_blocks(d["user"], d["item"], r)
    assert (B.i_val < 0).any() and (B.i_val == 0).any()
    npos = np.add.reduceat(B.i_val > 0, B.i_ptr[:-1])
    assert (npos == 0).any() and (npos > 0).any()
    return B


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
def test_c_oracle_matches_numpy_oracle_on_signed_nonunit_ratings(implicit):
    """cbind.half_sweep (Cholesky) and cbind.solve_rows_nnls against the numpy oracle on non-unit,
    negative and zero ratings, implicit and explicit, both halves (tolerances of
    test_numpy_oracle_matches_c_oracle / test_c_nnls_matches_numpy_nnls_on_f5)."""
    B = _signed_small_set()
    rng = np.random.default_rng(7)
    alpha, reg = (10.0, 0.5) if implicit else (1.0, 0.1)
    for ptr, col, val, n_src in ((B.i_ptr, B.i_col, B.i_val, len(B.user_ids)), (B.u_ptr, B.u_col, B.u_val, len(B.item_ids))):
        Y = rng.standard_normal((n_src, 12)).astype(np.float32)
        a = O.half_sweep(Y, ptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
        b = cbind.half_sweep(Y, ptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
        assert np.allclose(a, b, rtol=1e-6, atol=1e-7)
        Yn = np.abs(Y)
        Yn[:, ::5] *= -1.0
        a = O.half_sweep(Yn, ptr, col, val, reg=reg, alpha=alpha, implicit=implicit, nonnegative=True)
        b, it = cbind.solve_rows_nnls(Yn, O.gram(Yn), ptr, col, val, reg=reg, alpha=alpha, implicit=implicit, threads=3)
        assert np.all(b >= 0) and (a == 0).any() and (a > 0).any()
        assert np.allclose(a, b, rtol=1e-6, atol=1e-7)
        assert np.mean((a == 0) == (b == 0)) == 1.0


def _solve_rows64(Y, ptr, col, val, implicit, alpha, reg, mistake=None):
    """fp64 solutions of Spark's normal equations, row by row; `mistake` restates one plausible kernel
    bug: "mask_zero" (explicit ratings of 0 left out of A), "cmax" (every implicit confidence taken
    as alpha·max|r|), "nosign" (the sign of r ignored in b's weight)."""
    Y = np.asarray(Y, np.float64)
    k = Y.shape[1]
    G = Y.T @ Y if implicit else np.zeros((k, k))
    rmax = float(np.max(np.abs(val)))
    X = np.zeros((len(ptr) - 1, k))
    for j in range(len(ptr) - 1):
        Yj = Y[col[ptr[j]:ptr[j + 1]]]
        r = val[ptr[j]:ptr[j + 1]].astype(np.float64)
        if implicit:
            c = alpha * (np.full(r.size, rmax) if mistake == "cmax" else np.abs(r))
            w = np.where((r != 0) if mistake == "nosign" else (r > 0), 1.0 + c, 0.0)
            n = int(np.sum(r > 0))
        else:
            c = np.where(r == 0, 0.0, 1.0) if mistake == "mask_zero" else np.ones(r.size)
            w, n = r, r.size
        X[j] = np.linalg.solve(G + (Yj.T * c) @ Yj + reg * n * np.eye(k), Yj.T @ w)
    return X


@pytest.mark.parametrize("mode,mistake", [("stars_signed", "mask_zero"), ("varying", "cmax"), ("mixed", "cmax"),
                                          ("signed_uniform", "nosign"), ("mixed", "nosign")])
def test_ladder_inputs_expose_wrong_rating_weights(mode, mistake):
    """The ladder inputs tell a kernel with a plausible rating-weight bug from a right one: on every
    row the bug touches (with a non-zero solution, or a zero one the bug makes non-zero) the mistaken
    fp64 solution is more than 10x the GPU tolerance (1e-4) away from the oracle's: item half at ranks
    50 / 128 / 256.  On the user half (rank 50, from the oracle's own item factors, whose rows differ in
    size by orders of magnitude) the same holds for more than 90 % of the touched rows."""
    from tests import ladder as LD
    implicit, alpha, reg = LD.MODES[mode]
    user, item, ideg = LD.ladder_coo()
    B = O.make_blocks(user, item, LD.ladder_ratings(mode, user, ideg))

    def touched(Y, col, val, ptr):  # a rating the bug treats differently, on a src row that is not all zero
        hit = {"mask_zero": val == 0, "cmax": np.abs(val) != np.max(np.abs(val)), "nosign": val < 0}[mistake]
        return np.add.reduceat(hit & Y[col].any(axis=1), ptr[:-1]) > 0

    def check(Y, ptr, col, val, what, every=True):
        good = _solve_rows64(Y, ptr, col, val, implicit, alpha, reg)
        ref = O.half_sweep(Y, ptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
        assert LD.row_errors(good, ref).max() < 1e-6  # the helper restates the oracle
        dev = LD.row_errors(_solve_rows64(Y, ptr, col, val, implicit, alpha, reg, mistake), good)
        rows = touched(Y, col, val, ptr) & (good.any(axis=1) | (dev > 0))
        assert rows.sum() >= 20, what
        if every:
            assert dev[rows].min() > 10 * 1e-4, (what, float(dev[rows].min()))
        assert np.mean(dev[rows] > 10 * 1e-4) > 0.9, what
        return ref

    for k in (50, 128, 256):
        V = check(LD.unit_rows(np.random.default_rng(k), len(B.user_ids), k), B.i_ptr, B.i_col, B.i_val, f"item k={k}")
        if k == 50:
            check(V, B.u_ptr, B.u_col, B.u_val, "user k=50", every=False)


def test_ladder_data_and_path_labels():
    """The ladder holds every degree twice, every configuration's expected paths have at least 2 rows
    on the item side (and light16 pairs, light16 and D = 32 on the user side), `mixed` has at least 4
    item rows without a positive rating, and every user keeps a positive rating in the implicit modes."""
    from tests import ladder as LD
    user, item, ideg = LD.ladder_coo()
    assert 6000 < user.size < 7500 and np.any(np.diff(user) < 0)  # shuffled COO
    assert np.unique(user.astype(np.int64) << 32 | item).size == user.size
    assert np.max(np.diff(np.unique(user))) > 1  # sparse raw ids
    B = O.make_blocks(user, item, np.ones(user.size, np.float32))
    deg_i, deg_u = np.diff(B.i_ptr), np.diff(B.u_ptr)
    assert sorted(deg_i.tolist()) == sorted(LD.LADDER + LD.LADDER)
    assert 650 <= len(B.user_ids) <= 700 and 16 < deg_u.max() <= 32
    assert LD.path_of(8, 64, -1, 8192) == "light16-pair" and LD.path_of(9, 64, -1, 8192) == "light16"
    assert LD.path_of(32, 64, -1, 8192) == "light32" and LD.path_of(33, 64, -1, 8192) == "wave"
    assert LD.path_of(64, 128, -1, 8192) == "light64" and LD.path_of(65, 128, -1, 8192) == "wave"
    assert LD.path_of(96, 128, 96, 8192) == "light96" and LD.path_of(97, 128, 96, 8192) == "wave"
    assert LD.path_of(64, 256, -1, 8192) == "light64" and LD.path_of(65, 256, 96, 8192) == "heavy"
    assert LD.path_of(256, 256, -1, 256) == "heavy" and LD.path_of(257, 256, -1, 256) == "split"
    assert LD.path_of(1, 128, 0, 256) == "wave" and LD.path_of(257, 128, 0, 0) == "wave"
    for k, light, chunk in LD.CONFIGS:
        KP, ch = LD.padded_rank(k), LD.split_chunk(chunk or "8192")
        for deg in (deg_i, deg_u):
            paths = np.array([LD.path_of(d, KP, light, ch) for d in deg])
            want = LD.expected_paths(KP, light, ch, int(deg.max()))
            assert set(paths.tolist()) == set(want), (k, light, chunk)
            assert all(np.sum(paths == p) >= 2 for p in want), (k, light, chunk)
    for mode, (implicit, _, _) in LD.MODES.items():
        r = LD.ladder_ratings(mode, user, ideg)
        if implicit:
            assert np.isin(user, user[r > 0]).all(), mode
        if mode == "mixed":
            Bm = O.make_blocks(user, item, r)
            npos = np.add.reduceat(Bm.i_val > 0, Bm.i_ptr[:-1])
            assert np.sum(npos == 0) >= 4
            assert set(np.diff(Bm.i_ptr)[npos == 0].tolist()) >= set(LD.NONPOS_DEGREES)
        if mode in ("mixed", "stars_signed"):
            assert 0.08 < np.mean(r == 0) < 0.2 and (r < 0).any()
        if mode == "signed_uniform":
            assert set(np.unique(r).tolist()) == {-2.0, 2.0} and 0.2 < np.mean(r < 0) < 0.35


def test_assert_rows_names_the_failing_row(tmp_path):
    """The failure report of the rating-mode tests: one row off by 1 % is named with its raw id, degree
    and path label, and its got / ref are saved; an all-zero reference row must be exactly zero."""
    from tests import ladder as LD
    rng = np.random.default_rng(8)
    ref = rng.standard_normal((40, 16)).astype(np.float32)
    ref[5] = 0.0
    ids = np.arange(40, dtype=np.int32) * 37 + 1000
    deg = np.arange(40) + 1
    paths = [LD.path_of(d, 128, -1, 8192) for d in deg]
    got = ref + 1e-6 * np.abs(ref).max(axis=1, keepdims=True) * rng.uniform(-1, 1, ref.shape).astype(np.float32)
    assert LD.assert_rows(got, ref, ids, deg, paths, 1e-4, "clean", tmp_path) < 2e-6
    got[17] *= 1.01
    with pytest.raises(AssertionError) as e:
        LD.assert_rows(got, ref, ids, deg, paths, 1e-4, "item half [mixed-k128]", tmp_path)
    msg = str(e.value)
    assert "1 of 40 rows" in msg and f"id {ids[17]} degree 18 path light32" in msg and "item half [mixed-k128]" in msg
    saved = np.load(msg.rsplit("saved to ", 1)[1].strip())
    assert saved["ids"].tolist() == [ids[17]] and saved["deg"].tolist() == [18]
    assert np.array_equal(saved["got"][0], got[17]) and np.array_equal(saved["ref"][0], ref[17])
    got[17] = ref[17]
    got[5, 3] = 1e-30
    with pytest.raises(AssertionError, match=f"id {ids[5]} degree 6 path light16-pair"):
        LD.assert_rows(got, ref, ids, deg, paths, 1e-4, "zero row", tmp_path)
    got[5, 3] = np.nan
    with pytest.raises(AssertionError, match=f"id {ids[5]} "):
        LD.assert_rows(got, ref, ids, deg, paths, 1e-4, "nan", tmp_path)


# ---- the top-k edge cases (tests/topk_cases.py) --------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _normal_or_zero(a):
    a = np.abs(np.asarray(a, np.float32))
    return bool(np.all(np.isfinite(a)) and not np.any((a != 0) & (a < np.finfo(np.float32).tiny)))


@pytest.mark.parametrize("rank", [1, 2, 3, 4, 5, 50, 100, 200])
def test_topk_edge_case_preconditions(rank):
    """What each generator of tests/topk_cases.py promises, asserted with the oracle alone, so that a
    failure of tests/test_gpu_topk_edges.py is about the kernel and not about its inputs."""
    from tests import topk_cases as TC
    CH = TC.chunk_rows(rank)
    for gen, args in (("negative", (rank,)), ("mass_tie", (rank,)), ("zeros", (rank,)), ("group_ties", (rank, 4))):
        uid, _, iid, _ = TC.case(gen, *args)
        for ids in (uid, iid):  # sparse, shuffled, partly negative, distinct
            assert np.unique(ids).size == ids.size and ids.min() < 0 < ids.max()
            assert np.any(np.diff(ids) < 0) and np.ptp(ids.astype(np.int64)) > 4 * ids.size
    # negative: every listed score below 0, and the last chunk is padded
    uid, uf, iid, itf = TC.case("negative", rank)
    assert iid.size > TC.TOPK_KC and iid.size % CH != 0 and uid.size == 77
    _, ids, sc = TC.oracle_lists("negative", (rank,), 64)
    assert np.all(ids >= iid.min()) and np.all(sc < 0)
    # mass_tie: the list is the k smallest ids of the 300 identical rows, one score throughout
    uid, uf, iid, itf = TC.case("mass_tie", rank)
    tied = TC.mass_tie_ids(iid, itf)
    assert tied.size == 300 > TC.TOPK_CAP
    for k in (30, 64):
        _, ids, sc = TC.oracle_lists("mass_tie", (rank,), k)
        assert np.array_equal(ids, np.broadcast_to(tied[:k], ids.shape))
        assert np.array_equal(_bits(sc[:, 0]), _bits(sc[:, k - 1]))
    # group_ties: the k-th and the (k+1)-th score are one value for every src row
    for k, copies in TC.GROUP_TIES.items():
        _, ids, sc = TC.oracle_lists("group_ties", (rank, copies), k + 1)
        assert np.array_equal(_bits(sc[:, k - 1]), _bits(sc[:, k])), (k, copies)
        assert np.all(ids[:, k - 1] < ids[:, k])
    # zeros: all-zero lists, k-th scores of exactly 0, and +0.0 only (F2J's sum starts from +0.0)
    uid, uf, iid, itf = TC.case("zeros", rank)
    assert 0.3 < np.mean(~itf.any(axis=1)) < 0.5 and np.sum(~uf.any(axis=1)) >= 10
    for k in (30, 64):
        for swap in (False, True):
            _, ids, sc = TC.oracle_lists("zeros", (rank,), k, swap)
            assert not np.any(_bits(sc) == 0x80000000), (k, swap)
            if not swap:
                assert np.sum(np.all(sc == 0, axis=1)) >= 10, k
                assert np.mean(sc[:, k - 1] == 0) >= 0.2, (k, float(np.mean(sc[:, k - 1] == 0)))
    if rank < 50:
        return
    # dynamic_range: no product and no score is subnormal or overflows, so the case says nothing
    # about subnormal handling
    for kind in TC.DYNAMIC_KINDS:
        uid, uf, iid, itf = TC.case("dynamic_range", rank, kind)
        assert TC.products_are_normal(uf, itf), kind
        assert _normal_or_zero(O.f2j_sdot(uf[:, None, :], itf[None, :, :])), kind
        nrm = np.linalg.norm(itf.astype(np.float64), axis=1)
        if kind == "dst_spread":
            assert nrm.max() / np.median(nrm) > 1e4 and nrm.max() / nrm.min() > 1e7
        if kind == "src_spread":
            snrm = np.linalg.norm(uf.astype(np.float64), axis=1)
            assert snrm.max() / snrm.min() > 1e6
        if kind == "dst_tiny":  # 13 - ceil(log2 max norm) is above pow2_scale's upper clamp of 60
            assert 13 - np.frexp(nrm.max())[1] > 60
        if kind == "dst_huge":
            assert np.frexp(nrm.max())[1] > 60
    # anisotropic: half of the src rows on the negative side of the leading direction
    uid, uf, iid, itf = TC.case("anisotropic", rank)
    w, V = np.linalg.eigh(itf.astype(np.float64).T @ itf.astype(np.float64))
    lead = uf.astype(np.float64) @ V[:, -1]
    assert 0.4 < np.mean(lead < 0) < 0.6 and w[-1] > 5 * w[-3]
    # the size grid holds every boundary once
    grid = TC.size_grid(rank)
    assert set(TC.size_n_dst(rank)) | {100, 1000} == set(grid) and len(TC.size_n_dst(rank)) == 13
    assert {1, 2, 63, 64, 65, CH - 1, CH, CH + 1, 511, 512, 513, 16 * CH - 1, 16 * CH + 1} <= set(grid)
    assert all((67, k) in grid[n] for n in TC.size_n_dst(rank) for k in (1, 30, 64))
    assert all((n, 30) in grid[16 * CH + 1] for n in TC.SIZE_N_SRC) and len(TC.SIZE_N_SRC) == 13
    assert all((67, k) in grid[1000] for k in TC.SIZE_K_AT_1000) and len(TC.SIZE_K_AT_1000) == 13
    assert all((67, k) in grid[100] for k in TC.SIZE_K_AT_100)


@pytest.mark.parametrize("rank", [3, 50])
def test_topk_edge_case_lists_two_restatements(rank):
    """The expected lists of the tie, zero-row and negative-score cases from the numpy oracle and from
    the C restatement: ids and score bits equal."""
    from tests import topk_cases as TC
    for gen in ("mass_tie", "zeros", "negative"):
        uid, uf, iid, itf = TC.case(gen, rank)
        for k in (30, 64):
            src, ids, sc = TC.oracle_lists(gen, (rank,), k)
            order = np.argsort(uid, kind="stable")
            assert np.array_equal(src, uid[order])
            cid, csc = cbind.recommend(uf[order], iid, itf, k, threads=4)
            assert np.array_equal(ids, cid), (gen, k)
            assert np.array_equal(_bits(sc), _bits(csc)), (gen, k)


# ---- the ingest edge cases (tests/ingest_cases.py) -----------------------------------------------

def test_ingest_edge_case_preconditions():
    """What the generators of tests/ingest_cases.py promise: the extreme ids survive the int32 cast on
    both sides, the top-bit and bit-0 pairs differ in that bit alone, the duplicated pairs sit in rows
    of every listed degree in both orientations with the listed copy counts and different ratings
    (one pair +r / -r), the degenerate shapes and sizes are what their names say, and every COO
    arrives shuffled."""
    from tests import ingest_cases as IC
    user, item, r = IC.case("extreme_ids")
    assert user.dtype == item.dtype == np.int32 and r.dtype == np.float32
    for ids in (user, item):
        assert set(IC.EXTREME_IDS) <= set(ids.tolist()) and set(IC.special_ids()) <= set(ids.tolist())
        assert np.unique(ids).size >= 128 and np.any(np.diff(ids.astype(np.int64)) < 0)
    assert all((a ^ b) & 0xFFFFFFFF == 0x80000000 for a, b in IC.TOP_BIT_PAIRS)
    assert all((a ^ b) == 1 for a, b in IC.BIT0_PAIRS) and np.all(r > 0)
    B = O.make_blocks(user, item, r)
    assert B.user_ids[0] == IC.I32_MIN and B.user_ids[-1] == IC.I32_MAX and np.all(np.diff(B.user_ids.astype(np.int64)) > 0)
    assert B.item_ids[0] == IC.I32_MIN and B.item_ids[-1] == IC.I32_MAX

    user, item, r = IC.case("duplicates")
    B = O.make_blocks(user, item, r)
    assert IC.dup_rows() == [(8, 2), (8, 3), (16, 2), (16, 3), (17, 2), (17, 3), (64, 2), (64, 3), (64, 64),
                             (65, 2), (65, 3), (65, 64)]
    for ids, ptr, col, val in ((B.user_ids, B.u_ptr, B.u_col, B.u_val), (B.item_ids, B.i_ptr, B.i_col, B.i_val)):
        assert np.unique(ids).size >= 128  # the Gram of either side has full rank at rank 128
        for d, c in IC.dup_rows():
            j = int(np.searchsorted(ids, 700000 + 1000 * d + c))
            assert ids[j] == 700000 + 1000 * d + c and ptr[j + 1] - ptr[j] == d, (d, c)
            cols, cnt = np.unique(col[ptr[j]:ptr[j + 1]], return_counts=True)
            assert sorted(cnt.tolist()) == [1] * (d - c) + [c], (d, c)
            rr = val[ptr[j]:ptr[j + 1]][col[ptr[j]:ptr[j + 1]] == cols[np.argmax(cnt)]]
            assert np.unique(rr).size == c, (d, c)
            if c == 2:
                assert sorted(rr.tolist()) == [-2.5, 2.5]
    # the copies also land in ordinary rows of the other orientation, which then hold > 64 ratings
    assert np.diff(B.u_ptr).max() >= 64 and np.diff(B.i_ptr).max() >= 64

    assert IC.case("single")[0].size == 1
    for name, nu, ni, n in (("one_user", 1, 300, 300), ("one_item", 300, 1, 300), ("one_user_repeats", 1, 40, 300)):
        user, item, r = IC.case(name)
        assert (np.unique(user).size, np.unique(item).size, user.size) == (nu, ni, n), name
    for v in (255, 256, 257):
        user, item, r = IC.case("square", v)
        assert np.unique(user).size == np.unique(item).size == v and user.size == 4 * v
    for n in (255, 256, 257):
        assert IC.case("sized", n)[0].size == n
    assert IC.N_PAST_CAP == 8192 * 256 + 257 and (255, 256, 257) == tuple(c[1][0] for c in IC.SMALL_CASES[-3:])
    for c in IC.SMALL_CASES[:2] + IC.SMALL_CASES[3:]:
        user, item, r = IC.case(*c[0:1], *c[1])
        assert user.size == item.size == r.size
        assert np.any(np.diff(user.astype(np.int64)) < 0) or np.any(np.diff(item.astype(np.int64)) < 0), c


def test_ingest_past_cap_shape():
    """The case past the grid-stride launch cap: 8192 * 256 + 257 ratings over a few thousand rows per side."""
    from tests import ingest_cases as IC
    user, item, r = IC.case("past_cap")
    assert user.size == IC.N_PAST_CAP > IC.GRID_CAP
    assert 2000 <= np.unique(user).size <= 4000 and 2000 <= np.unique(item).size <= 4000


@pytest.mark.parametrize("k", [50, 128])
def test_duplicates_case_exposes_a_merging_ingest(k):
    """Duplicates enter the normal equation once per copy.  An ingest that merged the copies of a pair
    into one summed rating would change b by (copies - 1)·y, lambda·n by reg·(copies - 1) and, for the
    +r / -r pair, drop the pair altogether: on every row of the duplicates case that holds a
    duplicated pair the oracle on the merged COO is more than 10x the GPU tolerance (1e-4) away from
    the true one, on both halves; rows without a duplicate do not move on the item half."""
    from tests import ingest_cases as IC
    from tests import ladder as LD
    user, item, r = IC.case("duplicates")
    B = O.make_blocks(user, item, r)
    Bm = O.make_blocks(*IC.merge_duplicates(user, item, r))
    assert np.array_equal(B.user_ids, Bm.user_ids) and np.array_equal(B.item_ids, Bm.item_ids)
    assert len(Bm.u_col) < len(B.u_col)
    kw = dict(reg=0.5, alpha=10.0, implicit=True)
    U = LD.unit_rows(np.random.default_rng(k), len(B.user_ids), k)
    V = O.half_sweep(U, B.i_ptr, B.i_col, B.i_val, **kw)
    Vm = O.half_sweep(U, Bm.i_ptr, Bm.i_col, Bm.i_val, **kw)
    X = O.half_sweep(V, B.u_ptr, B.u_col, B.u_val, **kw)
    Xm = O.half_sweep(V, Bm.u_ptr, Bm.u_col, Bm.u_val, **kw)
    for name, a, b, deg, degm in (("item", V, Vm, np.diff(B.i_ptr), np.diff(Bm.i_ptr)),
                                  ("user", X, Xm, np.diff(B.u_ptr), np.diff(Bm.u_ptr))):
        err = LD.row_errors(b, a)
        has_dup = deg != degm
        assert has_dup.sum() >= len(IC.dup_rows()), name
        assert err[has_dup].min() > 10 * 1e-4, (name, float(err[has_dup].min()))
        assert err[~has_dup].max() == 0.0, name


# ---- the NDCG edge cases (tests/eval_cases.py) ----------------------------------------------------

def _into_user_items_float64(user, item, order_key, k):
    """O.into_user_items as it was before it ordered integer keys exactly (keys cast to float64)."""
    user, item = np.asarray(user), np.asarray(item)
    key = np.asarray(order_key, dtype=np.float64)
    order = np.lexsort((item, -key, user))
    u_s, i_s, k_s = user[order], item[order], key[order]
    out = {}
    start = np.r_[0, 1 + np.nonzero(u_s[1:] != u_s[:-1])[0]]
    for a, b in zip(start, np.r_[start[1:], u_s.size]):
        ranks = 1 + np.searchsorted(-k_s[a:b], -k_s[a:b], side="left")
        out[int(u_s[a])] = [int(x) for x in i_s[a:b][ranks <= k]]
    return out


@pytest.mark.parametrize("k", [30, 10])
def test_into_user_items_integer_keys_exact_and_unchanged(k):
    """The integer-exact O.into_user_items returns the lists the float64 version returned on the input
    of test_device_ndcg_matches_oracle (timestamps far below 2^53) and on float keys; it keeps keys
    apart that differ by 1 above 2^53, and orders INT64_MIN (whose negation overflows) last."""
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(2500, 600, 40000, seed=19), with_timestamps=True)
    rng = np.random.default_rng(k)
    ts = d["ts"] // 1_000_000
    dup = rng.choice(d["user"].size, 400, replace=False)
    users = np.r_[d["user"], d["user"][dup], np.full(5, 123456789, np.int32)]
    items = np.r_[d["item"], d["item"][dup], d["item"][:5]]
    keys = np.r_[ts, ts[dup] + 1 + rng.integers(0, 3, dup.size), ts[:5]]
    assert keys.dtype == np.int64 and np.abs(keys).max() < 2 ** 53
    old = _into_user_items_float64(users, items, keys, k)
    assert O.into_user_items(users, items, keys, k) == old
    assert O.into_user_items(users, items, keys.astype(np.float64), k) == old
    assert O.into_user_items(users, items, keys.astype(np.int32) if np.abs(keys).max() < 2 ** 31 else keys, k) == old
    big = 1 << 60
    ky = np.array([big, big + 1, -(1 << 63), (1 << 63) - 1, -5], np.int64)
    it = np.array([1, 2, 0, 9, 3])
    assert O.into_user_items(np.zeros(5, np.int32), it, ky, 5) == {0: [9, 2, 1, 3, 0]}
    assert O.into_user_items(np.zeros(5, np.int32), it, ky, 2) == {0: [9, 2]}
    assert _into_user_items_float64(np.zeros(5, np.int32), it, ky, 2)[0][1] == 1  # the float order: a tie


def test_eval_edge_case_preconditions():
    """What the generators of tests/eval_cases.py promise, asserted with the oracle alone."""
    from tests import eval_cases as EC
    k = 30
    for variant in EC.LENGTH_VARIANTS:
        m, (users, items, keys) = EC.case("lengths", variant)
        who, cnt = np.unique(users, return_counts=True)
        assert sorted(cnt.tolist()) == EC.LENGTHS and np.all(np.isin(who, m[0]))  # every length is present
        assert {1, 29, 30, 31, 63, 64, 65, 127, 128, 129, 200, 1000} == set(cnt.tolist())
        assert np.any(np.diff(users) < 0)
        for u in who:
            ky = keys[users == u]  # the user's rows in input order
            if variant == "ties":
                assert np.all(ky == ky[0])
            if variant == "last64":
                assert np.unique(ky).size == ky.size
                assert np.sort(ky)[-k:][0] <= np.min(np.sort(ky[-64:])[-k:]), u  # the top k are among the last 64 rows
                if ky.size > 128:
                    assert np.max(ky[:-64]) < np.sort(ky)[-k:][0]
        if variant == "random":
            assert any(np.unique(keys[users == u]).size < np.sum(users == u) for u in who)
    # keys: the 2^53 pairs are two int64 keys and one float64, and they decide the k-th place
    m, (users, items, keys) = EC.case("keys")
    assert np.int64(EC.BIG) != np.int64(EC.BIG + 1) and float(EC.BIG) == float(EC.BIG + 1) and EC.BIG > 2 ** 53
    exact, lossy = O.into_user_items(users, items, keys, k), _into_user_items_float64(users, items, keys, k)
    swapped = [u for u in exact if exact[u][:k] != lossy[u][:k]]
    assert len(swapped) >= 40 and all(np.sum((users == u) & (keys >= EC.BIG)) == k + 1 for u in m[0][:40])
    assert {EC.I64_MIN, EC.I64_MAX, -1, 0} <= set(keys.tolist()) and np.sum(keys < 0) > 100
    _, ref_exact, _ = EC.reference("keys", (), k)
    known, pred = EC.predicted_lists(m, users, k)
    ref_lossy = np.array([O.ndcg_at([(pred[int(u)], lossy[int(u)][:k])], k) for u in known])
    assert np.sum(ref_exact != ref_lossy) >= 3  # a float64 order of the keys changes per-user values
    # item id extremes: catalogues of either sign, the special ids, lists shorter than k
    neg, mix, ext = (EC.case("bag", c)[0][2] for c in ("negative", "mixed", "extreme"))
    assert neg.max() < 0 and mix.min() < 0 < mix.max() and {-1, EC.I32_MIN, EC.I32_MAX} <= set(ext.tolist())
    assert EC.case("bag", "five")[0][2].size == 5 and EC.case("bag", "twentynine")[0][2].size == 29
    for kind in EC.CATALOGUES:
        m, (users, items, keys) = EC.case("bag", kind)
        roles = EC.bag_roles()
        actual = O.into_user_items(users, items, keys, k)
        known, vals, mean = EC.reference("bag", (kind,), k)
        val = dict(zip(known.tolist(), vals.tolist()))
        assert set(known.tolist()) == set(sum((roles[r] for r in roles if r != "unknown_users"), []))
        assert not np.isin(roles["unknown_users"], m[0]).any() and np.isin(roles["unknown_users"], users).all()
        assert min(roles["unknown_users"]) < m[0].min() and max(roles["unknown_users"]) > m[0].max()
        assert all(not np.isin(actual[u], m[2]).any() and val[u] == 0.0 for u in roles["unknown_items"])
        assert all(len(set(actual[u])) == 1 for u in roles["one_item"])
        assert any(len(actual[u]) > 1 for u in roles["one_item"])
        sent = (items == EC.I32_MAX) & (keys == EC.I64_MIN)
        assert all(np.sum(sent & (users == u)) >= 1 for u in roles["sentinel"])
        # hits exist, so a kernel that never credits a hit on this catalogue is caught
        assert np.sum(vals > 0) >= 10 and 0 < mean < 1, (kind, int(np.sum(vals > 0)))
        if kind in ("five", "twentynine"):  # n is decided by |labSet| for some users
            known, pred = EC.predicted_lists(m, users, k)
            assert all(len(p) == m[2].size < k for p in pred.values())
            assert any(len(set(actual[int(u)][:k])) > m[2].size for u in known)
    # with hits only at negative ids, dropping them changes the value of most users
    m, (users, items, keys) = EC.case("bag", "negative")
    known, pred = EC.predicted_lists(m, users, k)
    assert all(x < 0 for p in pred.values() for x in p)
    # join edges
    m, (users, items, keys) = EC.case("only_unknown_users")
    assert users.size > 0 and not np.isin(users, m[0]).any()
    known, vals, mean = EC.reference("only_unknown_users", (), k)
    assert known.size == 0 and np.isnan(mean)
    m, (users, items, keys) = EC.case("bag", "mixed", 1)
    assert m[0].size == 1 and EC.reference("bag", ("mixed", 1), k)[0].tolist() == [10]
    assert np.unique(users).size == 7


def test_actual_lists_two_restatements():
    """tests/eval_cases.py actual_lists (one lexsort, first k of each group) equals
    O.into_user_items(...)[:k] on every small case at k = 1, 2, 30, 63, 64."""
    from tests import eval_cases as EC
    for c in EC.SMALL_CASES:
        _, (users, items, keys) = EC.case(c[0], *c[1])
        for k in (1, 2, 30, 63, 64):
            a = EC.actual_lists(users, items, keys, k)
            b = {u: v[:k] for u, v in O.into_user_items(users, items, keys, k).items()}
            assert a == b, (c, k)


def test_eval_large_case_shapes():
    """The case past ev_map_rows_kernel's launch cap and the three-pass case."""
    from tests import eval_cases as EC
    m, (users, items, keys) = EC.case("past_cap")
    assert users.size == EC.N_PAST_CAP == 16384 * 256 + 257
    who = np.unique(users)
    assert np.isin(who, m[0]).sum() == 36 and (~np.isin(who, m[0])).sum() == 3
    m, (users, items, keys) = EC.case("passes")
    lm, (lu, li, lk) = EC.case("lengths", "random")
    known = np.intersect1d(np.unique(users), m[0])
    assert known.size == EC.PASS_USERS + 12 > 2 * EC.PASS_ROWS and np.isin(lm[0][:12], known).all()
    at = np.searchsorted(known, np.sort(lm[0][:12])) // EC.PASS_ROWS  # the pass of each user of lengths
    assert at.tolist() == [0] * 6 + [1] * 6 and (known.size - 1) // EC.PASS_ROWS == 2
    for u in lm[0][:12]:
        assert np.array_equal(np.sort(keys[users == u]), np.sort(lk[lu == u]))


# ---- the front-end edge cases (tests/spectrum_cases.py) -------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 16, 17, 50, 63, 64, 65, 127, 128, 129, 200, 255, 256])
def test_spectrum_case_properties(k):
    """Every matrix of tests/spectrum_cases.py has the property its name claims (rank, multiplicities,
    cluster width, exact zeros), by LAPACK alone."""
    from tests import spectrum_cases as SC
    assert SC.spectrum_kinds(k) == [s for s in SC.SPECTRA if k >= SC.MIN_K[s]] and "identity" in SC.spectrum_kinds(k)
    if k >= 4:
        assert SC.spectrum_kinds(k) == list(SC.SPECTRA)
    for kind in SC.spectrum_kinds(k):
        G = SC.spectrum(kind, k)
        assert G.shape == (k, k) and G.dtype == np.float64 and np.isfinite(G).all(), kind
        assert np.array_equal(G, G.T), kind  # exactly symmetric: the kernels read one triangle
        w = np.linalg.eigvalsh(G)
        wmax = max(float(np.abs(w).max()), 1e-300)
        d = np.diag(G)
        if kind == "identity":
            assert np.array_equal(G, SC.IDENTITY_C * np.eye(k))
        elif kind == "zero":
            assert not G.any()
        elif kind == "diag":
            assert np.array_equal(G, np.diag(d)) and np.unique(d).size == k and d.min() > 0
            assert k == 1 or d.max() / d.min() == pytest.approx(100.0)
            assert k < 5 or (np.any(np.diff(d) < 0) and np.any(np.diff(d) > 0))  # in no order
        elif kind == "allones":
            assert np.all(G == 1.0) and np.linalg.matrix_rank(G) == 1 and w[-1] == pytest.approx(k)
        elif kind == "rank1":
            assert np.linalg.matrix_rank(G) == 1 and np.all(G != 0)
        elif kind == "deficient":
            r = SC.deficient_rows(k)
            assert r == max(1, k // 10) < k and np.linalg.matrix_rank(G) == r
            assert np.abs(w[:k - r]).max() < 1e-13 * wmax and w[k - r] > 1e-3 * wmax
        elif kind == "pairs":
            want = SC.pairs_eigenvalues(k)
            assert np.abs(w - want).max() < 1e-12 * wmax and want[-1] / want[0] == pytest.approx(1e3)
            assert np.all(want[0:2 * (k // 2):2] == want[1:2 * (k // 2):2])  # every value twice
            assert k < 6 or np.min(np.diff(np.unique(want))) > 1e-3  # and the pairs well apart
        elif kind == "twoclusters":
            lo, hi = w[:k // 2], w[k // 2:]
            assert np.abs(lo - 1.0).max() < 1e-12 and np.abs(hi - 2.0).max() < 1e-12
            assert SC.CLUSTER_WIDTH == 1e-15 and np.ptp(lo) < 1e-12 and np.ptp(hi) < 1e-12
        elif kind == "graded":
            assert np.log10(d.max() / d.min()) > 15 and np.argmin(d) < np.argmax(d)
            assert w[-1] / max(abs(w[0]), 1e-300) > 1e14  # 16 decades; the small end is at LAPACK's rounding
        elif kind == "zerocols":
            z = np.arange(k) % 3 == 0
            assert not G[z].any() and not G[:, z].any() and np.all(d[~z] > 0)
            assert np.linalg.matrix_rank(G) == int((~z).sum())
        elif kind == "sparkinit":
            c = SC.SPARKINIT_ROWS / k
            assert np.trace(G) == pytest.approx(SC.SPARKINIT_ROWS, rel=1e-5)
            assert 0.5 * c < w[0] and w[-1] < 1.6 * c
    if k >= 4:
        G = SC.spectrum("pairs", k)
        ws = SC.warm_starts(G)
        assert list(ws) == list(SC.WARM_STARTS)
        V = ws["exact"]
        assert np.abs(V.T @ V - np.eye(k)).max() < 1e-13
        assert sorted(map(tuple, np.round(ws["permuted"].T, 9))) == sorted(map(tuple, np.round(V.T, 9)))
        assert k < 16 or not np.allclose(ws["permuted"], V)
        assert np.sum(np.any(ws["reflected"] != V, axis=0)) == 1
        assert np.linalg.det(V) * np.linalg.det(ws["reflected"]) == pytest.approx(-1.0)
        e = np.abs(ws["noisy"].T @ ws["noisy"] - np.eye(k)).max()
        assert 1e-9 < e < 1e-6  # not orthogonal, by about the noise


@pytest.mark.parametrize("k", [3, 17, 50, 65])
def test_jacobi_restatement_converges_on_every_spectrum(k):
    """tools/jacobi_ref.py (the numpy restatement of eig.hip's Jacobi) meets the stopping rule within
    JAC_MAX_SWEEPS on every spectrum, and what it returns meets the residual bound the GPU test asks of
    the device.  (k = 127 .. 256: SC.REF_SWEEPS, produced once, all within the budget; the restatement
    takes up to 10 s per matrix there.)"""
    from tests import spectrum_cases as SC
    from tools import jacobi_ref as JR
    for kind in SC.spectrum_kinds(k):
        G = SC.spectrum(kind, k)
        w, VT, sweeps = SC.ref_sweeps(G)
        assert sweeps is not None and sweeps <= JR.JAC_MAX_SWEEPS, kind
        assert np.linalg.norm(VT @ G @ VT.T - np.diag(w)) <= 1e-12 * np.linalg.norm(G), kind
        assert np.abs(VT @ VT.T - np.eye(k)).max() < 1e-12, kind
        if kind in ("identity", "zero", "diag"):
            assert sweeps == 0 and np.array_equal(w, np.diag(G))
    assert set(SC.REF_SWEEPS) == {(kind, kk) for kk in SC.EIG_KS if kk > 65 for kind in SC.SPECTRA}
    assert all(0 <= s <= JR.JAC_MAX_SWEEPS for s in SC.REF_SWEEPS.values())
    assert max(SC.REF_SWEEPS.values()) == SC.REF_SWEEPS["twoclusters", 256] == 22  # 8 under the budget


def test_reference_sweep_table_is_the_restatement():
    """SC.REF_SWEEPS against a fresh run of the restatement at k = 127 on the two cheapest kinds with a
    count above 1 (one sweep either side: the count depends on the last bits of the BLAS products)."""
    from tests import spectrum_cases as SC
    for kind in ("graded", "twoclusters"):
        assert abs(SC.ref_sweeps(SC.spectrum(kind, 127))[2] - SC.REF_SWEEPS[kind, 127]) <= 1, kind


@pytest.mark.parametrize("kind,k", [("graded", 65), ("twoclusters", 17), ("twoclusters", 50), ("twoclusters", 65)])
def test_spectra_expose_a_jacobi_that_stops_early(kind, k):
    """Mutation: a Jacobi stopped at off-diagonal mass 1e-18 of the diagonal's instead of 1e-28 misses
    the residual bound of the GPU test (‖VᵀGV - diag(w)‖_F < 1e-12 ‖G‖_F) by more than two decades on
    these inputs, while the real rule meets it.  (`graded` at k = 17 and 50 does not tell the two apart:
    its last sweep takes the mass from above 1e-18 straight to rounding, so both rules stop there.)"""
    from tests import spectrum_cases as SC
    G = SC.spectrum(kind, k)
    gn = np.linalg.norm(G)
    w, VT, s = SC.ref_sweeps(G)
    assert np.linalg.norm(VT @ G @ VT.T - np.diag(w)) < 1e-12 * gn
    w, VT, s_early = SC.ref_sweeps(G, tol=1e-18)
    assert s_early < s
    assert np.linalg.norm(VT @ G @ VT.T - np.diag(w)) > 1e-10 * gn


def _fp32_vs_fp64(Y, ptr, col, val, reg, alpha):
    from tests import ladder as LD
    from tests import spectrum_cases as SC
    x64 = SC.row_solutions(Y, ptr, col, val, reg, alpha)
    x32 = SC.row_solutions(Y, ptr, col, val, reg, alpha, np.float32)
    ref = O.half_sweep(Y, ptr, col, val, reg=reg, alpha=alpha)
    assert LD.row_errors(x64, ref).max() < 1e-6  # the helper restates the oracle
    return float(LD.row_errors(x32, x64).max()), ref


FP32_PRECONDITION = 2e-5  # a fifth of the half-sweep tolerance, the project's own worst on trained factors


@pytest.mark.parametrize("family", ["rows-64", "rows-100", "rows-256", "degenerate-50", "degenerate-128",
                                    "degenerate-200", "zero", "reg0"])
def test_front_end_half_sweep_inputs_are_well_conditioned(family):
    """A condition on the inputs of tests/test_gpu_gram_eig_edges.py, not a measurement: every row
    system of every half (built in fp64 as oracle.spark_als.normal_equation builds it, the chain of
    halves continued from the oracle's own factors) solved by a plain fp32 Cholesky stays within 2e-5 of
    the fp64 solve in the metric of ladder.row_errors, so a miss of 1e-4 on the device is the device's.
    The case generators also deliver what they promise: every source id kept, the degrees asked for."""
    from tests import spectrum_cases as SC
    worst = 0.0

    def chain(n, k, kind, halves, F=None, reg=SC.REG):
        nonlocal worst
        B = SC.blocks(n)
        src = SC.factors(n, k, kind) if F is None else F
        assert len(B.user_ids) == n and src.shape == (n, k) and src.dtype == np.float32
        for h in range(halves):
            ptr, col, val = (B.i_ptr, B.i_col, B.i_val) if h % 2 == 0 else (B.u_ptr, B.u_col, B.u_val)
            err, ref = _fp32_vs_fp64(src, ptr, col, val, reg, SC.ALPHA)
            assert err <= FP32_PRECONDITION, (n, k, kind, h, err)
            assert SC.rhs_cancellation(src, ptr, col, val) * 2.0 ** -24 <= FP32_PRECONDITION, (n, k, kind, h)
            worst = max(worst, err)
            src = ref

    name, _, arg = family.partition("-")
    if name == "rows":
        for c in SC.ROW_COUNT_CASES:
            if c[1] == int(arg):
                chain(c[0], c[1], c[2], 1)
    elif name == "degenerate":
        for c in SC.DEGENERATE_CASES:
            if c[1] == int(arg) and c[3] == -1:
                chain(c[0], c[1], c[2], 4)
    elif name == "zero":
        for c in SC.ZERO_CASES:
            if c[3] == -1:
                chain(c[0], c[1], c[2], 2)
    else:
        for k in SC.REG0_RANKS:
            for variant in ("full", "tiny"):
                chain(4 * k, k, "unit", 1, F=SC.reg0_factors(k, variant), reg=0.0)
    print(f"FP32_PRECONDITION {family}: worst {worst:.2e}")


def test_front_end_case_generators():
    """What tests/spectrum_cases.py promises about its factor matrices and rating sets."""
    from tests import ladder as LD
    from tests import spectrum_cases as SC
    assert SC.ROW_COUNTS == (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025)
    assert [LD.padded_rank(k) for k in SC.ROW_COUNT_RANKS] == [64, 128, 256]  # one per Gram kernel
    assert len(SC.ROW_COUNT_CASES) == 42 and len(SC.DEGENERATE_CASES) == 42 and len(SC.LADDER_CASES) == 13
    for n in SC.ROW_COUNTS + SC.DEFICIENT_ROWS + (SC.SAME_ROWS, SC.ZEROCOLS_ROWS, 200, 512):
        user, item, r = SC.coo(n, SC.DEGREES)
        B = SC.blocks(n)
        assert len(B.user_ids) == n == np.unique(user).size  # every source id rated at least once
        assert set(np.unique(r).tolist()) <= set(SC.RATINGS) and np.all(r > 0)
        deg = np.diff(B.i_ptr)
        want = sorted(min(n, d) for d in SC.DEGREES)
        got = sorted(deg.tolist())
        for d in want:  # one row of each asked degree (the cover rows add more)
            assert d in got, (n, d)
            got.remove(d)
        assert all(1 <= d <= SC.COVER_DEGREE for d in got)
        assert np.unique(user.astype(np.int64) << 32 | (item.astype(np.int64) & 0xFFFFFFFF)).size == user.size
        assert n < 3 or np.any(np.diff(user.astype(np.int64)) < 0)  # shuffled
    for k in SC.DEGENERATE_RANKS:
        for n, kind in SC.degenerate_cases(k):
            F = SC.factors(n, k, kind)
            G = O.gram(F)
            if kind == "unit":
                assert n < k and np.linalg.matrix_rank(G) == n
                assert np.allclose(np.linalg.norm(F.astype(np.float64), axis=1), 1.0, atol=1e-6)
            elif kind == "same":
                assert n == SC.SAME_ROWS and np.all(F == F[0]) and np.linalg.matrix_rank(G) == 1
            elif kind == "zerocols":
                z = np.arange(k) % 3 == 0
                assert not F[:, z].any() and np.all(np.abs(F[:, ~z]).max(axis=0) > 0)
            elif kind == "ortho":
                assert n == SC.ortho_rows(k) and n % k == 0 and abs(n - 512) <= k // 2
                c = 0.25 * n / k
                assert np.abs(G - c * np.eye(k)).max() < 1e-6 * c
        assert not SC.factors(64, k if k != 200 else 50, "zero").any()
    for k in SC.REG0_RANKS:
        w = np.linalg.eigvalsh(O.gram(SC.reg0_factors(k, "full")))
        assert w[0] > 1e-2 * w[-1]  # far above the switch at 1e-12
        F = SC.reg0_factors(k, "tiny")
        w = np.linalg.eigvalsh(O.gram(F))
        assert 0 < w[0] < 1e-12 * w[-1] and w[1] > 1e-2 * w[-1] and np.all(F[:, 1] != 0)
        F = SC.reg0_factors(k, "zerocol")
        assert not F[:, 1].any() and np.linalg.matrix_rank(O.gram(F)) == k - 1


@pytest.mark.parametrize("k", [1, 2, 3, 10, 63, 65, 127, 129, 255])
def test_rank_ladder_inputs_are_well_conditioned(k):
    """The same fp32 condition on the rank ladder of the GPU file (ladder_coo, mode `varying`): the item
    half at every rank, the user half (from the oracle's item factors) at ranks up to 65.  The user half
    at ranks 127, 129 and 255 measures 2.2e-5, 2.3e-5 and 5.1e-5 in plain fp32: its source side is the 52
    item rows, rank-deficient above rank 52, and the ladder's data is not this file's to make smaller, so
    those three halves are held to 1e-4 on the device without this condition."""
    from tests import ladder as LD
    from tests import spectrum_cases as SC
    implicit, alpha, reg = LD.MODES["varying"]
    user, item, ideg = LD.ladder_coo()
    B = O.make_blocks(user, item, LD.ladder_ratings("varying", user, ideg))
    F = SC.rank_ladder_factors(k, len(B.user_ids))
    if k != 1:
        assert np.array_equal(F, LD.unit_rows(np.random.default_rng(k), len(B.user_ids), k))
    err, V = _fp32_vs_fp64(F, B.i_ptr, B.i_col, B.i_val, reg, alpha)
    assert err <= FP32_PRECONDITION, err
    if k <= 65:
        err, _ = _fp32_vs_fp64(V, B.u_ptr, B.u_col, B.u_val, reg, alpha)
        assert err <= FP32_PRECONDITION, err
    # b = Σ (1 + c) y itself, summed in fp32, is good to 2^-24 times its cancellation
    for Y, ptr, col, val in ((F, B.i_ptr, B.i_col, B.i_val), (V, B.u_ptr, B.u_col, B.u_val)):
        assert SC.rhs_cancellation(Y, ptr, col, val, alpha) * 2.0 ** -24 <= FP32_PRECONDITION
    if k == 1:  # what the seed of rank 1 avoids: the rank's own seed leaves one user row cancelling 3551-fold
        F1 = LD.unit_rows(np.random.default_rng(1), len(B.user_ids), 1)
        V1 = O.half_sweep(F1, B.i_ptr, B.i_col, B.i_val, reg=reg, alpha=alpha)
        assert SC.rhs_cancellation(V1, B.u_ptr, B.u_col, B.u_val, alpha) > 3000


@pytest.mark.parametrize("k", [64, 100, 256])
def test_row_count_cases_expose_a_gram_that_drops_the_last_row(k):
    """Mutation: a Gram without the last source row (a tail the kernel never reaches) is more than 1e-6
    of max|G| away from the true one at every row count of the GPU test, so the Gram check sees it."""
    from tests import spectrum_cases as SC
    for n in SC.ROW_COUNTS:
        F = SC.factors(n, k, "unit")
        G = O.gram(F)
        miss = np.abs(O.gram(F[:-1]) - G).max() / np.abs(G).max()
        assert miss > 1e-6, (n, miss)


# ---- the NNLS edge cases (tests/nnls_cases.py) ----------------------------------------------------

def test_nnls_path_restatement_against_the_table_of_limits():
    """nnls_cases.nnls_path_of against the lockstep limits YBUDGET / (slots * KP) capped by the light limit
    (KP 64: 24 | 32; KP 128: 12 | 24, then 48 | 64 behind ALBEDO_NNLS_MIN_SLOTS; KP 256: 6 | 12, then
    24 | 48 | 64), the per-row labels and their split forms."""
    from tests import nnls_cases as NC
    table = {(64, 8): [(16, 24), (8, 32)], (64, 1): [(16, 24), (8, 32)],
             (128, 8): [(16, 12), (8, 24)], (128, 4): [(16, 12), (8, 24), (4, 48)],
             (128, 1): [(16, 12), (8, 24), (4, 48), (2, 64)],
             (256, 16): [(16, 6)], (256, 8): [(16, 6), (8, 12)], (256, 4): [(16, 6), (8, 12), (4, 24)],
             (256, 2): [(16, 6), (8, 12), (4, 24), (2, 48)], (256, 1): [(16, 6), (8, 12), (4, 24), (2, 48), (1, 64)]}
    for (KP, ms), rows in table.items():
        assert [(sv, hi) for sv, (_, hi) in NC.variant_ranges(KP, ms).items()] == rows, (KP, ms)
        lo = 1
        for sv, hi in rows:
            for d in (lo, hi):
                assert NC.nnls_path_of(d, KP, 8192, ms) == f"lockstep-{sv}", (KP, ms, d)
            lo = hi + 1
        assert NC.nnls_path_of(lo, KP, 8192, ms) == f"row-{KP}"
        assert NC.nnls_path_of(256, KP, 256, ms) == f"row-{KP}" and NC.nnls_path_of(257, KP, 256, ms) == f"row-{KP}-split"
        assert NC.nnls_path_of(9000, KP, 0, ms) == f"row-{KP}"
    assert NC.batch_limits(256, 3) == NC.batch_limits(256, 8)  # an invalid knob value is the default
    assert NC.nnls_path_of(65, 256, 256, 8, "1024") == "row-256-1024" and NC.nnls_path_of(513, 256, 256, 8, "1024") == "row-256-1024-split"
    assert NC.nnls_path_of(65, 128, 256, 8, "1024") == "row-128"
    assert NC.path_stats([3, 30, 300], ["lockstep-16", "row-64", "row-64-split"]) == [1, 3, 2, 330]


def test_nnls_ladder_reaches_every_expected_path():
    """The NNLS ladder holds every degree twice; under every configuration of tests/test_gpu_nnls_edges.py
    each expected label holds at least 2 rows, and every lockstep variant that can hold a row has at least
    2 rows at its limit and 2 one above it, on another path."""
    from tests import ladder as LD
    from tests import nnls_cases as NC
    user, item, r, B = NC.ladder_data("varying")
    assert np.unique(user.astype(np.int64) << 32 | item).size == user.size and np.any(np.diff(user) < 0)
    deg_i, deg_u = np.diff(B.i_ptr), np.diff(B.u_ptr)
    assert sorted(deg_i.tolist()) == sorted(NC.NNLS_LADDER + NC.NNLS_LADDER)
    assert 650 <= len(B.user_ids) <= 700 and 6 < deg_u.max() <= 12
    for k in (50, 100, 128, 256):
        KP = LD.padded_rank(k)
        for chunk in (8192, 256):
            for ms in (8, 4, 1):
                for rk in (None, "1024"):
                    paths = np.array([NC.nnls_path_of(d, KP, chunk, ms, rk) for d in deg_i])
                    want = NC.expected_nnls_paths(KP, chunk, ms, int(deg_i.max()), rk)
                    assert set(paths.tolist()) == set(want), (k, chunk, ms, rk)
                    assert all(np.sum(paths == p) >= 2 for p in want), (k, chunk, ms)
                    for sv, (at, above) in NC.boundary_rows(deg_i, paths, KP, ms).items():
                        assert at >= 2 and above >= 2, (k, ms, sv)
        upaths = np.array([NC.nnls_path_of(d, KP, 8192) for d in deg_u])
        assert set(upaths.tolist()) == set(NC.expected_nnls_paths(KP, 8192, 8, int(deg_u.max())))
        assert all(np.sum(upaths == p) >= 2 for p in set(upaths.tolist()))
    assert set(NC.variant_ranges(256, 1)) == {16, 8, 4, 2, 1} and set(NC.variant_ranges(128, 1)) == {16, 8, 4, 2}
    for mode in LD.MODES:
        Bm = NC.ladder_data(mode)[3]
        if mode == "mixed":
            assert np.sum(np.add.reduceat(Bm.i_val > 0, Bm.i_ptr[:-1]) == 0) >= 4
    # the row-count cases: every row on the one variant they name
    from tests.test_gpu_nnls_edges import ROW_COUNT_CASES
    assert {sv for _, sv, *_ in ROW_COUNT_CASES} == {16, 8, 1}
    for k, sv, ms, d, n, _ in ROW_COUNT_CASES:
        u, i = NC.uniform_degree_coo(n, d)
        Bn = O.make_blocks(u, i, np.ones(u.size, np.float32))
        assert np.diff(Bn.i_ptr).tolist() == [d] * n and n >= 1
        assert NC.nnls_path_of(d, LD.padded_rank(k), 8192, ms or 8) == f"lockstep-{sv}"


@pytest.mark.parametrize("k", [50, 128, 256])
def test_nnls_scale_cases_are_decided_by_the_absolute_step_threshold(k):
    """Src rows of norm 2^10: the first step (g·res) / (g·A·g) at x = 0 of every row is below 1e-7 / 8, so
    Spark stops at once and returns exactly 0 after 0 iterations; at 2^-10 every row iterates and none is
    zero.  The same rows at unit norm iterate too."""
    from tests import nnls_cases as NC
    big = NC.item_reference("varying", k, "large")
    steps = []
    for j in range(len(big.it)):
        A, b, n = O.normal_equation(big.src, big.ptr, big.col, big.val, j, True, big.alpha, big.G)
        A = A + big.reg * n * np.eye(k)
        res = -b
        g = np.where(res > 0, 0.0, res)
        steps.append(float(g @ res) / (float(g @ A @ g) + 1e-20))
    assert 0 < min(steps) and max(steps) < 1e-7 / 8, (min(steps), max(steps))
    assert not big.X.any() and not big.it.any()
    small = NC.item_reference("varying", k, "small")
    assert small.it.min() >= 1 and small.X.any(axis=1).all()
    assert np.allclose(np.linalg.norm(small.src, axis=1), 2.0 ** -10, rtol=1e-6)
    assert np.allclose(np.linalg.norm(big.src, axis=1), 2.0 ** 10, rtol=1e-6)


def test_nnls_oracle_iteration_windows():
    """On every input of the NNLS edge suite the oracle stops by Spark's rule well before the cap
    max(400, 20 k) (below half of it), so both sides stop at a defined point; regParam = 0 at rank 128 / 256
    and regParam 1e-3 with alpha 200 at rank 128 have at least 20 rows past 128 iterations (two residual
    refreshes of the per-row kernels); all-negative src factors give 0 iterations, all-positive ones no
    zero row and at least 4 rows without a zero."""
    from tests import nnls_cases as NC
    many = {("reg0", 128), ("reg0", 256), ("stiff", 128)}
    for name, (_, _, _, ranks) in NC.PARAM_CASES.items():
        for k in ranks:
            ref = NC.item_reference("varying", k, "nonneg", name)
            assert ref.it.max() < NC.iteration_cap(k) // 2, (name, k, int(ref.it.max()))
            if (name, k) in many:
                assert np.sum(ref.it > 128) >= 20, (name, k)
    for kind in ("nonneg", "aniso", "pos"):
        for k in (50, 128, 256):
            ref = NC.item_reference("varying", k, kind)
            assert 1 <= ref.it.min() and ref.it.max() < NC.iteration_cap(k) // 2, (kind, k)
            if kind == "pos":
                assert ref.X.any(axis=1).all() and np.sum((ref.X > 0).all(axis=1)) >= 4  # interior rows
            if kind == "aniso":
                d = np.diag(ref.G)
                assert d.max() / d.min() > 3e3  # G spans about four decades
    for k in (50, 256):
        ref = NC.item_reference("varying", k, "neg")
        assert not ref.X.any() and not ref.it.any() and (ref.src < 0).all()
    for k in (1, 2):
        assert (NC.src_factors("nonneg", 20, k) > 0).all()
    assert (NC.src_factors("nonneg", 20, 3)[:, 2] < 0).all()


def test_nnls_check_rows_rejects_what_the_whole_matrix_checks_accept(tmp_path):
    """The per-row check of the NNLS edge suite on CPU-side mutations of a correct result: a low-norm row
    scaled by 1.01, an exactly-zero row set to 1e-6, k // 64 + 2 zeros of a row flipped.  The whole-matrix
    checks (relative error against the largest entry of the matrix < 1e-3, equal zero pattern on > 99.5 %
    of the entries) accept all three; check_rows names each with its criterion."""
    from tests import ladder as LD
    from tests import nnls_cases as NC
    k = 50
    user, item, r, B = NC.ladder_data("mixed")
    r = np.where(item == B.item_ids[np.diff(B.i_ptr) == 5][0], np.float32(2.0 ** -8), r)  # one low-confidence row
    B = O.make_blocks(user, item, r)
    ref = NC.reference(NC.src_factors("nonneg", len(B.user_ids), k), B.i_ptr, B.i_col, B.i_val, reg=0.5, alpha=10.0, implicit=True)
    deg = np.diff(B.i_ptr)
    paths = np.array([NC.nnls_path_of(d, 64, 8192) for d in deg])
    margin = 16.0

    def whole_matrix_accepts(X):  # as part of a half of 5 x 52 rows, the others correct
        err = np.max(np.abs(X.astype(np.float64) - ref.X)) / np.max(np.abs(ref.X))
        same = (np.sum((X == 0) == (ref.X == 0)) + 4 * X.size) / (5 * X.size)
        return err < 1e-3 and same > 0.995 and np.all(X >= 0)

    stats = NC.check_rows(ref.X, ref, B.item_ids, deg, paths, "clean", tmp_path, margin)
    assert set(stats) == set(paths.tolist()) and all(s["err"] == 0 and s["flips"] == 0 for s in stats.values())
    norms = np.abs(ref.X).max(axis=1)
    zero = np.nonzero(norms == 0)[0]
    assert zero.size >= 4
    low = int(np.argmin(np.where(norms > 0, norms, np.inf)))
    assert deg[low] == 5 and norms[low] < 0.08 * norms.max()
    # a low-norm row off by 1 % in every digit
    X = ref.X.copy()
    X[low] *= np.float32(1.01)
    assert whole_matrix_accepts(X)
    with pytest.raises(AssertionError) as e:
        NC.check_rows(X, ref, B.item_ids, deg, paths, "scaled row", tmp_path, margin)
    msg = str(e.value)
    assert "1 of 52 rows" in msg and f"id {B.item_ids[low]} degree {deg[low]} path {paths[low]} fails" in msg and "d:distance" in msg
    saved = np.load(msg.rsplit("saved to ", 1)[1].strip())
    assert saved["ids"].tolist() == [B.item_ids[low]] and np.array_equal(saved["got"][0], X[low])
    # an exactly-zero row at 1e-6
    X = ref.X.copy()
    X[zero[0]] = 1e-6
    assert whole_matrix_accepts(X)
    with pytest.raises(AssertionError, match=f"id {B.item_ids[zero[0]]} degree {deg[zero[0]]} ") as e:
        NC.check_rows(X, ref, B.item_ids, deg, paths, "zero row", tmp_path, margin)
    assert "b:zero row" in str(e.value)
    # k // 64 + 2 zeros of one row flipped (to a value the distance criterion cannot see)
    row = int(np.argmax((ref.X == 0).sum(axis=1) * (norms > 0)))
    at = np.nonzero(ref.X[row] == 0)[0][:k // 64 + 2]
    assert at.size == k // 64 + 2
    X = ref.X.copy()
    X[row, at] = np.float32(1e-7 * norms[row])
    assert whole_matrix_accepts(X) and LD.row_errors(X, ref.X).max() < 1e-6
    with pytest.raises(AssertionError, match=f"id {B.item_ids[row]} degree {deg[row]} ") as e:
        NC.check_rows(X, ref, B.item_ids, deg, paths, "flipped zeros", tmp_path, margin)
    assert "e:zero pattern" in str(e.value)
    # negative and non-finite entries, and a KKT residual the distance does not show
    X = ref.X.copy()
    X[low, 0] = -1e-9
    with pytest.raises(AssertionError, match="a:sign/finite"):
        NC.check_rows(X, ref, B.item_ids, deg, paths, "negative", tmp_path, margin)
    X[low, 0] = np.nan
    with pytest.raises(AssertionError, match="a:sign/finite"):
        NC.check_rows(X, ref, B.item_ids, deg, paths, "nan", tmp_path, margin)
    X = ref.X.copy()
    X[low] *= np.float32(1.0005)  # inside the 1e-3 distance, 5e-4 |b| off the optimum
    with pytest.raises(AssertionError) as e:
        NC.check_rows(X, ref, B.item_ids, deg, paths, "kkt", tmp_path, margin)
    assert "c:kkt" in str(e.value) and "d:distance" not in str(e.value)
    # the iteration parity: a path that takes 20 % more iterations than the oracle
    lock, rest = NC.iteration_sums(ref.it, paths)
    assert lock > 100 and rest > 100
    assert NC.check_iterations([lock + rest, int(ref.it.max()), 52, lock], ref, paths, k, "clean") == [1.0, 1.0]
    with pytest.raises(AssertionError, match="lockstep iterations"):
        NC.check_iterations([int(1.2 * lock) + rest, int(ref.it.max()), 52, int(1.2 * lock)], ref, paths, k, "slow")
    with pytest.raises(AssertionError, match="iteration cap"):
        NC.check_iterations([lock + rest, NC.iteration_cap(k), 52, lock], ref, paths, k, "cap")
    with pytest.raises(AssertionError):
        NC.check_iterations([lock + rest, int(ref.it.max()), 51, lock], ref, paths, k, "rows")


def test_nnls_fit_reference_is_the_numpy_fit():
    """nnls_cases.fit_reference (the C restatement of NNLS.solve, half-sweep by half-sweep) is O.fit with
    nonnegative = true; pinned at rank 16, where the numpy loop takes a second (at rank 128 it takes 30 s,
    which is why the GPU fit test uses the C restatement)."""
    from tests import nnls_cases as NC
    user, item, r, B = NC.ladder_data("varying")
    U0 = NC.src_factors("nonneg", len(B.user_ids), 16)
    V0 = NC.src_factors("nonneg", len(B.item_ids), 16, seed=77)
    U, V = O.fit(B, rank=16, max_iter=2, reg=0.5, alpha=10.0, implicit=True, nonnegative=True, init_user=U0, init_item=V0)
    Uc, Vc = NC.fit_reference(B, U0, max_iter=2, reg=0.5, alpha=10.0, implicit=True)
    assert np.max(np.abs(U - Uc)) <= 1e-6 * np.max(np.abs(U)) and np.max(np.abs(V - Vc)) <= 1e-6 * np.max(np.abs(V))
    assert np.array_equal(U == 0, Uc == 0) and np.array_equal(V == 0, Vc == 0)

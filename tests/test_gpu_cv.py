"""CrossValidator on the device (albedo_amd/tuning.py, albedo_amd/cv.py): 300 users x 120 items, about
6,000 synthetic stars with distinct timestamps, 2 folds, grid rank {4, 6} x regParam {0.1, 0.5},
maxIter 3.

The yardstick of every (fold, map) is a standalone ALS.fit on the fold's training rows, whose factors
go through the oracle route of tests/cv_cases.py: O.f2j_sdot on the held-out pairs, unknown ids
dropped, O.into_user_items at the formatter's top-15 cut to k = 30, O.into_user_items of the WHOLE
dataset for the actual lists, O.ndcg_at per user.  Per-user values are compared bit for bit; the
average is Spark's arithmetic (the fold metrics summed in fold order, scaled by 1.0 / numFolds)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import spark_als as O
from tests import cv_cases as CC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLDS, TOP_K, K, SEED = 2, 15, 30, 11
BASE = dict(implicitPrefs=True, alpha=10.0, maxIter=3, seed=42, coldStartStrategy="drop", userCol="user_id",
            itemCol="repo_id", ratingCol="starring")


def _stars():
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(300, 120, 6000, seed=21))
    n = d["user"].size
    ts = 1_500_000_000_000_000 + 1000 * np.random.default_rng(22).permutation(n).astype(np.int64)
    return {"user_id": d["user"], "repo_id": d["item"], "starring": d["rating"].astype(np.float64), "starred_at": ts}


def _oracle_fold(model, val_users, val_items, actual):
    """(users, per-user NDCG@K) of one fitted model on one fold's held-out pairs, by the oracle route."""
    uid, uf = model.user_factors_np()
    iid, itf = model.item_factors_np()
    known = np.isin(val_users, uid) & np.isin(val_items, iid)
    u, it = val_users[known], val_items[known]
    sc = O.f2j_sdot(uf[np.searchsorted(uid, u)], itf[np.searchsorted(iid, it)])
    live = ~np.isnan(sc)
    lists = O.into_user_items(u[live], it[live], sc[live], TOP_K)
    users = np.array(sorted(set(lists) & set(actual)), np.int32)
    vals = np.array([O.ndcg_at([(lists[int(x)][:K], actual[int(x)][:K])], K) for x in users], np.float64)
    return users, vals


def test_cross_validator_matches_standalone_fits(gpu_lib):
    from albedo_amd import ALS
    from albedo_amd.tuning import CrossValidator, DeviceRankingEvaluator, ParamGridBuilder, k_fold
    stars = _stars()
    assert 5000 < stars["user_id"].size < 7000 and np.unique(stars["starred_at"]).size == stars["user_id"].size
    data = {c: stars[c] for c in ("user_id", "repo_id", "starring")}
    grid = ParamGridBuilder().addGrid("rank", [4, 6]).addGrid("regParam", [0.1, 0.5]).build()
    ev = DeviceRankingEvaluator(stars["user_id"], stars["repo_id"], stars["starred_at"], metricName="NDCG@k", k=K,
                                formatterTopK=TOP_K, keepPerUser=True)
    cvm = CrossValidator(estimator=ALS(**BASE), estimatorParamMaps=grid, evaluator=ev, numFolds=FOLDS, seed=SEED).fit(data)

    actual = O.into_user_items(stars["user_id"], stars["repo_id"], stars["starred_at"], K)
    fold = k_fold(stars["user_id"].size, FOLDS, SEED)
    want = np.zeros(len(grid))
    for f in range(FOLDS):
        train = {c: v[fold != f] for c, v in data.items()}
        vu, vi = data["user_id"][fold == f], data["repo_id"][fold == f]
        for i, pm in enumerate(grid):
            model = ALS(**BASE).fit(train, pm)
            users, vals = _oracle_fold(model, vu, vi, actual)
            mean, gu, gv = ev.per_user[f * len(grid) + i]
            assert np.array_equal(gu, users), f"fold {f} map {pm}: evaluated users differ"
            assert np.array_equal(gv, vals), f"fold {f} map {pm}: per-user values differ"
            assert mean == CC.sequential_mean(vals) == cvm.foldMetrics[f][i]
            assert users.size > 100 and 0 < np.mean(vals > 0)
            want[i] += mean
    want *= 1.0 / FOLDS
    assert cvm.avgMetrics == want.tolist()
    assert cvm.bestIndex == int(np.argmax(want))
    full = ALS(**BASE).fit(data, grid[cvm.bestIndex])
    for side in ("user_factors_np", "item_factors_np"):
        (ia, fa), (ib, fb) = getattr(cvm.bestModel, side)(), getattr(full, side)()
        assert np.array_equal(ia, ib) and np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    assert cvm.bestModel.rank == grid[cvm.bestIndex]["rank"]


def test_cv_driver_prints_one_line_per_map(gpu_lib, tmp_path):
    """python -m albedo_amd.cv at the same size, in a fresh child process: one "metric: ParamMap" line
    per map, best first."""
    r = subprocess.run([sys.executable, "-m", "albedo_amd.cv", "--users", "300", "--repos", "120", "--stars", "6000",
                        "--ranks", "4,6", "--reg-params", "0.1,0.5", "--alphas", "10", "--max-iters", "3", "--no-cache"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 4, r.stdout[-2000:]
    metrics = []
    for ln in lines:
        m = re.match(r"^([0-9.eE+-]+): (\{.*\})$", ln)
        assert m, ln
        metrics.append(float(m.group(1)))
        assert "'rank'" in m.group(2) and "'regParam'" in m.group(2) and "'maxIter': 3" in m.group(2)
    assert metrics == sorted(metrics, reverse=True) and 0 < metrics[0] <= 1

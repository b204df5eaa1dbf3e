"""Spark ml.tuning for the ALS mirror: `ParamGridBuilder`, `CrossValidator`, and the device evaluator
of albedo's cross-validation job (ALSRecommenderCV.scala:54-90, albedo_toolkit/evaluators.py:42-67).

Per fold the job fits every ParamMap on the training folds, runs ALSModel.transform on the held-out
pairs (coldStartStrategy "drop"), turns the predictions into per-user lists with
RankingMetricFormatter("als") (rank() over prediction desc <= topK, topK left at its default 15) and
scores them with RankingEvaluator at k against the actual lists of the WHOLE dataset.  Here one
`ALS.fit(train, maps)` shares the fold's ingest between the maps, and `ALSModel.evaluate_pairs` does
the transform, the formatter and the evaluator on the device.
"""
from __future__ import annotations

import itertools

import numpy as np

from . import _lib


class ParamGridBuilder:
    """pyspark.ml.tuning.ParamGridBuilder over param names: `addGrid(name, values)` in call order,
    `build()` -> list of dicts, the cartesian product with the first-added param varying slowest
    (pyspark's itertools.product over the grid in insertion order)."""

    def __init__(self):
        self._grid = {}

    def addGrid(self, param, values):
        self._grid[str(param)] = list(values)
        return self

    def baseOn(self, *pairs, **kw):
        for d in pairs:
            for k, v in dict(d).items():
                self.addGrid(k, [v])
        for k, v in kw.items():
            self.addGrid(k, [v])
        return self

    def build(self):
        names = list(self._grid)
        return [dict(zip(names, vs)) for vs in itertools.product(*(self._grid[n] for n in names))]


def k_fold(n_rows, num_folds, seed):
    """Fold of every row: int32 [n_rows] in [0, num_folds), each row drawn independently and uniformly
    from numpy's PCG64 seeded with `seed`, so every row is in exactly one validation fold and the
    assignment depends on (n_rows, num_folds, seed) alone.

    MLUtils.kFold draws one uniform number per row and cuts [0, 1) into num_folds ranges
    (BernoulliCellSampler), the same law; its membership comes from XORShiftRandom streams seeded per
    partition of the input RDD, so which rows Spark would put in a fold cannot be reproduced without
    Spark and its partitioning of the data."""
    if num_folds < 2:
        raise ValueError("numFolds must be >= 2")
    return np.random.default_rng(seed).integers(0, int(num_folds), int(n_rows)).astype(np.int32)


def _n_rows(dataset):
    return len(dataset) if hasattr(dataset, "iloc") else len(next(iter(dataset.values())))


def _take(dataset, mask):
    if hasattr(dataset, "iloc"):
        return dataset[mask]
    return {k: np.asarray(v)[mask] for k, v in dataset.items()}


class DeviceRankingEvaluator:
    """RankingEvaluator(userActualItemsDF) behind RankingMetricFormatter("als"), on the device:
    `evaluate(model, validation)` = model.evaluate_pairs of the validation pairs against
    intoUserActualItems(actual_users, actual_items, actual_keys desc, k).  `formatterTopK` is the
    formatter's topK (15, which the job never sets); `metricName` one of "NDCG@k", "Precision@k",
    "MAP".  With keepPerUser the (mean, users, values) of every call are appended to `per_user`."""

    def __init__(self, actual_users, actual_items, actual_keys, metricName="NDCG@k", k=30, formatterTopK=15,
                 keepPerUser=False):
        if metricName not in _lib.METRICS:
            raise ValueError(f"unsupported metric {metricName}; supports {', '.join(_lib.METRICS)}")
        self.actual = (np.asarray(actual_users), np.asarray(actual_items), np.asarray(actual_keys))
        self.metricName = metricName
        self.k = int(k)
        self.formatterTopK = int(formatterTopK)
        self.keepPerUser = keepPerUser
        self.per_user = []

    def isLargerBetter(self):
        return True

    def getFormattedMetricName(self):
        return self.metricName.replace("@k", f"@{self.k}")

    def evaluate(self, model, validation):
        from .als import _column
        users = _column(validation, model.getUserCol())
        items = _column(validation, model.getItemCol())
        out = model.evaluate_pairs(users, items, *self.actual, metric=self.metricName, topK=self.formatterTopK,
                                   k=self.k, per_user=self.keepPerUser)
        if self.keepPerUser:
            self.per_user.append(out)
            return out[0]
        return out


class CrossValidatorModel:
    def __init__(self, bestModel, avgMetrics, bestIndex, foldMetrics, estimatorParamMaps):
        self.bestModel = bestModel
        self.avgMetrics = avgMetrics
        self.bestIndex = bestIndex
        self.foldMetrics = foldMetrics  # [numFolds][len(maps)]
        self.estimatorParamMaps = estimatorParamMaps

    def getEstimatorParamMaps(self):
        return self.estimatorParamMaps


class CrossValidator:
    """Spark 2.2 ml.tuning.CrossValidator.fit for the ALS mirror: per fold one shared-ingest
    `estimator.fit(train, maps)` and the evaluator on every model; the metrics are summed in fold
    order and scaled by 1.0 / numFolds (CrossValidator.scala's dscal), the best map (first maximum,
    or minimum when the evaluator says smaller is better) is refitted on the whole dataset.  Folds
    come from `k_fold(len(dataset), numFolds, seed)`."""

    def __init__(self, estimator=None, estimatorParamMaps=None, evaluator=None, numFolds=3, seed=42, parallelism=8):
        self.estimator = estimator
        self.estimatorParamMaps = estimatorParamMaps
        self.evaluator = evaluator
        self.numFolds = int(numFolds)
        self.seed = seed
        self.parallelism = parallelism

    def setEstimator(self, v):
        self.estimator = v
        return self

    def setEstimatorParamMaps(self, v):
        self.estimatorParamMaps = v
        return self

    def setEvaluator(self, v):
        self.evaluator = v
        return self

    def setNumFolds(self, v):
        self.numFolds = int(v)
        return self

    def setSeed(self, v):
        self.seed = v
        return self

    def fit(self, dataset):
        maps = [dict(m) for m in self.estimatorParamMaps]
        if not maps:
            raise ValueError("estimatorParamMaps is empty")
        fold = k_fold(_n_rows(dataset), self.numFolds, self.seed)
        metrics = np.zeros(len(maps), np.float64)
        fold_metrics = []
        for f in range(self.numFolds):
            train, validation = _take(dataset, fold != f), _take(dataset, fold == f)
            models = self.estimator.fit(train, maps, parallelism=self.parallelism)
            row = [float(self.evaluator.evaluate(m, validation)) for m in models]
            del models
            fold_metrics.append(row)
            metrics += np.asarray(row, np.float64)
        metrics *= 1.0 / self.numFolds
        best = int(np.argmax(metrics) if self.evaluator.isLargerBetter() else np.argmin(metrics))
        best_model = self.estimator.fit(dataset, maps[best])
        return CrossValidatorModel(best_model, metrics.tolist(), best, fold_metrics, maps)

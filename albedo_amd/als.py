"""Spark-shaped `ALS` estimator and `ALSModel` over libalbedo_als.so.

Mirrors the surface albedo's jobs use:
  * ALSRecommenderBuilder.scala:46-58 / Playground.scala:54-65 / train_als.py:55-61:
      ALS().setImplicitPrefs(True).setRank(50).setRegParam(0.5).setAlpha(40).setMaxIter(26)
           .setSeed(42).setColdStartStrategy("drop").setUserCol(..).setItemCol(..)
           .setRatingCol(..).fit(dataset)
  * ALSRecommender.scala:16-19,33-36 reads model.userFactors / model.itemFactors / model.rank
  * ALSRecommender.scala:28-65 (+ BoundedPriorityQueue.scala:30-53) is recommendForUserSubset
  * LogisticRegressionRanker.scala:167-174,229 uses model.transform (coldStartStrategy drop)
  * ModelUtils.scala:7-20 persists with model.write.overwrite().save(path) / ALSModel.load(path)
Parameter names, defaults and validation messages follow Spark 2.2.0's ALSParams.  Datasets are
pandas DataFrames or dicts of arrays (there is no JVM here); outputs are pandas DataFrames.
All compute runs on the MI355X through the C ABI; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _lib
from ._lib import IllegalArgumentException, check, load, ptr

SPARK_DEFAULT_SEED = 1994790107  # "org.apache.spark.ml.recommendation.ALS".hashCode (ALS setDefault(seed))


def _column(dataset, name):
    if dataset is None:
        raise IllegalArgumentException(_lib.ALS_E_INVALID_ARGUMENT, "dataset is None")
    try:
        col = dataset[name]
    except (KeyError, IndexError, TypeError):
        raise IllegalArgumentException(_lib.ALS_E_INVALID_ARGUMENT, f"Field \"{name}\" does not exist.") from None
    return np.asarray(col)


def _checked_cast(values, col):
    """ALS.checkedCast: ids must be numeric and within Int range (Spark 2.2.0 error messages)."""
    v = np.asarray(values)
    if v.dtype.kind not in "iuf":
        raise IllegalArgumentException(_lib.ALS_E_INVALID_ARGUMENT,
                                       f"ALS only supports values in Integer range for column {col}. "
                                       f"Column {col} was not numeric.")
    if v.size == 0:
        return v.astype(np.int32)
    if v.dtype.kind == "f":
        bad = (v != np.floor(v)) | (v < -2**31) | (v > 2**31 - 1) | ~np.isfinite(v)
    else:
        bad = (v < -2**31) | (v > 2**31 - 1)
    if np.any(bad):
        x = v[np.argmax(bad)]
        raise IllegalArgumentException(_lib.ALS_E_INVALID_ARGUMENT,
                                       f"ALS only supports values in Integer range and without fractional part "
                                       f"for columns {col}. Value {x} was either out of Integer range or "
                                       f"contained a fractional part that could not be converted.")
    return v.astype(np.int32)


class _Params:
    _defaults = dict(rank=10, maxIter=10, regParam=0.1, numUserBlocks=10, numItemBlocks=10,
                     implicitPrefs=False, alpha=1.0, userCol="user", itemCol="item",
                     ratingCol="rating", predictionCol="prediction", seed=SPARK_DEFAULT_SEED,
                     nonnegative=False, checkpointInterval=10, coldStartStrategy="nan",
                     intermediateStorageLevel="MEMORY_AND_DISK", finalStorageLevel="MEMORY_AND_DISK",
                     device=-1, lightMaxDegree=-1)
    _doc = dict(rank="rank of the factorization", maxIter="max number of iterations (>= 0)",
                regParam="regularization parameter (>= 0)", alpha="alpha for implicit preference",
                implicitPrefs="whether to use implicit preference", nonnegative="whether to use nonnegative constraint for least squares",
                coldStartStrategy="strategy for dealing with unknown or new users/items at prediction time: nan, drop",
                seed="random seed", numUserBlocks="number of user blocks", numItemBlocks="number of item blocks",
                userCol="column name for user ids", itemCol="column name for item ids",
                ratingCol="column name for ratings", predictionCol="prediction column name",
                checkpointInterval="checkpoint interval (kept for API parity; factors stay resident in HBM)",
                intermediateStorageLevel="kept for API parity", finalStorageLevel="kept for API parity",
                device="HIP device ordinal (-1 = current)",
                lightMaxDegree="rows with <= this many ratings use the push-through solve (-1 default, 0 off)")

    _uid_prefix = "als"

    def __init__(self, uid=None, **kw):
        from .persistence import random_uid
        self.uid = uid or random_uid(self._uid_prefix)  # Identifiable.randomUID("als")
        self._p = dict(self._defaults)
        for k, v in kw.items():
            self._set(k, v)

    def _set(self, k, v):
        if k not in self._defaults:
            raise IllegalArgumentException(_lib.ALS_E_INVALID_ARGUMENT, f"unknown param {k}")
        if k == "coldStartStrategy":
            v = str(v).lower()
            if v not in ("nan", "drop"):
                raise IllegalArgumentException(_lib.ALS_E_INVALID_ARGUMENT,
                                               f"als parameter coldStartStrategy given invalid value {v}.")
        if k == "checkpointInterval" and not (v == -1 or v >= 1):
            raise IllegalArgumentException(_lib.ALS_E_INVALID_ARGUMENT,
                                           f"als parameter checkpointInterval given invalid value {v}.")
        self._p[k] = v
        return self

    def explainParams(self) -> str:
        lines = []
        for k in self._defaults:
            cur = self._p[k]
            dft = self._defaults[k]
            extra = f"(default: {dft}" + (f", current: {cur})" if cur != dft else ")")
            lines.append(f"{k}: {self._doc.get(k, '')} {extra}")
        return "\n".join(lines)


def _make_accessors(cls):
    for k in _Params._defaults:
        cap = k[0].upper() + k[1:]
        setattr(cls, "set" + cap, (lambda key: lambda self, v: self._set(key, v))(k))
        setattr(cls, "get" + cap, (lambda key: lambda self: self._p[key])(k))
    return cls


@_make_accessors
class ALS(_Params):
    """Spark ml.recommendation.ALS (estimator)."""

    def _c_params(self, pm=None):
        v = dict(self._p)
        if pm:
            v.update(pm)
        p = _lib.als_params()
        check(load().als_params_default(C.byref(p)))
        p.rank = int(v["rank"])
        p.max_iter = int(v["maxIter"])
        p.implicit_prefs = 1 if v["implicitPrefs"] else 0
        p.nonnegative = 1 if v["nonnegative"] else 0
        p.num_user_blocks = int(v["numUserBlocks"])
        p.num_item_blocks = int(v["numItemBlocks"])
        p.reg_param = float(v["regParam"])
        p.alpha = float(v["alpha"])
        p.seed = int(v["seed"])
        p.device = int(v["device"])
        p.light_max_degree = int(v["lightMaxDegree"])
        return p

    def _context(self, pm=None):
        lib = load()
        p = self._c_params(pm)
        h = C.c_void_p()
        check(lib.als_create(C.byref(p), C.byref(h)))
        return h

    def _param_map(self, pm):
        """Validate a ParamMap (dict of param name -> value) like Params.copy(extra)."""
        probe = ALS(uid=self.uid, **self._p)
        for k, v in pm.items():
            probe._set(k, v)
        return dict(probe._p)

    def _ratings(self, dataset, cols):
        user = _checked_cast(_column(dataset, cols["userCol"]), cols["userCol"])
        item = _checked_cast(_column(dataset, cols["itemCol"]), cols["itemCol"])
        rating = np.ascontiguousarray(_column(dataset, cols["ratingCol"]), dtype=np.float32)
        if user.size == 0:
            raise IllegalArgumentException(_lib.ALS_E_INVALID_ARGUMENT,
                                           "No ratings available from the input dataset.")
        return np.ascontiguousarray(user), np.ascontiguousarray(item), rating

    def _run_fit(self, h, pm, tracked, tol):
        """als_fit, or als_fit_tracked when asked: (seconds, objective history or None, sweeps run or None)."""
        t0 = time.perf_counter()
        hist = ran = None
        if tracked:
            hist, ran = _lib.fit_tracked(h, int(pm["maxIter"]), tol)
        else:
            check(load().als_fit(h))
        return time.perf_counter() - t0, hist, ran

    def fit(self, dataset, params=None, initialUserFactors=None, initialItemFactors=None, parallelism=8,
            trackObjective=False, tol=None):
        """ALS.fit (Spark Estimator.fit(dataset[, paramMap | paramMaps])).

        `params` = one ParamMap (dict) -> one ALSModel fitted with those overrides; a list of ParamMaps
        -> a list of ALSModels (the CV grid of ALSRecommenderCV.scala:67-90) that share ONE ingest
        (id remap, both CSR orientations, shards) on the device: between fits only the
        rank-dependent buffers are rebuilt (als_set_params).  The column names must agree across the
        maps.  `initial*Factors` = (ids, factors[n, rank]) injects the start point (parity path, one
        map only); without it the Spark-style XORShiftRandom initialisation is used.  `parallelism`
        (the name of Spark 2.3's CrossValidator knob) caps the maps of a list fitted at once.

        `trackObjective` / `tol` (arguments of this call, not Params): with either, the fit evaluates the
        training loss (ALSModel.objective, als_objective) after the initialisation and after every sweep;
        the model carries `objectiveHistory` (a list of floats, entry 0 = after the initialisation) and
        `sweepsRun`.  tol > 0 stops the fit after the first sweep whose relative decrease of the loss is
        below tol; the factors are those of a fit with maxIter = sweepsRun.  In a list of ParamMaps every
        map is fitted the same way.  Without either the fit is als_fit and the two attributes are None."""
        tracked = bool(trackObjective) or tol is not None
        if isinstance(params, (list, tuple)):
            return self._fit_many(dataset, [self._param_map(pm) for pm in params], max_concurrent=parallelism,
                                  tracked=tracked, tol=tol)
        pm = self._param_map(params or {})
        user, item, rating = self._ratings(dataset, pm)
        lib = load()
        h = self._context(pm)
        try:
            check(lib.als_set_ratings(h, user.size, ptr(user, C.c_int32), ptr(item, C.c_int32),
                                      ptr(rating, C.c_float)))
            for side, init in ((_lib.ALS_USER, initialUserFactors), (_lib.ALS_ITEM, initialItemFactors)):
                if init is not None:
                    ids = np.ascontiguousarray(init[0], dtype=np.int32)
                    f = np.ascontiguousarray(init[1], dtype=np.float32)
                    check(lib.als_set_initial_factors(h, side, ids.size, ptr(ids, C.c_int32), ptr(f, C.c_float)))
            fit_s, hist, ran = self._run_fit(h, pm, tracked, tol)
        except Exception:
            lib.als_destroy(h)
            raise
        model = ALSModel(h, pm, uid=self.uid)
        model.fit_seconds = fit_s
        model.objectiveHistory, model.sweepsRun = hist, ran
        return model

    def _fit_many(self, dataset, maps, max_concurrent=8, tracked=False, tol=None):
        """The CV grid (ALSRecommenderCV.scala:67-90): one ingest; the maps of one rank are fitted
        CONCURRENTLY, each on an als_fork of the ingest context (own factors and streams, shared CSR)
        driven by its own host thread; every model is bit-identical to its standalone fit.

        Each fork holds its own factor, rotation and split-K buffers, so at most `max_concurrent`
        forks exist at once and fewer when the device runs out of memory: a fork or a fit that fails
        with ALS_E_OUT_OF_MEMORY ends the batch, and its map runs again in a smaller batch (alone, if
        need be: the sequential path)."""
        if not maps:
            return []
        from concurrent.futures import ThreadPoolExecutor
        cols = ("userCol", "itemCol", "ratingCol")
        if any(m[c] != maps[0][c] for m in maps for c in cols):
            raise IllegalArgumentException(_lib.ALS_E_INVALID_ARGUMENT,
                                           "a shared-ingest multi-fit needs the same columns in every ParamMap")
        user, item, rating = self._ratings(dataset, maps[0])
        lib = load()
        h = self._context(maps[0])
        models = [None] * len(maps)

        def run(fh, pm):
            return self._run_fit(fh, pm, tracked, tol)

        def oom(e):
            return isinstance(e, _lib.ALSError) and e.code == _lib.ALS_E_OUT_OF_MEMORY

        try:
            for pm in maps:  # validate every map before the ingest (no fit runs on a bad grid)
                check(lib.als_set_params(h, C.byref(self._c_params(pm))))
            check(lib.als_set_ratings(h, user.size, ptr(user, C.c_int32), ptr(item, C.c_int32),
                                      ptr(rating, C.c_float)))
            groups = {}
            for i, pm in enumerate(maps):  # forks share the layout of one (rank, nonnegative, light limit)
                key = (int(pm["rank"]), bool(pm["nonnegative"]), int(pm["lightMaxDegree"]))
                groups.setdefault(key, []).append(i)
            for idx in groups.values():
                check(lib.als_set_params(h, C.byref(self._c_params(maps[idx[0]]))))
                todo = list(idx)
                cap = max(1, int(max_concurrent))
                while todo:
                    forks = []
                    try:
                        for i in todo[:cap]:
                            fh = C.c_void_p()
                            try:
                                check(lib.als_fork(h, C.byref(self._c_params(maps[i])), C.byref(fh)))
                            except _lib.ALSError as e:
                                if not (oom(e) and forks):
                                    raise
                                break  # fit the forks that fit in memory first
                            forks.append((i, fh))
                        with ThreadPoolExecutor(max_workers=len(forks)) as ex:
                            futs = [ex.submit(run, fh, maps[i]) for i, fh in forks]
                        done, failed = [], []
                        for (i, fh), fu in zip(forks, futs):
                            e = fu.exception()
                            if e is None:
                                fit_s, hist, ran = fu.result()
                                models[i] = self._snapshot(fh, maps[i], fit_s)
                                models[i].objectiveHistory, models[i].sweepsRun = hist, ran
                                done.append(i)
                            elif oom(e) and len(forks) > 1:
                                failed.append(i)
                            else:
                                raise e
                        cap = len(forks) if not failed else max(1, len(forks) // 2)
                        todo = [i for i in todo if i not in done]
                    finally:
                        for _, fh in forks:
                            lib.als_destroy(fh)
        finally:
            lib.als_destroy(h)
        return models

    def _snapshot(self, h, pm, fit_s):
        """A model-only context holding the fitted factors of context h (its ingest can then go)."""
        lib = load()
        k = int(pm["rank"])
        f = {}
        for side in (_lib.ALS_USER, _lib.ALS_ITEM):
            n = lib.als_num_rows(h, side)
            ids = np.empty(n, dtype=np.int32)
            fac = np.empty((n, k), dtype=np.float32)
            check(lib.als_get_factors(h, side, ptr(ids, C.c_int32), ptr(fac, C.c_float)))
            f[side] = (ids, fac)
        mh = C.c_void_p()
        (ui, uf), (ii, itf) = f[_lib.ALS_USER], f[_lib.ALS_ITEM]
        check(lib.als_model_create(k, ui.size, ptr(ui, C.c_int32), ptr(uf, C.c_float), ii.size,
                                   ptr(ii, C.c_int32), ptr(itf, C.c_float), int(pm["device"]), C.byref(mh)))
        m = ALSModel(mh, pm, uid=self.uid)
        m._cache.update(f)
        m.fit_seconds = fit_s
        return m


@_make_accessors
class ALSModel(_Params):
    """Spark ml.recommendation.ALSModel over an engine context holding both factor matrices."""

    def __init__(self, handle, params, uid=None):
        super().__init__(uid=uid)
        self._p.update(params)
        self._h = handle
        self._cache = {}
        self._loaded = False  # ALSModel.load: the estimator's params are not known
        self.objectiveHistory = None  # ALS.fit(trackObjective=True / tol=...): the loss per sweep, entry 0 = the start
        self.sweepsRun = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                load().als_destroy(h)
            except Exception:
                pass
            self._h = None

    @property
    def rank(self) -> int:
        return int(load().als_rank(self._h))

    def _factors(self, side):
        if side not in self._cache:
            lib = load()
            n = lib.als_num_rows(self._h, side)
            ids = np.empty(n, dtype=np.int32)
            f = np.empty((n, self.rank), dtype=np.float32)
            check(lib.als_get_factors(self._h, side, ptr(ids, C.c_int32), ptr(f, C.c_float)))
            self._cache[side] = (ids, f)
        return self._cache[side]

    def user_factors_np(self):
        return self._factors(_lib.ALS_USER)

    def item_factors_np(self):
        return self._factors(_lib.ALS_ITEM)

    @staticmethod
    def _frame(ids, f):
        import pandas as pd
        return pd.DataFrame({"id": ids, "features": list(f)})

    @property
    def userFactors(self):
        return self._frame(*self.user_factors_np())

    @property
    def itemFactors(self):
        return self._frame(*self.item_factors_np())

    # ---- ALSModel.transform ---------------------------------------------------------------------
    def transform(self, dataset):
        import pandas as pd
        user = _checked_cast(_column(dataset, self._p["userCol"]), self._p["userCol"])
        item = _checked_cast(_column(dataset, self._p["itemCol"]), self._p["itemCol"])
        out = np.empty(user.size, dtype=np.float32)
        check(load().als_predict(self._h, user.size, ptr(np.ascontiguousarray(user), C.c_int32),
                                 ptr(np.ascontiguousarray(item), C.c_int32), ptr(out, C.c_float)))
        df = pd.DataFrame(dataset).copy() if not isinstance(dataset, pd.DataFrame) else dataset.copy()
        df[self._p["predictionCol"]] = out
        if self._p["coldStartStrategy"] == "drop":
            df = df[~np.isnan(out)]
        return df

    # ---- recommendForAll* / recommendFor*Subset ------------------------------------------------
    def _recommend(self, side, num, subset=None):
        lib = load()
        if subset is not None:
            col = self._p["userCol"] if side == _lib.ALS_USER else self._p["itemCol"]
            # checkedCast like fit/transform: out-of-Int-range or fractional ids raise, never wrap
            sub = np.ascontiguousarray(np.unique(_checked_cast(subset, col)))
            nq = sub.size
        else:
            sub = None
            nq = lib.als_num_rows(self._h, side)
        src = np.empty(nq, dtype=np.int32)
        ids = np.empty((nq, num), dtype=np.int32)
        sc = np.empty((nq, num), dtype=np.float32)
        check(lib.als_recommend(self._h, side, int(num), ptr(sub, C.c_int32) if sub is not None else None,
                                nq, ptr(src, C.c_int32), ptr(ids, C.c_int32), ptr(sc, C.c_float)))
        return src, ids, sc

    def recommend_np(self, num, subset=None, side=_lib.ALS_USER):
        """(src ids, dst ids [n, num], scores [n, num]) sorted (score desc, id asc); -1/NaN padding."""
        return self._recommend(side, num, subset)

    def _rec_frame(self, src, ids, sc, src_col, dst_col):
        import pandas as pd
        recs = []
        for r in range(len(src)):
            m = ~np.isnan(sc[r])  # padding is told by the NaN score: -1 is a valid raw id
            recs.append([(int(i), float(s)) for i, s in zip(ids[r][m], sc[r][m])])
        keep = [i for i in range(len(src)) if recs[i]]
        return pd.DataFrame({src_col: src[keep], "recommendations": [recs[i] for i in keep]})

    def recommend_unseen_np(self, num, subset=None, side=_lib.ALS_USER, exclude=None):
        """recommend_np without each src row's known pairs (als_recommend_unseen).  exclude=None leaves out the
        dst rows of the row's ratings in the fitted context; exclude=(src ids, dst ids) leaves out those pairs
        (any order, repeats and unknown ids allowed), which is what a loaded model needs."""
        lib = load()
        if subset is not None:
            col = self._p["userCol"] if side == _lib.ALS_USER else self._p["itemCol"]
            sub = np.ascontiguousarray(np.unique(_checked_cast(subset, col)))
            nq = sub.size
        else:
            sub = None
            nq = lib.als_num_rows(self._h, side)
        mode, n_excl, es, ed = _lib.ALS_EXCLUDE_RATINGS, 0, None, None
        if exclude is not None:
            es = np.ascontiguousarray(exclude[0], dtype=np.int32).reshape(-1)
            ed = np.ascontiguousarray(exclude[1], dtype=np.int32).reshape(-1)
            if es.size != ed.size:
                raise ValueError("exclude should be (src ids, dst ids) of one length")
            mode, n_excl = _lib.ALS_EXCLUDE_PAIRS, int(es.size)
        src = np.empty(nq, dtype=np.int32)
        ids = np.empty((nq, max(int(num), 0)), dtype=np.int32)
        sc = np.empty((nq, max(int(num), 0)), dtype=np.float32)
        check(lib.als_recommend_unseen(self._h, side, int(num), ptr(sub, C.c_int32) if sub is not None else None, nq,
                                       mode, n_excl, ptr(es, C.c_int32) if n_excl else None,
                                       ptr(ed, C.c_int32) if n_excl else None, ptr(src, C.c_int32), ptr(ids, C.c_int32),
                                       ptr(sc, C.c_float)))
        return src, ids, sc

    def unseen_stats(self):
        """als_recommend_unseen_stats of the last call: rows served, rows through the exact scan, list entries
        the filter removed, dst rows the exact scan scored."""
        out = np.zeros(4, dtype=np.int64)
        check(load().als_recommend_unseen_stats(self._h, ptr(out, C.c_int64)))
        return dict(zip(("rows", "rows_exact", "entries_removed", "dst_rows_scored"), out.tolist()))

    def unseen_timing(self):
        """als_recommend_unseen_timing of the last call, device ms per stage."""
        out = np.zeros(5, dtype=np.float64)
        check(load().als_recommend_unseen_timing(self._h, ptr(out, C.c_double)))
        return dict(zip(("exclusions", "lists", "filter", "exact", "total"), out.tolist()))

    def _cols(self, side):
        u, i = self._p["userCol"], self._p["itemCol"]
        return (u, i) if side == _lib.ALS_USER else (i, u)

    def _recommend_all(self, side, num, excludeKnown):
        rec = self.recommend_unseen_np(num, None, side) if excludeKnown else self._recommend(side, num)
        return self._rec_frame(*rec, *self._cols(side))

    def recommendForAllUsers(self, numItems, excludeKnown=False):
        """Spark's recommendForAllUsers.  excludeKnown: each user's list leaves out the items of their ratings in
        the fitted context (als_recommend_unseen); a loaded model holds none and raises."""
        return self._recommend_all(_lib.ALS_USER, numItems, excludeKnown)

    def recommendForAllItems(self, numUsers, excludeKnown=False):
        return self._recommend_all(_lib.ALS_ITEM, numUsers, excludeKnown)

    def _recommend_subset(self, side, dataset, num, exclude, excludeKnown):
        src_col, dst_col = self._cols(side)
        rows = _column(dataset, src_col)
        if excludeKnown:
            if exclude is not None:
                raise ValueError("exclude and excludeKnown are alternatives: give one of them")
            return self._rec_frame(*self.recommend_unseen_np(num, rows, side), src_col, dst_col)
        if exclude is not None:  # the rows' factors go through als_recommend_vectors as queries
            sid, F = self._factors(side)
            sub = np.unique(_checked_cast(rows, src_col))
            at = np.minimum(np.searchsorted(sid, sub), max(sid.size - 1, 0))
            known = sid[at] == sub if sid.size else np.zeros(sub.size, bool)  # unknown ids get no row
            sub, at = sub[known], at[known]
            excl = self._exclusions(sub, _column(exclude, src_col), _column(exclude, dst_col))
            ids, sc = self.recommend_vectors_np(F[at], num, excl, "item" if side == _lib.ALS_USER else "user")
            return self._rec_frame(sub, ids, sc, src_col, dst_col)
        return self._rec_frame(*self._recommend(side, num, rows), src_col, dst_col)

    def recommendForUserSubset(self, dataset, numItems, exclude=None, excludeKnown=False):
        """Spark's recommendForUserSubset.  exclude: a frame of (userCol, itemCol) rows; each user's lists then
        leave out the items the frame gives them (their factors go through als_recommend_vectors as queries).
        excludeKnown: leave out the items of each user's ratings in the fitted context (als_recommend_unseen)."""
        return self._recommend_subset(_lib.ALS_USER, dataset, numItems, exclude, excludeKnown)

    def recommendForItemSubset(self, dataset, numUsers, exclude=None, excludeKnown=False):
        return self._recommend_subset(_lib.ALS_ITEM, dataset, numUsers, exclude, excludeKnown)

    # ---- RankingEvaluator on the device (RankingEvaluator.scala:83-139) ----------------------------
    def evaluate_ndcg(self, users, items, keys, k=30, per_user=False):
        """NDCG@k of this model's top-k recommendations against intoUserActualItems(users, items,
        keys desc, k), computed on the device (als_evaluate_ndcg): the albedo protocol of
        ALSRecommenderBuilder.scala:92-104 without the lists leaving HBM.  Returns the mean, or
        (mean, user ids, per-user values) with per_user=True."""
        lib = load()
        u = np.ascontiguousarray(_checked_cast(users, self._p["userCol"]))
        it = np.ascontiguousarray(_checked_cast(items, self._p["itemCol"]))
        ky = np.asarray(keys)
        if ky.dtype.kind == "M":  # starred_at timestamps
            ky = ky.astype("datetime64[us]").astype(np.int64)
        ky = np.ascontiguousarray(ky, dtype=np.int64)
        if not (u.size == it.size == ky.size):
            raise ValueError("users, items and keys must have the same length")
        mean = C.c_double()
        nu = C.c_int64()
        cap = int(np.unique(u).size) if per_user else 0
        uo = np.empty(max(cap, 1), np.int32)
        vo = np.empty(max(cap, 1), np.float64)
        check(lib.als_evaluate_ndcg(self._h, int(k), u.size, ptr(u, C.c_int32), ptr(it, C.c_int32),
                                    ptr(ky, C.c_int64), C.byref(mean), C.byref(nu),
                                    ptr(uo, C.c_int32) if per_user else None,
                                    ptr(vo, C.c_double) if per_user else None, cap))
        if per_user:
            return mean.value, uo[:nu.value], vo[:nu.value]
        return mean.value

    @staticmethod
    def _keys_i64(keys):
        ky = np.asarray(keys)
        if ky.dtype.kind == "M":  # starred_at timestamps
            ky = ky.astype("datetime64[us]").astype(np.int64)
        return np.ascontiguousarray(ky, dtype=np.int64)

    @staticmethod
    def _metric_code(metric):
        if metric not in _lib.METRICS:
            raise ValueError(f"unsupported metric {metric}; supports {', '.join(_lib.METRICS)}")
        return _lib.METRICS[metric]

    def evaluate_ranking(self, users, items, keys, k=30, metric="NDCG@k", per_user=False):
        """`evaluate_ndcg` with RankingEvaluator's metricName ("NDCG@k", "Precision@k", "MAP";
        RankingEvaluator.scala:21,97-101) on the device (als_evaluate_ranking)."""
        code = self._metric_code(metric)
        u = np.ascontiguousarray(_checked_cast(users, self._p["userCol"]))
        it = np.ascontiguousarray(_checked_cast(items, self._p["itemCol"]))
        ky = self._keys_i64(keys)
        if not (u.size == it.size == ky.size):
            raise ValueError("users, items and keys must have the same length")
        mean = C.c_double()
        nu = C.c_int64()
        cap = int(np.unique(u).size) if per_user else 0
        uo = np.empty(max(cap, 1), np.int32)
        vo = np.empty(max(cap, 1), np.float64)
        check(load().als_evaluate_ranking(self._h, code, int(k), u.size, ptr(u, C.c_int32), ptr(it, C.c_int32),
                                          ptr(ky, C.c_int64), C.byref(mean), C.byref(nu),
                                          ptr(uo, C.c_int32) if per_user else None,
                                          ptr(vo, C.c_double) if per_user else None, cap))
        if per_user:
            return mean.value, uo[:nu.value], vo[:nu.value]
        return mean.value

    # ---- held-out pairs (ALSRecommenderCV.scala:54-90, RankingMetricFormatter.scala:59-64) -----------
    def rank_pairs(self, users, items, topK=15, width=None):
        """RankingMetricFormatter("als") of transform(pairs) with coldStartStrategy "drop", on the
        device (als_rank_pairs): per user with a surviving pair, the pairs with rank() over
        (prediction desc) <= topK in (score desc, item asc) order, cut to `width` (default topK; ties
        at the boundary make a list longer than topK).  Returns (user ids ascending, lengths,
        items [n, width] padded with -1, scores [n, width] padded with NaN)."""
        width = int(topK if width is None else width)
        u = np.ascontiguousarray(_checked_cast(users, self._p["userCol"]))
        it = np.ascontiguousarray(_checked_cast(items, self._p["itemCol"]))
        if u.size != it.size:
            raise ValueError("users and items must have the same length")
        cap = max(int(np.unique(u).size), 1)
        nu = C.c_int64()
        uo, ln = np.empty(cap, np.int32), np.empty(cap, np.int32)
        io = np.empty((cap, max(width, 1)), np.int32)
        so = np.empty((cap, max(width, 1)), np.float32)
        check(load().als_rank_pairs(self._h, int(topK), width, u.size, ptr(u, C.c_int32), ptr(it, C.c_int32),
                                    C.byref(nu), ptr(uo, C.c_int32), ptr(ln, C.c_int32), ptr(io, C.c_int32),
                                    ptr(so, C.c_float), cap))
        n = nu.value
        return uo[:n], ln[:n], io[:n], so[:n]

    def evaluate_pairs(self, users, items, actual_users, actual_items, actual_keys, metric="NDCG@k", topK=15, k=30,
                       per_user=False):
        """RankingEvaluator(metric, k).evaluate of `rank_pairs(users, items, topK, width=k)` against
        intoUserActualItems(actual_*, keys desc, k), without the lists leaving the device
        (als_evaluate_pairs): one fold's step of ALSRecommenderCV.scala:72-90.  Returns the mean, or
        (mean, user ids, per-user values) with per_user=True."""
        code = self._metric_code(metric)
        u = np.ascontiguousarray(_checked_cast(users, self._p["userCol"]))
        it = np.ascontiguousarray(_checked_cast(items, self._p["itemCol"]))
        au = np.ascontiguousarray(_checked_cast(actual_users, self._p["userCol"]))
        ai = np.ascontiguousarray(_checked_cast(actual_items, self._p["itemCol"]))
        ak = self._keys_i64(actual_keys)
        if u.size != it.size or not (au.size == ai.size == ak.size):
            raise ValueError("the columns of the pairs, and those of the actual rows, must have the same length")
        mean = C.c_double()
        nu = C.c_int64()
        cap = int(np.unique(u).size) if per_user else 0
        uo = np.empty(max(cap, 1), np.int32)
        vo = np.empty(max(cap, 1), np.float64)
        check(load().als_evaluate_pairs(self._h, code, int(topK), int(k), u.size, ptr(u, C.c_int32), ptr(it, C.c_int32),
                                        au.size, ptr(au, C.c_int32), ptr(ai, C.c_int32), ptr(ak, C.c_int64),
                                        C.byref(mean), C.byref(nu), ptr(uo, C.c_int32) if per_user else None,
                                        ptr(vo, C.c_double) if per_user else None, cap))
        if per_user:
            return mean.value, uo[:nu.value], vo[:nu.value]
        return mean.value

    def eval_pairs_timing(self):
        """Device ms of the last rank_pairs / evaluate_pairs: map, sort, score, select, metric."""
        out = np.zeros(5, np.float64)
        check(load().als_eval_pairs_timing(self._h, ptr(out, C.c_double)))
        return dict(zip(("map", "sort", "score", "select", "metric"), out.tolist()))

    def audit(self, side, tol, per_row=False):
        """als_audit_rows: every row of `side` against its normal equation, in fp64 on the device.

        Returns the summary as a dict (rows, rows_over, non_finite, negative, worst_id, worst_degree,
        worst_path as a name of _lib.PATH_NAMES, worst_eta, sum_eta) and, with per_row, the relative
        residual of every row in ascending id order.  Needs the ratings: a model of ALS.fit(dataset) has
        them, a loaded model or one of a ParamMap list does not (IllegalStateException)."""
        lib = load()
        a = _lib.als_audit()
        eta = np.empty(max(int(lib.als_num_rows(self._h, int(side))), 0), np.float64) if per_row else None
        check(lib.als_audit_rows(self._h, int(side), float(tol), ptr(eta, C.c_double) if per_row else None, C.byref(a)))
        out = {name: getattr(a, name) for name, _ in _lib.als_audit._fields_}
        out["worst_path"] = _lib.PATH_NAMES[a.worst_path] if a.worst_path >= 0 else None
        return (out, eta) if per_row else out

    def objective(self, side="user", per_row=False):
        """als_objective: the loss ALS minimises, in fp64 on the device, walked through the rows of `side`.

        Returns a dict of als_objective_t's fields (total, all_pairs, ratings, reg_side, reg_other, sse,
        abs_terms, n_ratings, rows) with `rmse` = sqrt(sse / n_ratings) and, with per_row, each row's loss in
        ascending id order.  Needs the ratings, like audit: a loaded model or one of a ParamMap list raises
        IllegalStateException."""
        lib = load()
        side = self._side(side)
        o = _lib.als_objective_t()
        loss = np.empty(max(int(lib.als_num_rows(self._h, side)), 0), np.float64) if per_row else None
        check(lib.als_objective(self._h, side, ptr(loss, C.c_double) if per_row else None, C.byref(o)))
        out = {name: getattr(o, name) for name, _ in _lib.als_objective_t._fields_}
        out["rmse"] = float(np.sqrt(o.sse / o.n_ratings)) if o.n_ratings > 0 else float("nan")
        return (out, loss) if per_row else out

    def objective_timing(self):
        """Device ms of the last objective call: the fp64 Gram, the row pass and the sums, total."""
        out = np.zeros(3, np.float64)
        check(load().als_objective_timing(self._h, ptr(out, C.c_double)))
        return dict(zip(("gram", "rows", "total"), out.tolist()))

    # ---- fold-in: factors for rows the fit did not see (als_fold_in) ---------------------------------
    def _fold_params(self, regParam, alpha, implicitPrefs, nonnegative=None):
        vals = dict(regParam=regParam, alpha=alpha, implicitPrefs=implicitPrefs)
        for k, v in vals.items():
            if v is None:
                if self._loaded:  # Spark's saved ALSModel carries the rank and the column names only
                    raise ValueError(f"foldIn on a loaded ALSModel needs {k}: the saved model does not carry it")
                vals[k] = self._p[k]
        if nonnegative is None:  # a loaded model does not know how it was fitted: Cholesky unless told
            nonnegative = False if self._loaded else self._p["nonnegative"]
        return float(vals["regParam"]), float(vals["alpha"]), bool(vals["implicitPrefs"]), bool(nonnegative)

    @staticmethod
    def _side(side):
        if side in ("user", _lib.ALS_USER):
            return _lib.ALS_USER
        if side in ("item", _lib.ALS_ITEM):
            return _lib.ALS_ITEM
        raise ValueError(f"side should be 'user' or 'item', not {side!r}")

    def fold_in_np(self, rows, srcs, ratings, side="user", regParam=None, alpha=None, implicitPrefs=None,
                   nonnegative=None):
        """(ids ascending, degrees, factors [n, rank]) of the distinct ids of `rows`, each solved from its
        (row, src, rating) triples against the model's frozen factors of the other side (als_fold_in).
        Triples with a src id the model does not know are dropped; a row left with none gets zeros.
        nonnegative: each row by Spark's NNLS, as ALS(nonnegative=True) computes it, in place of the Cholesky."""
        t = self._side(side)
        cols = (self._p["userCol"], self._p["itemCol"])
        reg, al, imp, nn = self._fold_params(regParam, alpha, implicitPrefs, nonnegative)
        r = np.ascontiguousarray(_checked_cast(rows, cols[t]))
        s = np.ascontiguousarray(_checked_cast(srcs, cols[1 - t]))
        return _lib.fold_in(self._h, t, r, s, np.ascontiguousarray(ratings, dtype=np.float32), self.rank, reg, al, imp,
                            nonnegative=nn)

    def foldIn(self, dataset, side="user", regParam=None, alpha=None, implicitPrefs=None, nonnegative=None):
        """Factors of new users (side="user") or items from their ratings, as a frame of (id, features)
        shaped like userFactors.  A model of ALS.fit defaults regParam, alpha, implicitPrefs and nonnegative to
        its own; a loaded model needs the first three, and solves by Cholesky unless nonnegative=True."""
        t = self._side(side)
        self._fold_params(regParam, alpha, implicitPrefs, nonnegative)  # a missing parameter is named before a missing column
        cols = (self._p["userCol"], self._p["itemCol"])
        ids, _, f = self.fold_in_np(_column(dataset, cols[t]), _column(dataset, cols[1 - t]),
                                    _column(dataset, self._p["ratingCol"]), t, regParam, alpha, implicitPrefs, nonnegative)
        return self._frame(ids, f)

    def _exclusions(self, ids, users, items):
        """(ptr, item ids) for als_recommend_vectors: for each of the ascending user ids, their items among the
        (user, item) rows."""
        u = _checked_cast(users, self._p["userCol"])
        it = _checked_cast(items, self._p["itemCol"])
        if u.size != it.size:
            raise ValueError("the user and item columns must have the same length")
        o = np.argsort(u, kind="stable")
        us = u[o]
        ptr_ = np.zeros(len(ids) + 1, np.int64)
        np.cumsum(np.searchsorted(us, ids, "right") - np.searchsorted(us, ids, "left"), out=ptr_[1:])
        keep = o[np.isin(us, ids)]  # sorted by user like ids: the rows of other users are left out
        return ptr_, np.ascontiguousarray(it[keep], dtype=np.int32)

    def recommend_vectors_np(self, vectors, num, exclude=None, side="item"):
        """(dst ids [n, num], scores [n, num]) of the exact top-num of each row of `vectors` [n, rank] against
        the factors of `side` ("item": items are recommended; "user": users), sorted (score desc, id asc) with
        -1 / NaN padding (als_recommend_vectors; num <= 64).  The score is the F2J dot product of the vector
        and the row's factor.  exclude: one array of raw dst ids per vector (a list), or a (ptr, ids) tuple in
        CSR form; those rows are not listed.  Unknown and repeated ids are ignored."""
        return _lib.recommend_vectors(self._h, self._side(side), vectors, num, self.rank, exclude)

    def recommendForVectors(self, ids, vectors, num, exclude=None, side="item"):
        """recommend_vectors_np as the usual recommendation frame: `ids` label the vectors (the userCol column
        when items are recommended, the itemCol column with side="user")."""
        t = self._side(side)
        src_col, dst_col = ((self._p["userCol"], self._p["itemCol"]) if t == _lib.ALS_ITEM
                            else (self._p["itemCol"], self._p["userCol"]))
        src = np.asarray(ids)
        if src.ndim != 1 or src.shape[0] != np.shape(vectors)[0]:
            raise ValueError("ids should be one-dimensional, one per vector")
        dst, sc = self.recommend_vectors_np(vectors, num, exclude, t)
        return self._rec_frame(src, dst, sc, src_col, dst_col)

    def recommend_vectors_timing(self):
        """Device ms of the last recommend_vectors_np: exclusions (map + sort), scan, merge, total."""
        return dict(zip(("exclusions", "scan", "merge", "total"), _lib.recommend_vectors_timing(self._h).tolist()))

    # ---- cosine top-k within one side -----------------------------------------------------------
    def similar_np(self, num, subset=None, side="item"):
        """(src ids [n], ids [n, num], scores [n, num]): for each requested row of `side` (raw ids in `subset`,
        caller order, repeats kept; None: every row, ascending) the num <= 64 other rows of the same side with
        the largest cosine, sorted (score desc, id asc) with -1 / NaN padding (als_similar).  The row itself
        and rows without a direction (zero, non-finite) are never listed; unknown ids give an all-padding row."""
        t = self._side(side)
        if subset is not None:
            subset = _checked_cast(subset, self._p["userCol"] if t == _lib.ALS_USER else self._p["itemCol"])
        return _lib.similar(self._h, t, num, subset)

    def _similar_frame(self, side, dataset, num):
        import pandas as pd
        col = self._cols(side)[0]
        sub = None if dataset is None else np.unique(_checked_cast(_column(dataset, col), col))
        src, ids, sc = self.similar_np(num, sub, side)
        sims = []
        for r in range(len(src)):
            m = ~np.isnan(sc[r])  # padding is told by the NaN score: -1 is a valid raw id
            sims.append([(int(i), float(s)) for i, s in zip(ids[r][m], sc[r][m])])
        keep = [i for i in range(len(src)) if sims[i]]
        return pd.DataFrame({col: src[keep], "similarities": [sims[i] for i in keep]})

    def similarItems(self, dataset, numItems):
        """For each distinct item of `dataset`'s itemCol (None: every item of the model) the numItems most similar
        other items by cosine, as a frame (itemCol, similarities) shaped like recommendForItemSubset's; items
        the model does not know, and items with an empty list, have no row."""
        return self._similar_frame(_lib.ALS_ITEM, dataset, numItems)

    def similarUsers(self, dataset, numUsers):
        """similarItems on the user side: frame (userCol, similarities)."""
        return self._similar_frame(_lib.ALS_USER, dataset, numUsers)

    def similar_vectors_np(self, vectors, num, exclude=None, side="item"):
        """recommend_vectors_np with the cosine as the score: each row of `vectors` [n, rank] (a folded-in user, an
        average of repos) against the rows of `side` (als_similar_vectors).  A zero or non-finite vector gives
        an all-padding list; `exclude` as in recommend_vectors_np."""
        return _lib.similar_vectors(self._h, self._side(side), vectors, num, self.rank, exclude)

    def similar_timing(self):
        """Device ms of the last similar_np / similar_vectors_np: unit image, lists, merge / filter, total."""
        return dict(zip(("unit_image", "lists", "merge", "total"), _lib.similar_timing(self._h).tolist()))

    def similar_stats(self):
        """Counters of the last similar_np / similar_vectors_np: rows asked and known, rows of the side without a
        direction, tier (0 scan, 1 passes), rows the passes tier sent to its exact scan."""
        return dict(zip(("rows", "no_direction", "tier", "rows_exact"), _lib.similar_stats(self._h).tolist()))

    def recommendForNewUsers(self, dataset, numItems, excludeKnown=False, explain=None, **fold_kw):
        """recommendForUserSubset for users the model has not seen: their factors are folded in from
        `dataset` (foldIn's keywords apply), then scored against the model's items on the model's own
        context (als_recommend_vectors).  excludeKnown: a user's lists leave out their items in `dataset`.
        numItems > 64 is served by als_recommend on a transient context, without excludeKnown.
        explain=m adds an `explanation` column: for every listed item a dict of the item, its `score` in fp64
        before the factor was rounded (als_explain's total) and its `explanation`, the m ratings of the user
        that contribute most, as (item id, contribution)."""
        self._fold_params(*(fold_kw.get(k) for k in ("regParam", "alpha", "implicitPrefs", "nonnegative")))
        users, items = _column(dataset, self._p["userCol"]), _column(dataset, self._p["itemCol"])
        ratings = _column(dataset, self._p["ratingCol"])
        ids, _, f = self.fold_in_np(users, items, ratings, _lib.ALS_USER, **fold_kw)
        if int(numItems) > 64 and not excludeKnown:
            if explain is not None:
                raise ValueError("explain goes with numItems <= 64")
            return self._recommend_transient(ids, f, numItems)
        excl = self._exclusions(ids, users, items) if excludeKnown else None
        dst, sc = self.recommend_vectors_np(f, numItems, excl, "item")
        out = self._rec_frame(ids, dst, sc, self._p["userCol"], self._p["itemCol"])
        if explain is None:
            return out
        fold_kw.pop("nonnegative", None)  # resolved above: explain_np refuses an NNLS model itself
        listed = ~np.isnan(sc)
        pu, pt = np.repeat(ids, listed.sum(axis=1)), dst[listed]
        total, eids, ev = self.explain_np(users, items, ratings, pu, pt, explain, "user", **fold_kw)
        by_user, at = {}, 0
        for r in range(len(ids)):
            n = int(listed[r].sum())
            if n:
                by_user[int(ids[r])] = [
                    {self._p["itemCol"]: int(pt[p]), "score": float(total[p]),
                     "explanation": self._explanation(eids[p], ev[p])} for p in range(at, at + n)]
            at += n
        out["explanation"] = [by_user[int(u)] for u in out[self._p["userCol"]]]
        return out

    # ---- explanations: each rating's share of a score (als_explain) ----------------------------------
    @staticmethod
    def _explanation(ids, values):
        m = ~np.isnan(values)  # the NaN tells the padding: -1 is a valid raw id
        return [(int(i), float(v)) for i, v in zip(ids[m], values[m])]

    def explain_np(self, rows, srcs, ratings, pair_rows, pair_targets, num=10, side="user", regParam=None, alpha=None,
                   implicitPrefs=None):
        """(total [n_pairs], src ids [n_pairs, num], contributions [n_pairs, num]) of als_explain: for each pair
        (row, target) the share of the row's score for the target that each of the row's ratings contributes,
        the `num` largest by (value desc, id asc) with -1 / NaN padding, and their sum over all the row's
        ratings.  The rows are given by their (row, src, rating) triples as for fold_in_np; with side="user" the
        targets are items.  A model fitted with nonnegative=True has no such decomposition: an NNLS row is not
        linear in its ratings."""
        t = self._side(side)
        cols = (self._p["userCol"], self._p["itemCol"])
        reg, al, imp, nn = self._fold_params(regParam, alpha, implicitPrefs)
        if nn:
            raise ValueError("explain: an NNLS row is not linear in its ratings, so this decomposition is not its "
                             "score (the model was fitted with nonnegative=True)")
        r = np.ascontiguousarray(_checked_cast(rows, cols[t]))
        s = np.ascontiguousarray(_checked_cast(srcs, cols[1 - t]))
        pr = np.ascontiguousarray(_checked_cast(pair_rows, cols[t]))
        pt = np.ascontiguousarray(_checked_cast(pair_targets, cols[1 - t]))
        return _lib.explain(self._h, t, r, s, np.ascontiguousarray(ratings, dtype=np.float32), pr, pt, num, reg, al, imp)

    def _row_ratings(self, side, rid):
        lib = load()
        n = np.zeros(1, np.int64)
        check(lib.als_get_row_ratings(self._h, side, int(rid), 0, None, None, ptr(n, C.c_int64)))
        src, r = np.empty(max(int(n[0]), 1), np.int32), np.empty(max(int(n[0]), 1), np.float32)
        check(lib.als_get_row_ratings(self._h, side, int(rid), int(n[0]), ptr(src, C.c_int32), ptr(r, C.c_float),
                                      ptr(n, C.c_int64)))
        return src[:int(n[0])], r[:int(n[0])]

    def explain(self, pairs, dataset=None, num=10, side="user", regParam=None, alpha=None, implicitPrefs=None):
        """One row per (userCol, itemCol) pair of `pairs`: the two ids, `score` (the fp64 total) and
        `explanation`, the list of (src id, contribution) of the `num` ratings that contribute most: for
        side="user" the user's items ("because you starred X"), for side="item" the item's users.  The
        ratings come from `dataset` (userCol, itemCol, ratingCol); with dataset=None, on a model that still
        holds the ratings it was fitted on (not a loaded one), each distinct row's own ratings are used."""
        import pandas as pd
        t = self._side(side)
        cols = (self._p["userCol"], self._p["itemCol"])
        self._fold_params(regParam, alpha, implicitPrefs)  # a missing parameter is named before a missing column
        pr, pt = _column(pairs, cols[t]), _column(pairs, cols[1 - t])
        if dataset is None:
            if self._loaded:
                raise ValueError("explain on a loaded ALSModel needs dataset: the saved model does not carry the ratings")
            known = self._factors(t)[0]
            rows, srcs, ratings = [], [], []
            for rid in np.unique(_checked_cast(pr, cols[t])):
                at = np.searchsorted(known, rid)
                if at < known.size and known[at] == rid:  # a row the model does not know has no ratings here
                    s, r = self._row_ratings(t, rid)
                    rows.append(np.full(s.size, rid, np.int32))
                    srcs.append(s)
                    ratings.append(r)
            rows, srcs, ratings = (np.concatenate(a) if a else np.zeros(0, d)
                                   for a, d in ((rows, np.int32), (srcs, np.int32), (ratings, np.float32)))
        else:
            rows, srcs = _column(dataset, cols[t]), _column(dataset, cols[1 - t])
            ratings = _column(dataset, self._p["ratingCol"])
        total, ids, ev = self.explain_np(rows, srcs, ratings, pr, pt, num, t, regParam, alpha, implicitPrefs)
        return pd.DataFrame({cols[t]: np.asarray(pr), cols[1 - t]: np.asarray(pt), "score": total,
                             "explanation": [self._explanation(ids[p], ev[p]) for p in range(len(total))]})

    def explain_timing(self):
        """Device ms of the last explain: csr (map + sort + CSR of triples and pairs), gram (0 when cached),
        solve (build, factor, solves, contributions, selection), total."""
        return dict(zip(("csr", "gram", "solve", "total"), _lib.explain_timing(self._h).tolist()))

    def _recommend_transient(self, ids, f, numItems):
        """als_recommend of the given user rows on a model-only context of their own (numItems > 64)."""
        lib = load()
        ii, itf = self.item_factors_np()
        ii, itf = np.ascontiguousarray(ii), np.ascontiguousarray(itf)
        h = C.c_void_p()
        check(lib.als_model_create(self.rank, ids.size, ptr(ids, C.c_int32), ptr(f, C.c_float), ii.size,
                                   ptr(ii, C.c_int32), ptr(itf, C.c_float), int(self._p["device"]), C.byref(h)))
        try:
            src = np.empty(ids.size, dtype=np.int32)
            dst = np.empty((ids.size, numItems), dtype=np.int32)
            sc = np.empty((ids.size, numItems), dtype=np.float32)
            check(lib.als_recommend(h, _lib.ALS_USER, int(numItems), None, ids.size, ptr(src, C.c_int32),
                                    ptr(dst, C.c_int32), ptr(sc, C.c_float)))
        finally:
            lib.als_destroy(h)
        return self._rec_frame(src, dst, sc, self._p["userCol"], self._p["itemCol"])

    def fold_in_timing(self):
        """Device ms of the last fold-in: csr (map + sort + CSR), gram (0 when cached), solve, total."""
        return dict(zip(("csr", "gram", "solve", "total"), _lib.fold_in_timing(self._h).tolist()))

    def fold_in_stats(self):
        """NNLS iterations of the last fold-in: iterations (summed over rows), max_iterations, rows (solved by
        NNLS), rows_at_limit; all 0 after a Cholesky fold-in."""
        return dict(zip(("iterations", "max_iterations", "rows", "rows_at_limit"), _lib.fold_in_stats(self._h).tolist()))

    # ---- persistence (Spark 2.2 ALSModelWriter / ALSModelReader layout: albedo_amd/persistence.py) ----
    MODEL_PARAMS = ("userCol", "itemCol", "predictionCol", "coldStartStrategy")  # ALSModelParams

    def save(self, path, overwrite=False, rows_per_part=1 << 20):
        from . import persistence
        persistence.save_als_model(path, self.uid, {k: self._p[k] for k in self.MODEL_PARAMS}, self.rank,
                                   self.user_factors_np(), self.item_factors_np(), overwrite, rows_per_part)

    def write(self):
        model = self

        class _Writer:
            _ow = False

            def overwrite(self):
                self._ow = True
                return self

            def save(self, path):
                model.save(path, overwrite=self._ow)

        return _Writer()

    @classmethod
    def load(cls, path, device=-1):
        from . import persistence
        meta, (uid, uf), (iid, itf) = persistence.load_als_model(path)
        rank = int(meta["rank"])
        h = C.c_void_p()
        check(load().als_model_create(rank, uid.size, ptr(uid, C.c_int32), ptr(uf, C.c_float), iid.size,
                                      ptr(iid, C.c_int32), ptr(itf, C.c_float), int(device), C.byref(h)))
        params = dict(_Params._defaults)
        params.update({k: v for k, v in meta.get("paramMap", {}).items() if k in _Params._defaults})
        params["rank"] = rank
        model = cls(h, params, uid=meta.get("uid"))
        model._loaded = True
        return model

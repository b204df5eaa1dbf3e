"""ALSRecommenderCV.main (ALSRecommenderCV.scala:40-100) on the MI355X engine.

    python -m albedo_amd.cv [--users U --repos I --stars N --ranks 50,70 --max-iters 20 --folds 2]

Same protocol as the reference job (`make cv_als`):
  1. load the starring rows (user_id, repo_id, starred_at, starring = 1.0)            (:42)
  2. ALS(implicitPrefs, seed 42, coldStartStrategy "drop", user_id / repo_id / starring)
     followed by RankingMetricFormatter("als"), topK left at its default 15            (:46-63)
  3. grid rank {50, 70} x regParam {0.1, 0.5} x alpha {0.1, 40} x maxIter {20}         (:67-72)
  4. RankingEvaluator(loadUserActualItemsDF(30)), NDCG@30, of the WHOLE dataset         (:74-82)
  5. CrossValidator with 2 folds                                                        (:84-90)
  6. print "metric: ParamMap" per map, best first                                       (:94-99)

The starring rows follow builder.py's conventions (the parquet cache, else the seeded synthetic
stand-in).  Spark's fold membership cannot be reproduced (tuning.k_fold); the folds take `--seed`.
"""
from __future__ import annotations

import argparse

from .als import ALS
from .builder import load_raw_starring
from .tuning import CrossValidator, DeviceRankingEvaluator, ParamGridBuilder


def _list(cast):
    return lambda s: [cast(x) for x in str(s).split(",") if x != ""]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--repos", type=int, default=4000)
    ap.add_argument("--stars", type=int, default=400000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--starring-path", default=None,
                    help="parquet directory of Starring rows (default dataDir/today/rawStarringDF.parquet)")
    ap.add_argument("--no-cache", action="store_true", help="generate the synthetic rows in memory, no parquet cache")
    ap.add_argument("--ranks", type=_list(int), default=[50, 70])
    ap.add_argument("--reg-params", type=_list(float), default=[0.1, 0.5])
    ap.add_argument("--alphas", type=_list(float), default=[0.1, 40.0])
    ap.add_argument("--max-iters", type=_list(int), default=[20])
    ap.add_argument("--folds", type=int, default=2)
    ap.add_argument("--top-k", type=int, default=30, help="k of the evaluator and of the actual lists")
    ap.add_argument("--formatter-top-k", type=int, default=15, help="RankingMetricFormatter's topK")
    ap.add_argument("--metric", default="NDCG@k", choices=["NDCG@k", "Precision@k", "MAP"])
    args = ap.parse_args(argv)

    stars = load_raw_starring(args.users, args.repos, args.stars, args.seed,
                              path=False if args.no_cache else args.starring_path)
    als = (ALS().setImplicitPrefs(True).setSeed(42).setColdStartStrategy("drop")
           .setUserCol("user_id").setItemCol("repo_id").setRatingCol("starring"))
    grid = (ParamGridBuilder().addGrid("rank", args.ranks).addGrid("regParam", args.reg_params)
            .addGrid("alpha", args.alphas).addGrid("maxIter", args.max_iters).build())
    evaluator = DeviceRankingEvaluator(stars["user_id"], stars["repo_id"], stars["starred_at"],
                                       metricName=args.metric, k=args.top_k, formatterTopK=args.formatter_top_k)
    cv = CrossValidator(estimator=als, estimatorParamMaps=grid, evaluator=evaluator, numFolds=args.folds,
                        seed=args.seed)
    data = {k: stars[k] for k in ("user_id", "repo_id", "starring")}
    cv_model = cv.fit(data)
    pairs = sorted(zip(cv_model.avgMetrics, range(len(grid))), key=lambda p: (-p[0], p[1]))
    for metric, i in pairs:
        print(f"{metric}: {grid[i]}")
    return cv_model


if __name__ == "__main__":
    main()

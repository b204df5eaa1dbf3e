"""Shared pieces of the sharded-path edge tests (tests/test_shard_cases.py on the CPU, tests/shard_worker.py
and tests/test_gpu_shard_edges.py on the GPU): three small problems whose shard plans reach the layout
edges of the world > 1 path, a plain numpy restatement of that layout, the injected factors, the inputs of
the top-k / evaluation / prediction calls, and the per-row label of a failure message.

Problems (all deterministic, fixed seeds)
  ladder  tests/ladder.py's degree ladder with `varying` ratings: 52 item rows on both sides of every
          kernel boundary, 700 users.  The item side at world 3 gives the last rank 5 rows (one layout
          chunk: three of its four chunks are all padding while the other ranks fill theirs), at world 4
          two ranks with 3 rows.
  skew    1500 users, 160 items; the item with the lowest raw id is rated by every user and the other 159
          by 1..7 users, so at world 3 and 4 rank 1 owns NO item row (plan_shards gives it an empty range
          whenever one row holds more than 1 / world of the ratings).  The user side stays balanced.
  tiny    40 users, 3 items of degree 30 / 25 / 35 at rank 3: chpad = 1 with fewer rows than the 4 gather
          chunks, the last rank or ranks empty, and an item-side top-k with fewer src rows than ranks.

Layout (albedo_amd/csrc: host_math.cpp plan_shards, als_engine.cpp ingest_device, engine.h Side::pos,
topk_host.cpp rank_slice): a side's dense rows are cut into `world` contiguous shards balanced by
ratings; with maxrows the largest shard, chpad = max(1, ceil(maxrows / 4)); local row i of rank r sits at
(i // chpad)·world·chpad + r·chpad + i % chpad of the gathered layout, which has 4·world·chpad rows.
"""
import functools

import numpy as np

from oracle import spark_als as O
from tests import ladder as LD
from tests import nnls_cases as NC

NCH = 4  # gather chunks of a sharded side (als_engine.cpp gather_chunk_count)
CASES = ("ladder", "skew", "tiny")
MODES = ("cholesky", "nnls", "explicit")
NEW_REG = 0.125  # the regParam als_set_params switches to (step 6 of the worker)
TOPK_KS = (1, 10, 64, 65, 200)
EVAL_KS = (1, 10, 64)
SUBSETS = ("shuffled", "single", "few", "unknown")
EVAL_TABLES = ("mixed", "few")
COND_CAP = 3e3  # tests/test_gpu_rating_modes.py: below it an fp32 solve keeps two decades under 1e-4

# (case, rank k, world, ALBEDO_SPLIT_CHUNK or None, mode): the launches of tests/test_gpu_shard_edges.py
LAUNCHES = [
    ("ladder", 50, 2, "256", "cholesky"),
    ("ladder", 128, 3, "256", "cholesky"),
    ("ladder", 128, 4, None, "cholesky"),
    ("ladder", 256, 3, "256", "cholesky"),
    ("ladder", 50, 3, None, "nnls"),
    ("skew", 16, 3, None, "cholesky"),
    ("skew", 128, 3, "256", "cholesky"),
    ("skew", 128, 4, None, "cholesky"),
    ("skew", 16, 3, None, "nnls"),
    ("skew", 16, 3, None, "explicit"),
    ("tiny", 3, 2, None, "cholesky"),
    ("tiny", 3, 3, None, "cholesky"),
    ("tiny", 3, 4, None, "cholesky"),
]


def launch_id(cfg):
    case, k, world, chunk, mode = cfg
    return f"{case}-k{k}-w{world}-chunk{chunk or 'default'}-{mode}"


# ---- problems --------------------------------------------------------------------------------------

def _skew_coo(seed=5):
    rng = np.random.default_rng(seed)
    n_users, n_items = 1500, 160
    uid = np.sort(rng.choice(np.arange(-40000, 90000, dtype=np.int64), n_users, replace=False)).astype(np.int32)
    iid = np.sort(rng.choice(np.arange(-900, 9000, dtype=np.int64), n_items, replace=False)).astype(np.int32)
    assert uid[0] < 0 and iid[0] < 0
    deg = rng.integers(1, 8, n_items - 1)
    assert deg.sum() < 700
    # at most 4 further ratings per user (user degrees 1..5), drawn mostly from 150 "busy" users
    room = np.full(n_users, 4)
    weight = np.ones(n_users)
    weight[rng.choice(n_users, 150, replace=False)] = 25.0
    users, items = [uid], [np.full(n_users, iid[0], np.int32)]  # the lowest item id: every user
    for t, d in enumerate(deg):
        p = weight * (room > 0)
        pick = rng.choice(n_users, int(d), replace=False, p=p / p.sum())
        room[pick] -= 1
        users.append(uid[pick])
        items.append(np.full(int(d), iid[1 + t], np.int32))
    user, item = np.concatenate(users), np.concatenate(items)
    perm = rng.permutation(user.size)
    return user[perm], item[perm]


def _tiny_coo(seed=9):
    rng = np.random.default_rng(seed)
    uid = np.sort(rng.choice(np.arange(-50, 400, dtype=np.int64), 40, replace=False)).astype(np.int32)
    iid = np.array([-7, 12, 300], np.int32)
    rows = [np.arange(30), np.arange(15, 40), np.sort(rng.choice(40, 35, replace=False))]  # degree 30 / 25 / 35
    user = np.concatenate([uid[r] for r in rows])
    item = np.concatenate([np.full(len(r), iid[t], np.int32) for t, r in enumerate(rows)])
    perm = rng.permutation(user.size)
    return user[perm], item[perm]


@functools.lru_cache(maxsize=None)
def problem(case, mode="cholesky"):
    """(user, item, rating, blocks, (implicit, alpha, reg)) of a case.  cholesky / nnls: implicit, alpha 10,
    reg 0.5, ratings in {0.25, 0.5, 1, 2, 4}; explicit: integer ratings 1..5 (`stars`-like), reg 0.1."""
    if case == "ladder":
        user, item, ideg = LD.ladder_coo()
        r = LD.ladder_ratings("stars" if mode == "explicit" else "varying", user, ideg)
    else:
        user, item = {"skew": _skew_coo, "tiny": _tiny_coo}[case]()
        rng = np.random.default_rng(17)
        r = (rng.integers(1, 6, user.size) if mode == "explicit"
             else rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], user.size)).astype(np.float32)
    params = (False, 1.0, 0.1) if mode == "explicit" else (True, 10.0, 0.5)
    for a in (user, item, r):
        a.setflags(write=False)
    return user, item, r, O.make_blocks(user, item, r), params


def side_csr(B, side):
    """(ids, ptr, col, val, src ids) of dst side 0 (users) or 1 (items)."""
    if side == 0:
        return B.user_ids, B.u_ptr, B.u_col, B.u_val, B.item_ids
    return B.item_ids, B.i_ptr, B.i_col, B.i_val, B.user_ids


@functools.lru_cache(maxsize=None)
def injected(case, k, mode):
    """(U0, V0): the factors every rank injects; unit-norm Gaussian rows, the nonneg form for NNLS."""
    B = problem(case, mode)[3]
    nonneg = mode == "nnls"
    U0 = LD.unit_rows(np.random.default_rng(1000 + k), len(B.user_ids), k, nonneg=nonneg)
    V0 = LD.unit_rows(np.random.default_rng(2000 + k), len(B.item_ids), k, nonneg=nonneg)
    U0.setflags(write=False)
    V0.setflags(write=False)
    return U0, V0


# ---- the layout, restated -----------------------------------------------------------------------------

def plan_shards(ptr, world):
    """host_math.cpp plan_shards: starts[w] = the first row whose ptr reaches ceil(total·w / world), never
    below starts[w - 1]; starts[world] = n."""
    ptr = np.asarray(ptr, np.int64)
    n, total = len(ptr) - 1, int(ptr[-1])
    starts = np.zeros(world + 1, np.int64)
    r = 0
    for w in range(1, world):
        target = (total * w + world - 1) // world
        while r < n and ptr[r] < target:
            r += 1
        starts[w] = max(starts[w - 1], r)
    starts[world] = n
    return starts


class Layout:
    """The gathered layout of one side for `world` ranks."""

    def __init__(self, ptr, world):
        self.world = world
        self.starts = plan_shards(ptr, world)
        self.n = len(ptr) - 1
        self.rows = np.diff(self.starts)
        self.maxrows = int(self.rows.max())
        self.chpad = max(1, -(-self.maxrows // NCH))
        self.prows = NCH * world * self.chpad

    def pos(self, r, i):
        cp = self.chpad
        return (i // cp) * self.world * cp + r * cp + i % cp

    def pos_inv(self, p):
        """(rank, local row) of a gathered position (the local row may lie past the rank's rows: padding)."""
        cp = self.chpad
        span = self.world * cp
        q, rem = divmod(p, span)
        return rem // cp, q * cp + rem % cp

    def owner(self, row):
        """The rank that owns dense row `row` (empty ranks own nothing)."""
        return int(np.searchsorted(self.starts, row, side="right") - 1)

    def chunk(self, row):
        return int((row - self.starts[self.owner(row)]) // self.chpad)

    def own(self, r):
        return int(self.starts[r]), int(self.starts[r + 1])

    def chunks_used(self, r):
        """Layout chunks of rank r that hold at least one real row."""
        return -(-int(self.rows[r]) // self.chpad)

    def probe_rows(self, r):
        """Dense rows of rank r at the first and last own row and on both sides of every chunk boundary."""
        lo, hi = self.own(r)
        loc = {0, hi - lo - 1}
        for q in range(1, NCH):
            loc |= {q * self.chpad - 1, q * self.chpad}
        return sorted(lo + i for i in loc if 0 <= i < hi - lo)

    def foreign_row(self, r):
        """A dense row rank r does not own (None when it owns them all)."""
        lo, hi = self.own(r)
        return hi if hi < self.n else (lo - 1 if lo > 0 else None)


@functools.lru_cache(maxsize=None)
def layout(case, side, world, mode="cholesky"):
    return Layout(side_csr(problem(case, mode)[3], side)[1], world)


def rank_slice(n, rank, world):
    """topk_host.cpp rank_slice: (per, lo, hi), per = ceil(n / world) rows dealt to each rank in order."""
    per = -(-n // world)
    lo = min(n, rank * per)
    return per, lo, min(n, lo + per)


# ---- path labels ----------------------------------------------------------------------------------------

def row_paths(deg, k, mode, chunk, light=-1):
    """The solve path of every row (tests/ladder.py path_of; NNLS: tests/nnls_cases.py nnls_path_of); with the
    degree tiers on (rank 65..128, default light limit, Cholesky) degrees 33..48 and 65..80 are named."""
    KP = LD.padded_rank(k)
    ch = LD.split_chunk(chunk or str(LD.DEFAULT_SPLIT_CHUNK))
    if mode == "nnls":
        return np.array([NC.nnls_path_of(d, KP, ch) for d in deg])
    out = []
    for d in deg:
        p = LD.path_of(d, KP, light, ch)
        if KP == 128 and light == -1:
            p = "light48" if 32 < d <= 48 else ("tier80" if 64 < d <= 80 else p)
        out.append(p)
    return np.array(out)


def path_stats(deg, paths, mode):
    """als_path_stats of a whole side: light rows, their ratings, the other rows, their ratings (tier80
    counts with the rows above the light limit)."""
    deg = np.asarray(deg)
    if mode == "nnls":
        return NC.path_stats(deg, paths)
    light = np.array([p.startswith("light") for p in paths], bool)
    return [int(light.sum()), int(deg[light].sum()), int((~light).sum()), int(deg[~light].sum())]


def row_labels(paths, lay):
    """`path / owner rank / layout chunk` per dense row."""
    return np.array([f"{p}/r{lay.owner(i)}/c{lay.chunk(i)}" for i, p in enumerate(paths)])


# ---- inputs of the top-k, evaluation and prediction calls --------------------------------------------------

def unknown_ids(ids, n):
    """n raw ids the side does not hold, on both sides of its range."""
    ids = np.asarray(ids, np.int64)
    out = [int(ids.max()) + 1 + 3 * j for j in range((n + 1) // 2)] + [int(ids.min()) - 2 - 5 * j for j in range(n // 2)]
    return np.array(out[:n], np.int32)


def subset(name, ids, world):
    """A src id subset for als_recommend.  shuffled: up to 37 known ids in random order with 3 repeated and 4
    unknown ids among them; single: one known id; few: world - 1 known ids (fewer than ranks) and one
    unknown; unknown: unknown ids only."""
    ids = np.asarray(ids, np.int32)
    rng = np.random.default_rng(len(ids) + 31 * world)
    unk = unknown_ids(ids, 4)
    if name == "shuffled":
        known = rng.choice(ids, min(len(ids), 37), replace=False)
        s = np.concatenate([known, known[:3], unk])
        return np.ascontiguousarray(s[rng.permutation(s.size)], np.int32)
    if name == "single":
        return ids[len(ids) // 2:len(ids) // 2 + 1].copy()
    if name == "few":
        return np.ascontiguousarray(np.r_[unk[:1], rng.choice(ids, min(len(ids), world - 1), replace=False)], np.int32)
    if name == "unknown":
        return unk[:3].copy()
    raise ValueError(name)


def eval_table(name, B, world):
    """(user, item, key int64) rows for als_evaluate_ndcg / als_evaluate_ranking.  mixed: up to 60 model
    users with 1..12 rows each over known and unknown items, keys in 0..5 (ties), and 5 unknown users; few:
    world - 1 model users (fewer than ranks) and 2 unknown users."""
    rng = np.random.default_rng(77 + world + len(B.user_ids))
    n_known = min(len(B.user_ids), 60) if name == "mixed" else world - 1
    known = rng.choice(B.user_ids, n_known, replace=False)
    users = np.r_[known, unknown_ids(B.user_ids, 5 if name == "mixed" else 2)]
    cat = np.r_[B.item_ids, unknown_ids(B.item_ids, 3)]
    u, i = [], []
    for x in users:
        m = min(int(rng.integers(1, 13)), len(cat))
        u.append(np.full(m, x, np.int32))
        i.append(rng.choice(cat, m, replace=False))
    u, i = np.concatenate(u), np.concatenate(i).astype(np.int32)
    key = rng.integers(0, 6, u.size).astype(np.int64)
    perm = rng.permutation(u.size)
    return np.ascontiguousarray(u[perm]), np.ascontiguousarray(i[perm]), np.ascontiguousarray(key[perm])


def predict_pairs(B):
    """(user, item) pairs for als_predict: 50 known pairs, then an unknown user, an unknown item, both."""
    rng = np.random.default_rng(5 + len(B.user_ids))
    u = rng.choice(B.user_ids, 50)
    i = rng.choice(B.item_ids, 50)
    uu, ui = unknown_ids(B.user_ids, 1)[0], unknown_ids(B.item_ids, 1)[0]
    u = np.r_[u, uu, B.user_ids[0], uu].astype(np.int32)
    i = np.r_[i, B.item_ids[0], ui, ui].astype(np.int32)
    return np.ascontiguousarray(u), np.ascontiguousarray(i)

"""Shared inputs of the NDCG edge tests (tests/test_gpu_ingest_eval_edges.py on the GPU, the
precondition tests of tests/test_oracle.py on the CPU) for albedo_amd/csrc/eval.hip behind
als_evaluate_ndcg.

A case is a model (uid, uf, iid, itf: raw ids in shuffled order and fp32 factors, rank 24, for
als_model_create; no fit) and an evaluation set (users int32, items int32, keys int64) in the order the
engine receives it.  reference() is the expected answer: the oracle's top-k lists, the oracle's
actual lists and O.ndcg_at per user.  actual_lists() is a second, vectorised statement of the
actual-list rule, used where the oracle's Python loop would be slow.

  lengths     users with exactly 1 .. 1000 actual rows around k and around the 64-row rounds of the
              streaming sort (ev_actual_kernel); variants: equal keys within a user (item order
              alone), the k largest keys in the user's last 64 input rows
  keys        INT64_MIN, INT64_MAX, negative keys, keys that differ by 1 above 2^53 at the k-th place
  bag         on catalogues of any sign (all negative; mixed; with -1, INT32_MIN, INT32_MAX) and of 5
              and 29 items: users whose actual items are unknown to the model, users with one item
              repeated, the (INT64_MIN, INT32_MAX) row that equals the kernel's empty slot, unknown
              users below, between and above the model's ids
"""
import functools

import numpy as np

from oracle import spark_als as O

RANK = 24
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
LENGTHS = [1, 29, 30, 31, 63, 64, 65, 127, 128, 129, 200, 1000]
LENGTH_VARIANTS = ["random", "ties", "last64"]
CATALOGUES = ["negative", "mixed", "extreme", "five", "twentynine"]
MAP_CAP = 16384 * 256                 # id_front.h front_grid: at most 16384 blocks of 256 threads
N_PAST_CAP = MAP_CAP + 257
BIG = 1 << 60                         # BIG and BIG + 1 are one float64
PASS_ROWS = 1 << 16                   # the smallest ALBEDO_TOPK_PASS the engine accepts
PASS_USERS = 2 * PASS_ROWS + 9001     # evaluated users of the pass case: three passes


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def catalogue(kind, rng):
    """Distinct raw item ids, shuffled."""
    if kind == "negative":
        ids = -1 - rng.choice(50000, 300, replace=False)
    elif kind == "mixed":
        ids = rng.choice(100000, 300, replace=False) - 50000
    elif kind == "extreme":
        ids = np.r_[rng.integers(I32_MIN, I32_MAX, 293, endpoint=True),
                    [-1, 0, 1, I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX]]
        ids = np.unique(ids)
    elif kind == "five":
        ids = np.array([-9, -1, 4, I32_MAX, 100])
    elif kind == "twentynine":
        ids = rng.choice(2000, 29, replace=False) - 1000
    else:
        raise ValueError(kind)
    return rng.permutation(ids).astype(np.int32)


def model(rng, uid, kind):
    """(uid, uf, iid, itf) with small Gaussian factors of rank RANK over catalogue `kind`."""
    iid = catalogue(kind, rng)
    uid = np.asarray(uid).astype(np.int32)
    return (uid, _f32(0.3 * rng.standard_normal((uid.size, RANK))), iid,
            _f32(0.3 * rng.standard_normal((iid.size, RANK))))


def _interleave(rng, per_user):
    """One evaluation set from per-user (user, items, keys): the users' rows are interleaved at
    random, each user's rows keep their order."""
    n = sum(len(it) for _, it, _ in per_user)
    slots = rng.permutation(n)
    users, items, keys = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int64)
    s = 0
    for u, it, ky in per_user:
        at = np.sort(slots[s:s + len(it)])
        users[at], items[at], keys[at] = u, it, ky
        s += len(it)
    return users, items, keys


def lengths(variant, k=30):
    """Users 1000 + length with exactly `length` rows each over the `mixed` catalogue (40 further
    users in the model have none)."""
    rng = np.random.default_rng(9000 + LENGTH_VARIANTS.index(variant))
    m = model(rng, np.r_[1000 + np.array(LENGTHS), -500 + 7 * np.arange(40)], "mixed")
    iid = m[2]
    per_user = []
    for n in LENGTHS:
        it = iid[rng.integers(0, iid.size, n)]
        if variant == "random":
            ky = rng.integers(-(1 << 40), 1 << 40, n) // (1 << 33) * (1 << 33)  # ~256 values: ties
        elif variant == "ties":
            ky = np.full(n, 1_500_000_000_000_000 + n)
        elif variant == "last64":  # distinct keys, the k largest at random places of the last 64 rows
            ky = rng.permutation(n).astype(np.int64) * 1000
            order = np.argsort(-ky, kind="stable")
            tail = np.arange(max(0, n - 64), n)
            top = order[:min(k, n)]
            dest = rng.choice(tail, top.size, replace=False)
            rest_src = np.setdiff1d(np.arange(n), top)
            rest_dst = np.setdiff1d(np.arange(n), dest)
            new = np.empty(n, np.int64)
            new[dest] = ky[top]
            new[rest_dst] = ky[rest_src]
            ky = new
        else:
            raise ValueError(variant)
        per_user.append((1000 + n, it, ky))
    return m, _interleave(rng, per_user)


def keys(k=30):
    """40 users of k + 20 rows whose k-th and (k+1)-th keys are BIG + 1 and BIG with the larger item id
    on the larger key (a float64 order swaps the two); users with INT64_MIN / INT64_MAX / negative
    keys; the catalogue is `extreme`."""
    rng = np.random.default_rng(9100)
    m = model(rng, 50 + 3 * np.arange(60), "extreme")
    uid, iid = m[0], m[2]
    per_user = []
    for u in uid[:40]:
        it = rng.choice(iid, k + 20, replace=False)
        a, b = max(it[k - 1], it[k]), min(it[k - 1], it[k])
        it[k - 1], it[k] = a, b
        ky = np.r_[BIG + 1024 * (1 + rng.permutation(k - 1)), BIG + 1, BIG, rng.integers(-BIG, BIG, 19)].astype(np.int64)
        p = rng.permutation(it.size)
        per_user.append((u, it[p], ky[p]))
    ext = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX, -BIG - 1, -BIG], np.int64)
    for j, u in enumerate(uid[40:52]):
        n = [5, 9, 29, 30, 31, 40, 64, 65, 100, 128, 129, 150][j]
        ky = np.r_[ext, rng.integers(I64_MIN, I64_MAX, max(n - ext.size, 0), endpoint=True)][:n].astype(np.int64)
        p = rng.permutation(n)
        per_user.append((u, iid[rng.integers(0, iid.size, n)], ky[p]))
    return m, _interleave(rng, per_user)


def bag(kind, n_model_users=80):
    """The mixed bag on catalogue `kind`; model users 10, 13, 16, ... (the evaluated ones among them
    are listed by bag_roles)."""
    rng = np.random.default_rng(9200 + CATALOGUES.index(kind) + n_model_users)
    m = model(rng, 10 + 3 * np.arange(n_model_users), kind)
    uid, iid = m[0], m[2]
    unknown_items = np.setdiff1d(np.r_[iid.astype(np.int64) + 1, [-2, 2, I32_MIN + 2, I32_MAX - 2]], iid)
    unknown_items = np.setdiff1d(np.r_[unknown_items[unknown_items <= I32_MAX], 1009 * np.arange(-20, 20) + 3], iid)
    per_user = []
    roles = bag_roles(n_model_users)
    for u in roles["ordinary"]:          # catalogue items and unknown ones, some twice
        n = int(rng.integers(1, 101))
        it = np.where(rng.random(n) < 0.7, iid[rng.integers(0, iid.size, n)],
                      unknown_items[rng.integers(0, unknown_items.size, n)])
        per_user.append((u, it, rng.integers(0, 50, n)))
    for u in roles["unknown_items"]:
        n = int(rng.integers(1, 90))
        per_user.append((u, unknown_items[rng.integers(0, unknown_items.size, n)], rng.integers(0, 50, n)))
    for u, n in zip(roles["one_item"], [1, 5, 40, 100, 130]):
        per_user.append((u, np.full(n, iid[rng.integers(0, iid.size)]), rng.integers(-5, 5, n)))
    for u, n in zip(roles["sentinel"], [1, 7, 30, 31, 64, 100]):  # (INT64_MIN, INT32_MAX) = the empty slot
        it = np.r_[I32_MAX, I32_MAX, iid[rng.integers(0, iid.size, n)]][:n]
        ky = np.r_[I64_MIN, I64_MIN, rng.integers(I64_MIN, I64_MIN + 3, n)][:n]
        p = rng.permutation(n)
        per_user.append((u, it[p], ky[p]))
    for u in roles["many_labels"]:       # 35 distinct items: |labSet| = k although the catalogue may be smaller
        it = rng.permutation(iid)[:20]
        it = np.r_[it, rng.choice(unknown_items, 35 - it.size, replace=False)]
        per_user.append((u, rng.permutation(it), rng.permutation(35)))
    for u in roles["unknown_users"]:
        n = int(rng.integers(1, 70))
        per_user.append((u, iid[rng.integers(0, iid.size, n)], rng.integers(0, 50, n)))
    return m, _interleave(rng, per_user)


def bag_roles(n_model_users=80):
    """The users of bag()'s evaluation set by role; unknown users lie below, between and above the
    model's ids 10, 13, ..."""
    uid = 10 + 3 * np.arange(n_model_users)
    top = int(uid[-1])
    if n_model_users == 1:
        return {"ordinary": [10], "unknown_items": [], "one_item": [], "sentinel": [], "many_labels": [],
                "unknown_users": [I32_MIN, -3, 9, 11, 12, I32_MAX]}
    return {"ordinary": uid[0:40].tolist(), "unknown_items": uid[40:46].tolist(), "one_item": uid[46:51].tolist(),
            "sentinel": uid[51:57].tolist(), "many_labels": uid[57:60].tolist(),
            "unknown_users": [I32_MIN, -3, 9, 11, 12, top - 1, top + 1, I32_MAX]}


def only_unknown_users():
    m, (users, items, keys_) = bag("mixed")
    known = np.isin(users, m[0])
    return m, (users[~known], items[~known], keys_[~known])


def past_cap():
    """N_PAST_CAP rows over 36 of the model's 50 users (and 3 unknown ones), full-range keys."""
    rng = np.random.default_rng(9300)
    m = model(rng, 7 * np.arange(50) - 100, "mixed")
    who = np.r_[m[0][:36], [-101, 1, 400]].astype(np.int32)
    users = who[rng.integers(0, who.size, N_PAST_CAP)]
    items = m[2][rng.integers(0, m[2].size, N_PAST_CAP)]
    return m, (users, items, rng.integers(I64_MIN, I64_MAX, N_PAST_CAP, endpoint=True))


def passes():
    """lengths("random") (same 12 users, same rows, same catalogue) inside a model of PASS_USERS + 50
    users, PASS_USERS of which are evaluated too with 1 to 3 rows each: with ALBEDO_TOPK_PASS =
    PASS_ROWS the evaluated users take three passes, and PASS_ROWS - 6 of them have ids below the 12
    users of lengths, so the first pass ends between the users of 64 and 65 rows."""
    rng = np.random.default_rng(9400)
    (luid, _, liid, _), (lu, li, lk) = lengths("random")
    low = -3 * np.arange(1, PASS_ROWS - 5)
    high = 3000 + 3 * np.arange(PASS_USERS - low.size + 38)
    m = model(np.random.default_rng(9000), np.r_[luid[:12], low, high], "mixed")  # 9000: lengths' catalogue
    assert np.array_equal(m[2], liid)
    ev = np.repeat(np.r_[low, high[:-38]], rng.integers(1, 4, PASS_USERS))
    users = np.r_[lu, ev].astype(np.int32)
    items = np.r_[li, m[2][rng.integers(0, m[2].size, ev.size)]]
    keys_ = np.r_[lk, rng.integers(0, 1000, ev.size)]
    p = rng.permutation(users.size)
    return m, (users[p], items[p], keys_[p])


GENERATORS = {"lengths": lengths, "keys": keys, "bag": bag, "only_unknown_users": only_unknown_users,
              "past_cap": past_cap, "passes": passes}
# (generator, args) of the cases small enough for the oracle's Python loops
SMALL_CASES = ([("lengths", (v,)) for v in LENGTH_VARIANTS] + [("keys", ())] + [("bag", (c,)) for c in CATALOGUES]
               + [("bag", ("mixed", 1)), ("only_unknown_users", ())])


def case_id(c):
    return c[0] + "".join(f"-{a}" for a in c[1])


@functools.lru_cache(maxsize=None)
def case(name, *args):
    """(model, evaluation set) of GENERATORS[name](*args), read-only and cached."""
    m, ev = GENERATORS[name](*args)
    for a in m + ev:
        a.setflags(write=False)
    return m, ev


def actual_lists(users, items, keys_, k):
    """{user: the first k items of its rows in (key desc, item asc) order}: the actual-list rule
    (rank() <= k, collect_list, slice(0, k)) restated as one lexsort; integer keys only."""
    users, items = np.asarray(users), np.asarray(items)
    keys_ = np.asarray(keys_)
    assert keys_.dtype.kind == "i"
    order = np.lexsort((items, ~keys_.astype(np.int64), users))
    u_s = users[order]
    start = np.r_[0, 1 + np.nonzero(u_s[1:] != u_s[:-1])[0]] if u_s.size else np.zeros(0, np.int64)
    end = np.r_[start[1:], u_s.size]
    return {int(u_s[a]): [int(x) for x in items[order[a:min(b, a + k)]]] for a, b in zip(start, end)}


def predicted_lists(m, users, k):
    """{user: the oracle's top-k item ids} for the model users among `users`, ascending; every list
    holds min(k, catalogue) ids, whatever their sign."""
    uid, uf, iid, itf = m
    known = np.intersect1d(np.unique(users), uid)
    row = {int(u): r for r, u in enumerate(uid)}
    ids, _ = O.recommend_for_all(known, uf[[row[int(u)] for u in known]], iid, itf, k)
    n = min(k, iid.size)
    return known.astype(np.int32), {int(u): [int(x) for x in ids[r, :n]] for r, u in enumerate(known)}


@functools.lru_cache(maxsize=None)
def reference(name, args, k, vectorised=False):
    """(evaluated user ids ascending, per-user ndcgAt(k), their mean) of a case from the oracle:
    O.recommend_for_all, O.into_user_items (vectorised: actual_lists) and O.ndcg_at."""
    m, (users, items, keys_) = case(name, *args)
    known, pred = predicted_lists(m, users, k)
    actual = (actual_lists if vectorised else O.into_user_items)(users, items, keys_, k)
    vals = np.array([O.ndcg_at([(pred[int(u)][:k], actual[int(u)][:k])], k) for u in known], np.float64)
    mean = O.evaluate_ndcg(pred, actual, k) if known.size else float("nan")
    vals.setflags(write=False)
    return known, vals, mean

"""Shared inputs of the ingest edge tests (tests/test_gpu_ingest_eval_edges.py on the GPU, the
precondition tests of tests/test_oracle.py on the CPU): the role tests/topk_cases.py has for top-k.

Every generator is pure numpy and seeded and returns the COO (user int32, item int32, rating fp32) in
shuffled order, the way als_set_ratings receives it.  Each case aims at one place where
albedo_amd/csrc/ingest.hip (remap_ids, build_csr) is right only because of a detail that tame positive
ids without duplicates never reach:

  extreme_ids     INT32_MIN .. INT32_MAX on both sides, ids that differ only in the top bit or only in
                  bit 0: the signed order of the id tables (flip_keys_kernel)
  duplicates      one (user, item) pair 2, 3 and 64 times with different ratings (one pair +r / -r)
                  inside rows of degree 8, 16, 17, 64 and 65, in both orientations: every copy is a
                  rating of its own (Spark sums nothing), and the radix sort's key holds no rating
  degenerate      n = 1, one row on one side, n_dst = 2^8 - 1, 2^8, 2^8 + 1 (build_csr sorts
                  32 + bits_for(n_dst) bits)
  sizes           n around one 256-thread block and just past the 8192-block launch cap of the
                  grid-stride kernels
"""
import functools

import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
EXTREME_IDS = [I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX]
TOP_BIT_PAIRS = [(0x12345678, 0x12345678 - (1 << 31)), (5, 5 - (1 << 31)), (0x7FFFFFFE - 77, -79)]
BIT0_PAIRS = [(1000, 1001), (-1000, -999), (0x40000000, 0x40000001), (-0x40000000, -0x40000000 + 1)]
DUP_DEGREES = [8, 16, 17, 64, 65]      # rows that hold a duplicated pair: a kernel switch on either side
DUP_COPIES = [2, 3, 64]                # copies of the duplicated pair (64 only where the row holds them)
GRID_CAP = 8192 * 256                  # ingest.hip grid_for: at most 8192 blocks of 256 threads
N_PAST_CAP = GRID_CAP + 257
RATINGS = np.array([0.25, 0.5, 1.0, 2.0, 4.0], np.float32)


def _coo(rng, user, item, rating):
    p = rng.permutation(len(user))
    out = (np.asarray(user, np.int64)[p].astype(np.int32), np.asarray(item, np.int64)[p].astype(np.int32),
           np.asarray(rating, np.float32)[p])
    assert np.array_equal(out[0], np.asarray(user, np.int64)[p]), "user ids outside int32"
    assert np.array_equal(out[1], np.asarray(item, np.int64)[p]), "item ids outside int32"
    return out


def special_ids():
    """The ids extreme_ids puts on both sides, besides its random ones."""
    return sorted(set(EXTREME_IDS) | {x for p in TOP_BIT_PAIRS + BIT0_PAIRS for x in p})


def extreme_ids():
    """~200 ids per side (the special ones and draws from the whole int32 range), ~3600 distinct
    pairs with positive ratings, so that every row of an implicit half-sweep is well posed."""
    rng = np.random.default_rng(101)
    sp = np.array(special_ids(), np.int64)
    sides = []
    for _ in range(2):
        more = rng.integers(I32_MIN, I32_MAX, 180, endpoint=True)
        sides.append(np.unique(np.r_[sp, more]))
    uid, iid = sides
    cell = rng.choice(uid.size * iid.size, 3600, replace=False)
    u, i = cell // iid.size, cell % iid.size
    # every id of either side appears at least once
    u = np.r_[u, np.arange(uid.size), rng.integers(0, uid.size, iid.size)]
    i = np.r_[i, rng.integers(0, iid.size, uid.size), np.arange(iid.size)]
    return _coo(rng, uid[u], iid[i], rng.choice(RATINGS, u.size))


def dup_rows():
    """[(degree, copies)] of the rows of `duplicates` that hold a duplicated pair, per orientation."""
    return [(d, c) for d in DUP_DEGREES for c in DUP_COPIES if c < d or (c == d == 64)]


def dup_ratings(copies):
    """The ratings of a pair's copies: all different; two copies are +r and -r."""
    if copies == 2:
        return np.array([2.5, -2.5], np.float32)
    return (0.125 * (1 + np.arange(copies))).astype(np.float32)


def duplicates():
    """A background of 250 x 250 pool ids with ~2500 distinct pairs, and for each orientation one row
    per dup_rows() entry (ids 700000 + 1000 * degree + copies on the dst side): `copies` copies of one
    pair and degree - copies further distinct src ids of the other side's pool.  The 64 copies of
    degree 64 are the whole row."""
    rng = np.random.default_rng(202)
    pool = [np.sort(rng.choice(np.arange(-40000, 90000), 250, replace=False)) for _ in range(2)]
    cell = rng.choice(250 * 250, 2500, replace=False)
    user, item = [pool[0][cell // 250]], [pool[1][cell % 250]]
    rating = [rng.choice(RATINGS, cell.size)]
    for side in (0, 1):  # side of the dst rows; the src ids come from the other side's pool
        for d, c in dup_rows():
            dst = 700000 + 1000 * d + c
            src = rng.choice(pool[1 - side], d - c + 1, replace=False)
            src = np.r_[np.repeat(src[:1], c), src[1:]]
            r = np.r_[dup_ratings(c), rng.choice(RATINGS, d - c)]
            dsts = np.full(d, dst)
            user.append(dsts if side == 0 else src)
            item.append(src if side == 0 else dsts)
            rating.append(r)
    return _coo(rng, np.concatenate(user), np.concatenate(item), np.concatenate(rating))


def merge_duplicates(user, item, rating):
    """The COO with the copies of a pair summed into one rating (what a de-duplicating ingest would
    build): the wrong oracle of the precondition test."""
    key = (user.astype(np.int64) << 32) | (item.astype(np.int64) & 0xFFFFFFFF)
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    r = np.zeros(uniq.size, np.float64)
    np.add.at(r, inv, rating.astype(np.float64))
    return user[first], item[first], r.astype(np.float32)


def single():
    return (np.array([-7], np.int32), np.array([I32_MAX], np.int32), np.array([3.0], np.float32))


def one_user(n_items=300):
    rng = np.random.default_rng(303)
    item = rng.choice(np.arange(-5000, 5000), n_items, replace=False)
    return _coo(rng, np.full(n_items, -12345), item, rng.choice(RATINGS, n_items))


def one_item(n_users=300):
    rng = np.random.default_rng(304)
    user = rng.choice(np.arange(-5000, 5000), n_users, replace=False)
    return _coo(rng, user, np.full(n_users, 77), rng.choice(RATINGS, n_users))


def one_user_repeats():
    """One unique id on the user side, 40 on the other, 300 ratings: every pair about 7 times."""
    rng = np.random.default_rng(305)
    item = rng.choice(np.arange(-5000, 5000), 40, replace=False)
    return _coo(rng, np.full(300, I32_MIN), item[rng.integers(0, 40, 300)], rng.choice(RATINGS, 300))


def square(v):
    """v ids on both sides, 4 v ratings, every id present: the highest dense index is v - 1."""
    rng = np.random.default_rng(400 + v)
    uid = rng.choice(np.arange(-3 * v, 3 * v), v, replace=False)
    iid = rng.choice(np.arange(-3 * v, 3 * v), v, replace=False)
    u = np.r_[np.arange(v), rng.integers(0, v, 3 * v)]
    i = np.r_[rng.permutation(v), rng.integers(0, v, 3 * v)]
    return _coo(rng, uid[u], iid[i], rng.choice(RATINGS, 4 * v))


def sized(n, n_users=50, n_items=60):
    """n ratings over n_users x n_items ids drawn with replacement (so pairs repeat)."""
    rng = np.random.default_rng(500 + n % 1000 + n_users)
    uid = rng.choice(np.arange(-40 * n_users, 40 * n_users), n_users, replace=False)
    iid = rng.choice(np.arange(-40 * n_items, 40 * n_items), n_items, replace=False)
    return (uid[rng.integers(0, n_users, n)].astype(np.int32), iid[rng.integers(0, n_items, n)].astype(np.int32),
            rng.choice(RATINGS, n))


def past_cap():
    return sized(N_PAST_CAP, 3000, 2500)


GENERATORS = {"extreme_ids": extreme_ids, "duplicates": duplicates, "single": single, "one_user": one_user,
              "one_item": one_item, "one_user_repeats": one_user_repeats, "square": square, "sized": sized,
              "past_cap": past_cap}
# (generator, args) of every case but the one past the launch cap
SMALL_CASES = ([("extreme_ids", ()), ("duplicates", ()), ("single", ()), ("one_user", ()), ("one_item", ()),
                ("one_user_repeats", ())] + [("square", (v,)) for v in (255, 256, 257)]
               + [("sized", (n,)) for n in (255, 256, 257)])


def case_id(c):
    return c[0] + "".join(f"-{a}" for a in c[1])


@functools.lru_cache(maxsize=None)
def case(name, *args):
    """(user, item, rating) of GENERATORS[name](*args), read-only and cached."""
    out = GENERATORS[name](*args)
    for a in out:
        a.setflags(write=False)
    return out

"""Shared pieces of the rating-mode parity tests (tests/test_gpu_rating_modes.py on the GPU,
tests/test_oracle.py on the CPU): the degree-ladder data set, the rating modes, a test-side
restatement of the engine's path choice, and the per-row failure report.

The ladder puts one item row on each side of every degree at which the engine changes kernel
(light16 pairs <= 8, light16 <= 16, D = 32 / 64 / 96, the wave or heavy kernel above the light limit,
split-K above the chunk length), twice with different user draws; the user degrees (about 1..20)
cover light16 pairs, light16 and D = 32 on the return half.
"""
import os

import numpy as np

LADDER = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257, 511, 512, 513]
# item rows of these degrees hold only ratings <= 0 in mode `mixed` (npos = 0): one each on light16
# pairs, D = 32, the wave / heavy kernel (or D = 96) and split-K at a chunk of 256
NONPOS_DEGREES = (2, 17, 65, 257)

# name -> (implicit, alpha, reg)
MODES = {
    "varying": (True, 10.0, 0.5),
    "signed_uniform": (True, 20.0, 0.5),
    "mixed": (True, 10.0, 0.5),
    "stars": (False, 1.0, 0.1),
    "stars_signed": (False, 1.0, 0.1),
}

# (rank, light_max_degree, ALBEDO_SPLIT_CHUNK)
CONFIGS = [(50, -1, None), (50, 0, None), (50, -1, "256"),
           (100, -1, None), (100, 0, None),
           (128, -1, None), (128, 0, None), (128, 96, None), (128, -1, "256"),
           (200, -1, None), (200, 0, "256"),
           (256, -1, None), (256, 0, None), (256, -1, "256")]

DEFAULT_SPLIT_CHUNK = 8192


def config_id(cfg):
    k, light, chunk = cfg
    return f"k{k}-light{'default' if light < 0 else light}-chunk{chunk or 'default'}"


def padded_rank(k):
    return 64 if k <= 64 else (128 if k <= 128 else 256)


def light_limit(KP, light):
    """sweep_host.cpp light_limit: rows of degree <= this take the push-through (d x d) solve."""
    if light >= 0:
        return min(light, 96 if KP == 128 else 64)
    return 64 if KP >= 128 else 32


def split_chunk(chunk=None):
    """sweep_host.cpp split_chunk_len for an ALBEDO_SPLIT_CHUNK value (None: the environment's)."""
    if chunk is None:
        chunk = os.environ.get("ALBEDO_SPLIT_CHUNK")
    return max(0, int(chunk)) if chunk else DEFAULT_SPLIT_CHUNK


def path_of(degree, KP, light, chunk):
    """The Cholesky solve path of a row (sweep_host.cpp light_limit / bucket_of / rank_layout's split
    lists); chunk is the split-K chunk length in ratings (0: no split)."""
    d = int(degree)
    if d <= light_limit(KP, light):
        if d <= 8:
            return "light16-pair"
        if d <= 16:
            return "light16"
        if d <= 32:
            return "light32"
        return "light64" if d <= 64 else "light96"
    if chunk > 0 and d > chunk:
        return "split"
    return "wave" if KP <= 128 else "heavy"


def expected_paths(KP, light, chunk, max_degree):
    """The paths a configuration is meant to reach with row degrees 1..max_degree."""
    lim = min(light_limit(KP, light), max_degree)
    out = [name for above, name in ((0, "light16-pair"), (8, "light16"), (16, "light32"), (32, "light64"),
                                    (64, "light96")) if lim > above]
    if max_degree > lim:
        out.append("wave" if KP <= 128 else "heavy")
    if 0 < chunk < max_degree:
        out.append("split")
    return out


def ladder_coo(seed=7):
    """(user, item, item_of_entry_degree): the shuffled COO of the doubled ladder over ~700 users with
    sparse raw ids, and per entry the degree of its item row."""
    rng = np.random.default_rng(seed)
    n_users = 700
    uid = np.sort(rng.choice(np.arange(3, 90000, dtype=np.int64), n_users, replace=False)).astype(np.int32)
    users, items, degs = [], [], []
    for t, d in enumerate(LADDER + LADDER):
        users.append(uid[rng.choice(n_users, d, replace=False)])
        items.append(np.full(d, 1000 + 37 * t, np.int32))
        degs.append(np.full(d, d, np.int64))
    user, item, deg = np.concatenate(users), np.concatenate(items), np.concatenate(degs)
    perm = rng.permutation(user.size)
    return user[perm], item[perm], deg[perm]


def ladder_ratings(mode, user, item_deg, seed=11):
    """The ratings of `mode` for the ladder COO.

    Implicit modes with ratings <= 0: a user without a single positive rating has lambda·n = 0, and
    its system is then the Gram of the ~50 item factors alone, which is singular at every rank used
    here (Spark's dppsv fails on it too).  Such rows are covered on the item half, whose Gram comes
    from ~700 user factors; here every user keeps one positive rating: the first entry of such a user
    outside the all-non-positive item rows is set to |r| (or to 1 when it was 0).  Asserted below."""
    rng = np.random.default_rng(seed)
    n = user.size
    if mode == "varying":
        r = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], n)
    elif mode == "signed_uniform":
        r = np.where(rng.random(n) < 0.30, -2.0, 2.0)
    elif mode == "mixed":
        r = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], n)
        r[rng.random(n) < 0.15] = 0.0
        r = np.where(rng.random(n) < 0.15, -r, r) + 0.0  # + 0.0: no negative zeros
        forced = np.isin(item_deg, NONPOS_DEGREES)
        r[forced] = -np.abs(r[forced]) + 0.0
    elif mode == "stars":
        r = rng.integers(1, 6, n).astype(np.float64)
    elif mode == "stars_signed":
        r = rng.integers(1, 6, n).astype(np.float64)
        r = np.where(rng.random(n) < 0.25, -r, r)
        r[rng.random(n) < 0.125] = 0.0
    else:
        raise ValueError(mode)
    if MODES[mode][0] and mode != "varying":
        free = ~np.isin(item_deg, NONPOS_DEGREES) if mode == "mixed" else np.ones(n, bool)
        has_pos = np.isin(user, user[r > 0])
        for u in np.unique(user[~has_pos]):
            e = np.nonzero((user == u) & free)[0]
            assert e.size > 0, f"user {u} rates only all-non-positive item rows: choose another seed"
            r[e[0]] = abs(r[e[0]]) if r[e[0]] != 0 else 1.0
        assert np.isin(user, user[r > 0]).all()
    return r.astype(np.float32)


def unit_rows(rng, n, k, nonneg=False):
    """Unit-norm Gaussian rows in fp32; nonneg: |Gaussian| with every 5th column negated (NNLS tests)."""
    F = rng.standard_normal((n, k))
    if nonneg:
        F = np.abs(F)
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    if nonneg:
        F[:, ::5] *= -1.0
    return F.astype(np.float32)


def row_errors(got, ref, global_scale=False):
    """Per row max|x - ref| / max|ref|; a row whose reference is all zero scores 0 when it is exactly
    zero and inf otherwise.  global_scale: max|ref| over all rows instead of the row's own (the
    largest row error is then the whole-matrix relative error)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    num = np.max(np.abs(got - ref), axis=1)
    den = np.full(num.shape, np.max(np.abs(ref))) if global_scale else np.max(np.abs(ref), axis=1)
    err = num / np.where(den > 0, den, 1.0)
    return np.where(den > 0, err, np.where(num == 0, 0.0, np.inf))


def assert_rows(got, ref, ids, deg, paths, tol, what, tmp_path, global_scale=False):
    """Every row of `got` within `tol` of `ref` (row_errors); rows whose reference is all zero must
    be exactly zero (unless global_scale).  On failure the message names the failing rows' count and, for the 5 worst, raw
    id, degree, path label and error, and got / ref / ids / degrees of the failing rows are saved
    under tmp_path.  Returns the worst error."""
    ids, deg, paths = np.asarray(ids), np.asarray(deg), np.asarray(paths)
    err = row_errors(got, ref, global_scale)
    err = np.where(np.isfinite(np.asarray(got, np.float64)).all(axis=1), err, np.inf)
    bad = np.nonzero(~(err < tol))[0]
    if bad.size:
        worst = bad[np.argsort(-err[bad], kind="stable")[:5]]
        name = "".join(ch if ch.isalnum() else "_" for ch in what)
        out = os.path.join(str(tmp_path), f"failing_rows_{name}.npz")
        np.savez(out, got=np.asarray(got)[bad], ref=np.asarray(ref)[bad], ids=ids[bad], deg=deg[bad],
                 paths=paths[bad], err=err[bad])
        by_path = {p: int(np.sum(paths[bad] == p)) for p in sorted(set(paths[bad].tolist()))}
        lines = [f"  id {int(ids[r])} degree {int(deg[r])} path {paths[r]} err {err[r]:.3e}" for r in worst]
        raise AssertionError(f"{what}: {bad.size} of {err.size} rows fail tol {tol:g} (by path {by_path}); worst:\n"
                             + "\n".join(lines) + f"\n  failing rows saved to {out}")
    return float(err.max()) if err.size else 0.0

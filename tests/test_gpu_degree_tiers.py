"""Degree tiers at padded rank 128: solve_light_kernel<128, 48> for rows of degree 33..48 and
solve_light_kernel<128, 80> for rows of degree 65..80 (sweep_host.cpp bucket_of / degree_tiers_on).

Data: about 400 users x 400 items.  The first rows of either side are ladder rows whose degrees sit on
both sides of every tier edge (31 .. 129, two rows each) plus one row each of degree 40 and 72, which in
mode `mixed` hold no positive rating; a ladder row draws its entries from the other side's pool rows
(degree about 8), so both halves see the whole ladder.  Either half is solved from injected unit-norm
src factors, so the two halves are independent experiments with one oracle reference each.

Modes: `unit` implicit, every rating 1 (one confidence: the pre-split build of the wave kernel);
`mixed` implicit with zeros and negatives (tests/ladder.py); `stars` explicit ratings 1..5.

Tolerance: the one of the ladder tests for the D = 64 / D = 96 paths (tests/test_gpu_rating_modes.py):
every row max|x - x64| / max|x64| < 1e-4 against the fp64 oracle half-sweep, rows without a positive
rating exactly 0.  Tier rows against the tiers-off result: both are within 1e-4 of the same fp64 row,
and the bound asked of their difference is that same 1e-4.
"""
import functools

import numpy as np
import pytest

from oracle import spark_als as O
from tests import ladder as LD
from tests.test_gpu_parity import Ctx

pytestmark = pytest.mark.gpu

TOL = 1e-4
DEGREES = [31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 79, 80, 81, 95, 96, 97, 128, 129]
NONPOS_DEGREES = (40, 72)  # one row each per side; mode `mixed`: no positive rating
N_SIDE = 400
# name -> (implicit, alpha, reg)
MODES = {"unit": (True, 40.0, 0.5), "mixed": LD.MODES["mixed"], "stars": LD.MODES["stars"]}
RANKS = (128, 100)  # 100: kreal < KP = 128


def tier_of(d):
    """The tier a degree belongs to with the tiers on ("" outside both)."""
    return "L48" if 33 <= d <= 48 else ("M80" if 65 <= d <= 80 else "")


def label_of(d):
    return tier_of(d) or LD.path_of(d, 128, -1, LD.DEFAULT_SPLIT_CHUNK)


@functools.lru_cache(maxsize=None)
def _coo():
    """(user, item, forced): COO with sparse raw ids; forced marks the entries of the degree-40 / 72 rows."""
    rng = np.random.default_rng(31)
    uid = np.sort(rng.choice(np.arange(5, 70000, dtype=np.int64), N_SIDE, replace=False)).astype(np.int32)
    iid = np.sort(rng.choice(np.arange(9, 50000, dtype=np.int64), N_SIDE, replace=False)).astype(np.int32)
    ladder = DEGREES + DEGREES + list(NONPOS_DEGREES)
    nl = len(ladder)
    users, items, forced = [], [], []
    for t, d in enumerate(ladder):  # ladder item t: d pool users; ladder user t: d pool items
        users.append(uid[nl + rng.choice(N_SIDE - nl, d, replace=False)])
        items.append(np.full(d, iid[t], np.int32))
        forced.append(np.full(d, t >= 2 * len(DEGREES)))
        users.append(np.full(d, uid[t], np.int32))
        items.append(iid[nl + rng.choice(N_SIDE - nl, d, replace=False)])
        forced.append(np.full(d, t >= 2 * len(DEGREES)))
    user, item, forced = np.concatenate(users), np.concatenate(items), np.concatenate(forced)
    perm = rng.permutation(user.size)
    return user[perm], item[perm], forced[perm]


@functools.lru_cache(maxsize=None)
def _data(mode):
    user, item, forced = _coo()
    rng = np.random.default_rng(17)
    n = user.size
    if mode == "unit":
        r = np.ones(n)
    elif mode == "mixed":
        r = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], n)
        r[rng.random(n) < 0.15] = 0.0
        r = np.where(rng.random(n) < 0.15, -r, r) + 0.0  # + 0.0: no negative zeros
        r[forced] = -np.abs(r[forced]) + 0.0
    else:
        r = rng.integers(1, 6, n).astype(np.float64)
    r = r.astype(np.float32)
    return user, item, r, O.make_blocks(user, item, r)


@functools.lru_cache(maxsize=None)
def _src(k, n, seed):
    F = LD.unit_rows(np.random.default_rng(seed), n, k)
    F.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def _ref(mode, k, side):
    """The oracle's half-sweep of dst `side` from the injected src factors, computed once."""
    implicit, alpha, reg = MODES[mode]
    B = _data(mode)[3]
    if side == 1:
        X = O.half_sweep(_src(k, len(B.user_ids), k), B.i_ptr, B.i_col, B.i_val, reg=reg, alpha=alpha, implicit=implicit)
    else:
        X = O.half_sweep(_src(k, len(B.item_ids), k + 1), B.u_ptr, B.u_col, B.u_val, reg=reg, alpha=alpha, implicit=implicit)
    X.setflags(write=False)
    return X


def _ctx(gpu_lib, monkeypatch, mode, k, tiers, light=-1):
    """A context with the ratings of `mode`; ALBEDO_DEGREE_TIERS is read when the row layout is built."""
    implicit, alpha, reg = MODES[mode]
    if tiers is None:
        monkeypatch.delenv("ALBEDO_DEGREE_TIERS", raising=False)
    else:
        monkeypatch.setenv("ALBEDO_DEGREE_TIERS", "1" if tiers else "0")
    user, item, r, B = _data(mode)
    c = Ctx(gpu_lib, k, implicit=implicit, reg=reg, alpha=alpha, light=light)
    c.ratings(user, item, r)
    return c


def _halves(c, mode, k):
    """Both halves, each from the injected unit-norm src: {side: (ids, X, path stats)}."""
    B = _data(mode)[3]
    out = {}
    for side in (1, 0):
        c.inject(0, B.user_ids, _src(k, len(B.user_ids), k))
        c.inject(1, B.item_ids, _src(k, len(B.item_ids), k + 1))
        c.half(side)
        ids, X = c.factors(side)
        out[side] = (ids, X, c.stats(side).tolist())
    return out


def _degrees(mode, side):
    B = _data(mode)[3]
    return np.diff(B.i_ptr if side == 1 else B.u_ptr), (B.item_ids if side == 1 else B.user_ids)


def _parent_stats(deg):
    light = deg <= 64
    return [int(light.sum()), int(deg[light].sum()), int((~light).sum()), int(deg[~light].sum())]


def test_ladder_shape():
    """Both sides hold at least two rows of every ladder degree, and the degree-40 / 72 rows."""
    for side in (0, 1):
        deg, _ = _degrees("unit", side)
        for d in DEGREES:
            assert np.sum(deg == d) >= 2, (side, d)
        for d in NONPOS_DEGREES:
            assert np.sum(deg == d) == 1, (side, d)
        assert 350 <= deg.size <= N_SIDE


@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("mode", list(MODES))
def test_tiers_parity_and_routing(gpu_lib, monkeypatch, tmp_path, mode, k):
    """Tiers on (the default) and off on the same inputs: every row of both against the fp64 oracle at
    1e-4 (reported by tier), als_path_stats equal to the parent rule (light = degree <= 64) either way,
    tiers-off bit-identical to a second tiers-off context, rows outside 33..48 / 65..80 bit-identical
    between on and off, rows inside within 1e-4 of the tiers-off result."""
    on = _halves(_ctx(gpu_lib, monkeypatch, mode, k, None), mode, k)
    off = _halves(_ctx(gpu_lib, monkeypatch, mode, k, False), mode, k)
    off2 = _halves(_ctx(gpu_lib, monkeypatch, mode, k, False), mode, k)
    for side in (1, 0):
        name = "item" if side else "user"
        deg, ids_ref = _degrees(mode, side)
        ids, X_on, st_on = on[side]
        _, X_off, st_off = off[side]
        assert np.array_equal(ids, ids_ref)
        assert st_on == _parent_stats(deg), (name, st_on)
        assert st_off == _parent_stats(deg), (name, st_off)
        assert np.array_equal(X_off, off2[side][1]), f"{name}: two tiers-off contexts differ"
        X_ref = _ref(mode, k, side)
        labels = np.array([label_of(d) for d in deg])
        zero = ~X_ref.any(axis=1)
        if mode == "mixed":
            for d in NONPOS_DEGREES:  # no positive rating: b = 0 and the solution is exactly 0
                assert zero[deg == d].all() and not X_on[deg == d].any() and not X_off[deg == d].any(), (name, d)
        for what, X in (("on", X_on), ("off", X_off)):
            err = LD.row_errors(X, X_ref)
            by = ", ".join(f"{p} {err[labels == p].max():.2e}" for p in sorted(set(labels.tolist())))
            print(f"DEGREE_TIERS {mode} k{k} {name} half tiers {what}: by tier {by}")
            LD.assert_rows(X, X_ref, ids, deg, labels, TOL, f"{name} half tiers {what} [{mode}-k{k}]", tmp_path)
        tier = np.array([tier_of(d) for d in deg])
        outside = tier == ""
        assert np.array_equal(X_on[outside], X_off[outside]), f"{name}: rows outside the tiers moved"
        for t in ("L48", "M80"):
            sel = tier == t
            assert sel.sum() >= 6
            same = np.array_equal(X_on[sel], X_off[sel])
            diff = LD.row_errors(X_on[sel], X_off[sel]).max()
            print(f"DEGREE_TIERS {mode} k{k} {name} half {t}: {int(sel.sum())} rows, on vs off worst {diff:.2e}, "
                  f"bit-identical {same}")
            LD.assert_rows(X_on[sel], X_off[sel], ids[sel], deg[sel], labels[sel], TOL,
                           f"{name} half {t} on vs off [{mode}-k{k}]", tmp_path)


@pytest.mark.parametrize("light", [0, 96])
def test_forced_paths_ignore_the_switch(gpu_lib, monkeypatch, light):
    """An explicit light_max_degree keeps the routing it names: the environment switch changes nothing."""
    a = _halves(_ctx(gpu_lib, monkeypatch, "unit", 128, True, light=light), "unit", 128)
    b = _halves(_ctx(gpu_lib, monkeypatch, "unit", 128, False, light=light), "unit", 128)
    for side in (1, 0):
        deg, _ = _degrees("unit", side)
        lim = deg <= light
        want = [int(lim.sum()), int(deg[lim].sum()), int((~lim).sum()), int(deg[~lim].sum())]
        assert a[side][2] == want and b[side][2] == want, (side, a[side][2], b[side][2], want)
        assert np.array_equal(a[side][1], b[side][1]), side


def test_tiers_deterministic_over_two_sweeps(gpu_lib, monkeypatch):
    """Two contexts with the tiers on give bit-identical factors after two sweeps."""
    B = _data("unit")[3]
    res = []
    for _ in range(2):
        c = _ctx(gpu_lib, monkeypatch, "unit", 128, None)
        c.inject(0, B.user_ids, _src(128, len(B.user_ids), 128))
        c.inject(1, B.item_ids, _src(128, len(B.item_ids), 129))
        for _sweep in range(2):
            c.half(1)
            c.half(0)
        res.append((c.factors(0)[1], c.factors(1)[1]))
    assert np.isfinite(res[0][0]).all() and np.isfinite(res[0][1]).all()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])

"""Top-k parity where albedo_amd/csrc/topk.hip is correct only because of an inequality or a mask:
all-negative scores next to zero padding rows, ties wider than the candidate lists, exactly-zero rows
on either side, row norms many decades below the global fp16 scale, ranks below the bound's four
directions, anisotropic factors that make the chunk bound prune, and every size boundary of the
kernels.  The inputs come from tests/topk_cases.py; their preconditions are asserted on the CPU by
tests/test_oracle.py.

No tolerance anywhere: ids and the bits of the F2J scores equal oracle.spark_als.recommend_for_all
(BoundedPriorityQueue over ascending ids), +0.0 and -0.0 are different, the GPU lists are compared
in the order they arrive, and rows shorter than k are padded with -1 / NaN.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import spark_als as O
from tests import ladder as LD
from tests import topk_cases as TC
from tests.test_gpu_parity import Ctx

pytestmark = pytest.mark.gpu

ALL_RANKS = TC.LOW_RANKS + TC.RANKS


def _recommend(lib, h, side, k, subset=None):
    """One als_recommend on a context: (src ids, ids, scores, stats delta, rescanned src ids)."""
    from albedo_amd import _lib as L
    st0, st1 = np.zeros(4, np.int64), np.zeros(4, np.int64)
    L.check(lib.als_topk_stats(h, L.ptr(st0, C.c_int64)))
    if subset is not None:
        subset = np.ascontiguousarray(subset, np.int32)
    n = lib.als_num_rows(h, side) if subset is None else subset.size
    src = np.full(n, -(1 << 31), np.int32)
    ids = np.full((n, k), -7, np.int32)
    sc = np.full((n, k), 12345.0, np.float32)
    L.check(lib.als_recommend(h, side, k, None if subset is None else L.ptr(subset, C.c_int32), n,
                              L.ptr(src, C.c_int32), L.ptr(ids, C.c_int32), L.ptr(sc, C.c_float)))
    L.check(lib.als_topk_stats(h, L.ptr(st1, C.c_int64)))
    n_res = np.zeros(1, np.int64)
    L.check(lib.als_topk_last_rescan(h, None, 0, L.ptr(n_res, C.c_int64)))
    resc = np.empty(max(int(n_res[0]), 1), np.int32)
    L.check(lib.als_topk_last_rescan(h, L.ptr(resc, C.c_int32), resc.size, L.ptr(n_res, C.c_int64)))
    return src, ids, sc, st1 - st0, resc[:int(n_res[0])]


def _run(lib, rank, users, items, calls):
    """A model of users = (ids, factors) and items = (ids, factors); one _recommend per call
    (side, k, subset or None); the model is destroyed whatever happens."""
    from albedo_amd import _lib as L
    uid, uf = (np.ascontiguousarray(a) for a in users)
    iid, itf = (np.ascontiguousarray(a) for a in items)
    assert uf.dtype == itf.dtype == np.float32 and uid.dtype == iid.dtype == np.int32
    h = C.c_void_p()
    L.check(lib.als_model_create(rank, uid.size, L.ptr(uid, C.c_int32), L.ptr(uf, C.c_float), iid.size,
                                 L.ptr(iid, C.c_int32), L.ptr(itf, C.c_float), -1, C.byref(h)))
    try:
        return [_recommend(lib, h, side, k, subset) for side, k, subset in calls]
    finally:
        lib.als_destroy(h)


def _assert_lists(what, src, ids, sc, ref_src, ref_ids, ref_sc, n_dst):
    """src ids, ids and score bits equal the reference, rows past n_dst entries padded with -1 / NaN;
    a mismatch names the first differing src id, its position and both (id, score bits) pairs."""
    assert np.array_equal(src, ref_src), f"{what}: src ids differ"
    assert ids.shape == ref_ids.shape and sc.shape == ref_sc.shape, (what, ids.shape, ref_ids.shape)
    gb, rb = sc.view(np.uint32), np.ascontiguousarray(ref_sc).view(np.uint32)
    bad = (ids != ref_ids) | (gb != rb)
    if bad.any():
        r, p = (int(x[0]) for x in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.any(axis=1).sum())} of {ids.shape[0]} rows differ; first src id "
                             f"{int(src[r])} position {p}: got (id {int(ids[r, p])}, bits 0x{int(gb[r, p]):08x}) "
                             f"want (id {int(ref_ids[r, p])}, bits 0x{int(rb[r, p]):08x})")
    m = min(ids.shape[1], n_dst)
    known = ~np.isnan(ref_sc[:, 0])  # by the score: -1 is a valid raw id
    assert np.all(ids[known, m:] == -1) and np.all(np.isnan(sc[known, m:])), f"{what}: padding"
    assert not np.any(np.isnan(sc[known, :m])), f"{what}: padding inside a list"
    assert np.all(ids[~known] == -1) and np.all(np.isnan(sc[~known])), f"{what}: unknown src ids"


def _whole_side(lib, gen, args, ks, swap=False, side=0, first=None):
    """recommendForAll* of a case at every k of ks against its oracle lists; swap: users and items
    trade places in the model (with side = 1 the same lists are then asked of the item side);
    first(k, stats delta, rescanned ids) runs before a call's lists are compared."""
    rank = args[0]
    uid, uf, iid, itf = TC.case(gen, *args)
    users, items = ((iid, itf), (uid, uf)) if swap else ((uid, uf), (iid, itf))
    src_is_items = swap != (side == 1)
    n_dst = uid.size if src_is_items else iid.size
    out = _run(lib, rank, users, items, [(side, k, None) for k in ks])
    for k, (src, ids, sc, st, resc) in zip(ks, out):
        ref = TC.oracle_lists(gen, args, k, src_is_items)
        print(f"TOPK_EDGES {gen}{args} k {k} side {side} swap {swap}: rows {st[0]} rescans {st[1]} "
              f"scanned {st[2]} of {st[3]}")
        if first:
            first(k, st, resc)
        _assert_lists(f"{gen}{args} k={k} side={side}", src, ids, sc, *ref, n_dst)
    return out


@pytest.mark.parametrize("rank", ALL_RANKS)
def test_topk_all_negative_scores(gpu_lib, rank):
    """Every score below 0 and a padded last chunk: a zero padding row of the fp16 image or of the
    probe image scores 0 and would head every list."""
    _whole_side(gpu_lib, "negative", (rank,), [30, 64])


@pytest.mark.parametrize("rank", ALL_RANKS)
def test_topk_ties_wider_than_the_lists(gpu_lib, rank):
    """300 identical dst rows hold the top score: the k-th place ties with more rows than a candidate
    list (128) holds, and the lists keep them by scan position, not by id.  With tied rows outside
    the list, kth <= t + e for any valid error bound e, so no row may be certified: every src id
    is in the exact rescan, which breaks the ties by id."""
    uid = TC.case("mass_tie", rank)[0]

    def every_row_rescanned(k, st, resc):
        assert np.array_equal(np.sort(resc), np.sort(uid)) and st[1] == uid.size, \
            f"k={k}: {resc.size} of {uid.size} src rows rescanned; certified: {np.setdiff1d(uid, resc)[:8]}"

    _whole_side(gpu_lib, "mass_tie", (rank,), [30, 64], first=every_row_rescanned)


@pytest.mark.parametrize("rank", ALL_RANKS)
def test_topk_group_ties_across_k(gpu_lib, rank):
    """Groups of 4 (k = 30) and 7 (k = 64) identical dst rows: the k-th and (k+1)-th score are equal
    for every src row, so the last places go to the lowest ids of a group."""
    for k, copies in TC.GROUP_TIES.items():
        _whole_side(gpu_lib, "group_ties", (rank, copies), [k])


@pytest.mark.parametrize("rank", ALL_RANKS)
def test_topk_zero_rows(gpu_lib, rank):
    """Exactly-zero rows as src (no norm, no direction, every dst row ties at +0.0) and as dst (40 % of
    the catalogue scores +0.0, the k-th score of many rows), from the user side and, with users and
    items swapped in the model, from the item side."""
    _whole_side(gpu_lib, "zeros", (rank,), [30, 64])
    _whole_side(gpu_lib, "zeros", (rank,), [30, 64], swap=True, side=1)


@pytest.mark.parametrize("kind", TC.DYNAMIC_KINDS)
@pytest.mark.parametrize("rank", TC.RANKS)
def test_topk_norm_dynamic_range(gpu_lib, rank, kind):
    """Row norms six (dst) and eight (src) decades below the side's largest, which sets the one fp16
    scale of the side: such rows round to zero in the pre-selection and only the absolute term of the
    certification bound covers them; the whole dst side at 2^-60 (the scale's exponent is clamped to
    60) and at 2^60."""
    _whole_side(gpu_lib, "dynamic_range", (rank, kind), [30, 64])


@pytest.mark.parametrize("rank", TC.RANKS)
def test_topk_anisotropic_pruning(gpu_lib, rank):
    """Two dominant directions, half of the src rows on the negative side of the first (tk_bound's lo
    side of the box): the chunk bound must skip work (0 < scanned < total) and lose nothing; k = 100
    runs the exact kernel's own chunk pruning on the same model."""
    out = _whole_side(gpu_lib, "anisotropic", (rank,), [30, 100])
    st = out[0][3]
    assert 0 < st[2] < st[3], f"scanned {st[2]} of {st[3]}: the chunk bound skipped nothing"


@pytest.mark.parametrize("rank", TC.RANKS)
def test_topk_size_boundaries(gpu_lib, rank):
    """n_dst around 64, one chunk, the 512 probe rows and one super-chunk; n_src around the order wave
    (16), the select workgroup (4) and the scan workgroup (128); k around the saturation of kt (48),
    the 64 / 65 switch to the exact scan and its 64·P list sizes; k > 64 above a padded catalogue of
    100.  One model of 129 users per n_dst, fewer src rows through the subset path."""
    n_calls = 0
    for n_dst, points in TC.size_grid(rank).items():
        uid, uf, iid, itf = TC.case("sizes", rank, n_dst)
        ref_src, ref_ids, ref_sc = TC.oracle_lists("sizes", (rank, n_dst), max(k for _, k in points))
        out = _run(gpu_lib, rank, (uid, uf), (iid, itf), [(0, k, ref_src[:n]) for n, k in points])
        for (n, k), (src, ids, sc, st, resc) in zip(points, out):
            _assert_lists(f"sizes rank={rank} n_dst={n_dst} n_src={n} k={k}", src, ids, sc,
                          ref_src[:n], ref_ids[:n, :k], ref_sc[:n, :k], n_dst)
            n_calls += 1
    print(f"TOPK_EDGES sizes rank {rank}: {n_calls} calls")


@pytest.mark.parametrize("rank", [50, 100])
def test_topk_dst_norms_past_the_gram_range_raise(gpu_lib, rank):
    """dst rows of norm ~2^78: every score is still a finite fp32 number, but the squared norms
    overflow the fp32 partial sums of the dst Gram, so the chunk bound has no basis.  als_recommend
    says so (the host eigensolver used to walk past the end of its arrays on the Inf / NaN matrix),
    and the same model still answers from the other side, whose dst rows are ordinary."""
    from albedo_amd import _lib as L
    uid, uf, iid, itf = TC.case("dynamic_range", rank, "dst_huge")
    itf = np.ascontiguousarray(itf * np.float32(2.0 ** 15))
    assert np.all(np.isfinite(itf)) and np.all(np.isfinite(O.f2j_sdot(uf[:4, None, :], itf[None, :, :])))
    with pytest.raises(L.ALSError, match="Gram"):
        _run(gpu_lib, rank, (uid, uf), (iid, itf), [(0, 30, None)])
    order = np.argsort(iid, kind="stable")
    ref_ids, ref_sc = O.recommend_for_all(iid[order][:40], itf[order][:40], uid, uf, 30)
    (src, ids, sc, _, _), = _run(gpu_lib, rank, (uid, uf), (iid, itf), [(1, 30, iid[order][:40])])
    _assert_lists(f"huge src rows rank={rank}", src, ids, sc, iid[order][:40], ref_ids, ref_sc, uid.size)


def test_topk_subset_order_and_duplicates(gpu_lib):
    """A subset that is unsorted, repeats ids and interleaves unknown ids (the binary-search path of
    als_recommend), on both sides: each output row is the oracle list of its own id, unknown ids
    give all-padding rows; and the same without unknown ids (results land in place)."""
    rank, k = 50, 30
    uid, uf, iid, itf = TC.case("negative", rank)
    rng = np.random.default_rng(5)
    calls, refs = [], []
    for side, ids_side in ((0, uid), (1, iid)):
        ref_src, ref_ids, ref_sc = TC.oracle_lists("negative", (rank,), k, side == 1)
        unknown = np.setdiff1d(np.arange(ids_side.min() - 3, ids_side.max() + 4), ids_side)
        for with_unknown in (True, False):
            sub = rng.choice(ids_side, 45, replace=False)
            sub = np.concatenate([sub, sub[:9], sub[3:5]])
            if with_unknown:
                sub = np.concatenate([sub, rng.choice(unknown, 11, replace=False),
                                      [ids_side.min() - 1, ids_side.max() + 1]])
            sub = rng.permutation(sub).astype(np.int32)
            assert np.any(np.diff(sub) < 0) and np.unique(sub).size < sub.size
            row = np.searchsorted(ref_src, sub)
            hit = ref_src[np.minimum(row, ref_src.size - 1)] == sub
            assert hit.all() != with_unknown
            want_ids = np.where(hit[:, None], ref_ids[np.minimum(row, ref_src.size - 1)], -1).astype(np.int32)
            want_sc = np.where(hit[:, None], ref_sc[np.minimum(row, ref_src.size - 1)], np.float32(np.nan))
            calls.append((side, k, sub))
            refs.append((sub, want_ids, want_sc.astype(np.float32), iid.size if side == 0 else uid.size))
    out = _run(gpu_lib, rank, (uid, uf), (iid, itf), calls)
    for (side, _, sub), (src, ids, sc, st, resc), (rs, ri, rsc, n_dst) in zip(calls, out, refs):
        _assert_lists(f"subset side={side} n={sub.size}", src, ids, sc, rs, ri, rsc, n_dst)


def test_recommend_after_fit_with_zero_factor_rows(gpu_lib):
    """The `mixed` ladder fitted at rank 50 (implicit, 2 sweeps): item rows without a positive rating
    get exactly-zero factors from the solve, and those factors then go through als_recommend on both
    sides (zero src rows on the item side, zero dst rows on the user side) against the oracle scorer
    applied to the GPU's own factors."""
    from albedo_amd import _lib as L
    rank, k = 50, 30
    implicit, alpha, reg = LD.MODES["mixed"]
    user, item, ideg = LD.ladder_coo()
    r = LD.ladder_ratings("mixed", user, ideg)
    B = O.make_blocks(user, item, r)
    c = Ctx(gpu_lib, rank, implicit=implicit, reg=reg, alpha=alpha, max_iter=2)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, LD.unit_rows(np.random.default_rng(rank), len(B.user_ids), rank))
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), rank), np.float32))
    L.check(gpu_lib.als_run_sweeps(c.h, 2))
    uids, U = c.factors(0)
    iids, V = c.factors(1)
    nonpos = np.isin(np.diff(B.i_ptr), LD.NONPOS_DEGREES)
    assert np.array_equal(iids, B.item_ids) and nonpos.sum() >= 2 * len(LD.NONPOS_DEGREES)
    assert not V[nonpos].any(), "item rows without a positive rating are not exactly zero"
    assert V[~nonpos].any(axis=1).all() and U.any(axis=1).all()
    for side, (sid, sf, did, df) in ((0, (uids, U, iids, V)), (1, (iids, V, uids, U))):
        src, ids, sc, st, resc = _recommend(gpu_lib, c.h, side, k)
        ref_ids, ref_sc = O.recommend_for_all(sid, sf, did, df, k)
        _assert_lists(f"fitted factors side={side}", src, ids, sc, sid, ref_ids, ref_sc, did.size)
        if side == 1:
            assert not ref_sc[nonpos].any() and not np.any(sc[nonpos].view(np.uint32))  # +0.0 throughout

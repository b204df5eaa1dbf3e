"""Every way als_recommend gets its lists out, at the smallest size that reaches them: in place through
the mapped caller arrays (by slot ranges and in scan order, several passes on the post stream with
both buffer sets reused), the staged copies behind per-range events, the synchronous copy-back of one
pass, the exact scan of k > 64 through the in-place and staged paths, and the multi-pass scatter of a
subset with unknown ids (binary search and merge walk).

ALBEDO_TOPK_PASS is clamped to 65,536 rows, which is then also the output range, and the asynchronous
paths need more dense rows than one range: 3 * 65,536 + 517 users give four passes, the last short.
Every 997th user is an all-zero row: its 300 scores tie at +0.0, wider than a candidate list, so it
cannot be certified (tests/topk_cases.py) and each range of each pass has rows that only the exact
rescan writes, through the same per-range offset as the select.

No tolerance: ids and score bits equal oracle.cbind.recommend for every row.  Which path a call took
is not visible here (a refused host registration takes the synchronous one); ALBEDO_TOPK_TRACE=1 with
-s names it per pass on stderr.
"""
import numpy as np
import pytest

from tests.test_gpu_topk_edges import _assert_lists, _recommend

pytestmark = pytest.mark.gpu

RANK = 8
PASS = 1 << 16
N_USERS = 3 * PASS + 517
N_ITEMS = 300
ZERO_EVERY, ZERO_FIRST = 997, 500  # 196,909 is the zero row of the last, 517-row pass
KNOBS = ("ALBEDO_TOPK_PASS", "ALBEDO_TOPK_ZEROCOPY", "ALBEDO_TOPK_OVERLAP")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


class Model:
    def __init__(self, lib):
        import ctypes as C

        from albedo_amd import _lib as L
        rng = np.random.default_rng(20261020)
        self.uid = (np.cumsum(rng.integers(1, 4, N_USERS)) - 5000).astype(np.int32)  # gaps, ~2500 negative ids
        self.uf = rng.standard_normal((N_USERS, RANK)).astype(np.float32)
        self.uf[ZERO_FIRST::ZERO_EVERY] = 0.0
        self.iid = (np.cumsum(rng.integers(1, 6, N_ITEMS)) - 40).astype(np.int32)
        self.itf = rng.standard_normal((N_ITEMS, RANK)).astype(np.float32)
        assert self.uid[0] < 0 < self.uid[-1] and np.any(np.diff(self.uid) > 1)
        self.lib, self.h, self._ref = lib, C.c_void_p(), {}
        L.check(lib.als_model_create(RANK, N_USERS, L.ptr(self.uid, C.c_int32), L.ptr(self.uf, C.c_float), N_ITEMS,
                                     L.ptr(self.iid, C.c_int32), L.ptr(self.itf, C.c_float), -1, C.byref(self.h)))

    def ref(self, k):
        """The oracle's lists of every user at k: computed once, read-only."""
        if k not in self._ref:
            from oracle import cbind
            ids, sc = cbind.recommend(self.uf, self.iid, self.itf, k)
            ids.setflags(write=False)
            sc.setflags(write=False)
            self._ref[k] = (ids, sc)
        return self._ref[k]

    def subset(self):
        """Unsorted: 140,000 known ids, a few of them twice, and 1,000 unknown ones (in the gaps, past
        both ends, INT32_MIN and INT32_MAX)."""
        rng = np.random.default_rng(7)
        known = rng.choice(self.uid, 140_000, replace=False)
        gaps = np.setdiff1d(np.arange(self.uid[0] - 50, self.uid[-1] + 50, dtype=np.int64), self.uid)
        unknown = np.concatenate([rng.choice(gaps, 998, replace=False), [I32_MIN, I32_MAX]])
        sub = rng.permutation(np.concatenate([known, known[:5], known[70_000:70_002], unknown])).astype(np.int32)
        assert np.any(np.diff(sub) < 0) and np.unique(sub).size == sub.size - 7
        return sub


@pytest.fixture(scope="module")
def model(gpu_lib):
    m = Model(gpu_lib)
    yield m
    gpu_lib.als_destroy(m.h)


def _knobs(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)


def _assert_ranges_rescanned(what, call_ids, resc):
    """call_ids: the src id at each position of the call's (known) rows.  A condition on the input:
    every 65,536-row range of every pass holds a row that went to the exact rescan."""
    hit = np.isin(call_ids, resc)
    for o0 in range(0, call_ids.size, PASS):
        assert hit[o0:o0 + PASS].any(), f"{what}: no rescanned row at positions [{o0}, {min(o0 + PASS, call_ids.size)})"


FOUR = {"ALBEDO_TOPK_PASS": str(PASS)}
ALL_USER_CALLS = {
    # four passes of one range each, k = 30
    "in_place_by_slot_ranges": (30, FOUR),
    "in_place_scan_order": (30, {**FOUR, "ALBEDO_TOPK_ZEROCOPY": "1"}),
    "staged_copies": (30, {**FOUR, "ALBEDO_TOPK_ZEROCOPY": "0"}),
    # ALBEDO_TOPK_OVERLAP=1 only changes the default pass size: accepted, same lists
    "overlap_in_place_by_slot_ranges": (30, {**FOUR, "ALBEDO_TOPK_OVERLAP": "1"}),
    "overlap_in_place_scan_order": (30, {**FOUR, "ALBEDO_TOPK_ZEROCOPY": "1", "ALBEDO_TOPK_OVERLAP": "1"}),
    "overlap_staged_copies": (30, {**FOUR, "ALBEDO_TOPK_ZEROCOPY": "0", "ALBEDO_TOPK_OVERLAP": "1"}),
    # no knobs: one pass, one 4M-row range -> the synchronous copy-back (the baseline)
    "one_pass_synchronous": (30, {}),
    # k > 64: the exact scan alone; staged, the ready callback covers the whole pass
    "exact_scan_in_place": (65, FOUR),
    "exact_scan_staged_copies": (65, {**FOUR, "ALBEDO_TOPK_ZEROCOPY": "0"}),
}


@pytest.mark.parametrize("name", list(ALL_USER_CALLS))
def test_recommend_all_users(model, monkeypatch, name):
    k, env = ALL_USER_CALLS[name]
    _knobs(monkeypatch, env)
    ref_ids, ref_sc = model.ref(k)
    src, ids, sc, st, resc = _recommend(model.lib, model.h, 0, k)
    print(f"RECOMMEND_OUTPUTS {name} k {k}: rows {st[0]} rescans {st[1]} ({resc.size} ids)")
    if k <= 64:
        _assert_ranges_rescanned(name, model.uid, resc)
    _assert_lists(name, src, ids, sc, model.uid, ref_ids, ref_sc, N_ITEMS)


@pytest.mark.parametrize("ascending", [False, True], ids=["unsorted_binary_search", "ascending_merge_walk"])
def test_recommend_subset_scatter(model, monkeypatch, ascending):
    """Unknown ids make the output sparse: three synchronous passes scattered through the position
    list; unknown rows come back as -1 / NaN and src_ids_out echoes the subset."""
    k = 30
    _knobs(monkeypatch, FOUR)
    sub = model.subset()
    if ascending:
        sub = np.sort(sub)
    row = np.minimum(np.searchsorted(model.uid, sub), N_USERS - 1)
    hit = model.uid[row] == sub
    assert hit.sum() == 140_007 and (~hit).sum() == 1000 and sub.min() == I32_MIN and sub.max() == I32_MAX
    ref_ids, ref_sc = model.ref(k)
    want_ids = np.where(hit[:, None], ref_ids[row], -1).astype(np.int32)
    want_sc = np.where(hit[:, None], ref_sc[row], np.float32(np.nan)).astype(np.float32)
    src, ids, sc, st, resc = _recommend(model.lib, model.h, 0, k, sub)
    print(f"RECOMMEND_OUTPUTS subset ascending {ascending}: rows {st[0]} rescans {st[1]} ({resc.size} ids)")
    assert st[0] == hit.sum()
    _assert_ranges_rescanned(f"subset ascending={ascending}", sub[hit], resc)
    _assert_lists(f"subset ascending={ascending}", src, ids, sc, sub, want_ids, want_sc, N_ITEMS)

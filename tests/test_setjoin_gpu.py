"""GPU tests of the set-overlap join (anr_setjoin_*, anorag_hip.note_relations): the device equals the brute-force
restatement (tests/setjoin_ref.py) and the reference's own output (tests/golden/relation_cases.json) exactly — integers
as integers, floats by their bits — at the smallest shapes where the kernels can go wrong."""
import ctypes as C
import functools

import numpy as np
import pytest

import setjoin_ref as ref

pytestmark = pytest.mark.gpu
CASES = ref.load_cases()
ANR_EINVAL, ANR_ESTATE = -1, -3


class Raw:
    """the C ABI as it is, from rows of integer ids"""

    def __init__(self, rows_ids, n_items=None):
        from anorag_hip import _lib as L
        self.L, self.lib = L, L.load()
        self.indptr, self.items = ref.to_csr(rows_ids)
        if n_items is None:
            n_items = int(self.items.max()) + 1 if len(self.items) else 0
        self.h = C.c_void_p()
        rc = self.lib.anr_setjoin_create(len(rows_ids), n_items, self.indptr.ctypes.data, self.items.ctypes.data, 0,
                                         C.byref(self.h))
        assert rc == 0, L.last_error()

    def slots(self, s):
        assert self.lib.anr_setjoin_set_option(self.h, 1, s) == 0, self.L.last_error()

    def cooccur_raw(self, min_common):
        npairs, ncommon = C.c_int64(-7), C.c_int64(-7)
        stats = np.full(8, -7, np.int64)
        rc = self.lib.anr_setjoin_cooccur(self.h, min_common, C.byref(npairs), C.byref(ncommon), stats.ctypes.data)
        return rc, npairs.value, ncommon.value, stats

    def fetch_raw(self, npairs, ncommon):
        out = [np.full(npairs, -7, np.int32) for _ in range(4)] + [np.full(npairs + 1, -7, np.int64), np.full(ncommon, -7, np.int32)]
        rc = self.lib.anr_setjoin_cooccur_fetch(self.h, *[a.ctypes.data for a in out])
        return rc, tuple(out)

    def cooccur(self, min_common):
        rc, npairs, ncommon, stats = self.cooccur_raw(min_common)
        assert rc == 0, self.L.last_error()
        rc, out = self.fetch_raw(npairs, ncommon)
        assert rc == 0, self.L.last_error()
        assert stats[2] == npairs and stats[3] == ncommon
        return out, stats

    def pair_counts(self, I, J):
        I, J = np.ascontiguousarray(I, np.int32), np.ascontiguousarray(J, np.int32)
        inter, uni = np.full(len(I), -7, np.int32), np.full(len(I), -7, np.int32)
        rc = self.lib.anr_setjoin_pair_counts(self.h, len(I), I.ctypes.data, J.ctypes.data, inter.ctypes.data, uni.ctypes.data)
        assert rc == 0, self.L.last_error()
        return inter, uni

    def close(self):
        if self.h.value:
            assert self.lib.anr_setjoin_destroy(self.h) == 0
            self.h = C.c_void_p()


def same_arrays(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (k, np.flatnonzero(g != w)[:8])


def check_against_ref(rows, min_commons=(1, 2, 3)):
    raw = Raw(rows)
    try:
        for m in min_commons:
            got, stats = raw.cooccur(m)
            same_arrays(got, ref.cooccur(rows, m))
        return stats
    finally:
        raw.close()


@functools.lru_cache(maxsize=None)
def zipf_rows(n=5000, n_items=3000, seed=5):
    """0-8 items a row from a Zipf-Mandelbrot law, p(k) ~ (k + 20)^-1.2: the head item is in about 5 % of the rows, so the
    restatement's quadratic output stays small enough to compute"""
    rng = np.random.default_rng(seed)
    p = (np.arange(n_items) + 21.0) ** -1.2
    p /= p.sum()
    sizes = rng.integers(0, 9, size=n)
    draws = rng.choice(n_items, size=int(sizes.sum()), p=p)
    rows, at = [], 0
    for k in sizes.tolist():
        rows.append(tuple(sorted(set(draws[at:at + k].tolist()))))
        at += k
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def zipf_expected(min_common):
    return ref.cooccur([list(r) for r in zipf_rows()], min_common)


def popular_rows():
    """item 0 in all of 1 500 rows — a posting tail longer than a wave's stride and more candidates than the table holds —
    plus sparse others"""
    rng = np.random.default_rng(11)
    return [sorted({0} | set(int(x) for x in rng.integers(1, 400, size=int(rng.integers(0, 4))))) for _ in range(1500)]


@pytest.mark.parametrize("rows", [[], [[0, 1]], [[0, 1], [1, 2]], [[0], [1]], [[], [], []], [[], [0, 1], [], [1], []]],
                         ids=["n0", "n1", "n2", "n2_disjoint", "all_empty", "some_empty"])
def test_tiny_shapes(rows):
    check_against_ref(rows, (1, 2))


def test_identical_rows_keep_every_pair():
    rows = [[1, 4, 6, 9, 12]] * 300
    raw = Raw(rows)
    try:
        got, stats = raw.cooccur(5)
        assert len(got[0]) == 300 * 299 // 2 and (got[2] == 5).all() and (got[3] == 5).all()
        same_arrays(got, ref.cooccur(rows, 5))
        assert raw.cooccur(6)[0][0].shape == (0,)
    finally:
        raw.close()


def test_one_item_in_every_row():
    rows = popular_rows()
    stats = check_against_ref(rows, (1, 2))
    assert stats[0] > 0 and stats[1] >= 1500 * 1499 // 2


def test_row_longer_than_a_workgroup():
    rng = np.random.default_rng(3)
    rows = [sorted(set(int(x) for x in rng.integers(0, 900, size=8))) for _ in range(200)]
    rows[17] = list(range(100, 700))
    rows[120] = list(range(0, 900, 2))
    check_against_ref(rows, (1, 3))


def test_min_common_above_every_overlap_is_empty():
    rows = [list(r) for r in zipf_rows()[:400]]
    raw = Raw(rows)
    try:
        (I, J, inter, uni, ptr, common), stats = raw.cooccur(50)
        assert len(I) == 0 and ptr.tolist() == [0] and len(common) == 0 and stats[2] == 0
    finally:
        raw.close()


@pytest.mark.parametrize("rows_of", [popular_rows, lambda: [list(r) for r in zipf_rows()[:1200]]], ids=["popular", "zipf"])
def test_forced_small_table_is_byte_equal_and_overflows(rows_of):
    rows = rows_of()
    raw = Raw(rows)
    try:
        for m in (1, 2):
            raw.slots(0)
            want, st_default = raw.cooccur(m)
            raw.slots(64)
            got, st_small = raw.cooccur(m)
            same_arrays(got, want)
            assert st_default[5] == 4096 and st_small[5] == 64
            assert st_small[4] > 0 and st_small[6] > st_small[0] and st_small[4] >= st_default[4]
            assert st_small[1] == st_default[1]  # the insertions are the candidates, whatever the passes
        raw.slots(256)
        same_arrays(raw.cooccur(2)[0], want)
    finally:
        raw.close()


@pytest.mark.parametrize("min_common", [1, 2])
def test_zipf_5000_against_the_restatement(min_common):
    rows = [list(r) for r in zipf_rows()]
    raw = Raw(rows)
    try:
        got, stats = raw.cooccur(min_common)
        same_arrays(got, zipf_expected(min_common))
        again, stats2 = raw.cooccur(min_common)   # two calls byte-equal
        same_arrays(again, got)
        assert stats.tolist() == stats2.tolist() and stats[7] > 0
        # cooccur, then pair_counts on the same handle: every returned pair has the same sizes
        I, J, inter, uni = got[:4]
        pi, pu = raw.pair_counts(I, J)
        assert np.array_equal(pi, inter) and np.array_equal(pu, uni)
        rc, after = raw.fetch_raw(len(I), len(got[5]))  # the result is still there
        assert rc == 0
        same_arrays(after, got)
    finally:
        raw.close()


def test_pair_counts_edges():
    rng = np.random.default_rng(9)
    rows = [sorted(set(int(x) for x in rng.integers(0, 1500, size=int(k)))) for k in rng.integers(0, 40, size=300)]
    rows[5], rows[6], rows[7] = [], list(range(0, 1500, 3)), list(range(0, 1500))   # empty, long, longer
    raw = Raw(rows, n_items=1500)
    try:
        I = np.concatenate([np.arange(300), rng.integers(0, 300, size=2000), [5, 5, 6, 7, 7]]).astype(np.int32)
        J = np.concatenate([np.arange(300), rng.integers(0, 300, size=2000), [5, 6, 7, 6, 7]]).astype(np.int32)
        inter, uni = raw.pair_counts(I, J)
        wi, wu = ref.pair_counts(rows, I.tolist(), J.tolist())
        assert np.array_equal(inter, wi) and np.array_equal(uni, wu)
        assert (inter[:300] == uni[:300]).all() and inter[5] == 0 and inter[7] == 1500   # i == j
        e_i, e_u = raw.pair_counts(np.zeros(0, np.int32), np.zeros(0, np.int32))        # n == 0
        assert e_i.shape == (0,) and e_u.shape == (0,)
        bad = np.array([300], np.int32)
        rc = raw.lib.anr_setjoin_pair_counts(raw.h, 1, bad.ctypes.data, bad.ctypes.data, bad.ctypes.data, bad.ctypes.data)
        assert rc == ANR_EINVAL
    finally:
        raw.close()


def test_refusals():
    raw = Raw([[0, 1], [1, 2], [0, 2]])
    try:
        rc, _ = raw.fetch_raw(3, 3)
        assert rc == ANR_ESTATE and "before" in raw.L.last_error()
        for m in (0, -1):
            rc, _, _, _ = raw.cooccur_raw(m)
            assert rc == ANR_EINVAL and "min_common" in raw.L.last_error()
        rc, _ = raw.fetch_raw(3, 3)
        assert rc == ANR_ESTATE
        for s in (32, 100, 8192):
            assert raw.lib.anr_setjoin_set_option(raw.h, 1, s) == ANR_EINVAL
        assert raw.lib.anr_setjoin_set_option(raw.h, 9, 64) == ANR_EINVAL
        got, _ = raw.cooccur(1)
        same_arrays(got, ref.cooccur([[0, 1], [1, 2], [0, 2]], 1))
    finally:
        raw.close()


def test_setjoin_class():
    from anorag_hip import SetJoin
    rows = [["b", "a", "b"], [], ("c", "a"), ["c", "b", "c"]]
    with SetJoin(rows) as sj:
        assert sj.items == ["b", "a", "c"]
        I, J, inter, uni, ptr, common, stats = sj.cooccur(1, return_stats=True)
        assert list(zip(I.tolist(), J.tolist())) == [(0, 2), (0, 3), (2, 3)]
        assert inter.tolist() == [1, 1, 1] and uni.tolist() == [3, 3, 3] and common.tolist() == [1, 0, 2]
        assert stats["pairs"] == 3 and stats["table_slots"] == 4096 and stats["rows_overflowed"] == 0
        pi, pu = sj.pair_counts([0, 1, 3], [3, 1, 3])
        assert pi.tolist() == [1, 0, 2] and pu.tolist() == [3, 0, 2]
    assert sj._h is None


@pytest.mark.parametrize("name", sorted(CASES))
def test_relation_builders_equal_the_reference(name):
    from anorag_hip import entity_coexistence_relations, topic_relations
    case = CASES[name]
    got = entity_coexistence_relations(case["notes"], threshold=case["threshold"])
    ref.same_relations(ref.canonical(got, case["notes"]), case["coexistence"])
    ref.same_relations(got, ref.entity_coexistence(case["notes"], case["threshold"]))  # its own order, too
    ref.same_relations(topic_relations(case["notes"]), case["topic"])

"""GPU: every kernel path of csrc/bm25.hip against the exact-order reference of tests/bm25_ref.py, through ctypes on the
C ABI, on synthetic postings whose sums depend on the order of the additions.  Bar: bit-exact float64, no tolerances.

Which kernel scores a chunk is decided in score_chunk (n_cu = 256 on the MI355X):
    R = min(32, max(1, ceil(1024 / nq)));  R = max(1, n_docs // 4096) when n_docs < 4096 R;  R <= 1 -> k_bm25
  handle A,   5 000 documents: R = 1 for every nq                               -> k_bm25 (1024-stride loops, bisection)
  handle B,  12 290 documents: R = 3 for nq <= 341 and for nq = 400 (ceil(1024 / 400) = 3), bounds 4096 and 8193;
                               R = 2 for nq = 512, bound 6145;  ANORAG_BM25_ONE_WG=1 -> k_bm25 above 8192 documents
  handle C, 131 072 documents: R = 32 for nq <= 33 (bounds 4096 r), R = ceil(1024 / 53) = 20 for the whole batch of 53
Each handle exists twice: all weights positive, and LOW / ALL / EVEN / ODD negative with mixed signs elsewhere.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bm25_ref as br

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "anorag.h")) as _f:
    EINVAL = int(re.search(r"#define\s+ANR_EINVAL\s+\((-?\d+)\)", _f.read()).group(1))
VARIANTS = ("pos", "neg")


def _lib():
    from anorag_hip import _lib as L
    return L


def _read(ptr, shape, dtype, offset_bytes=0):
    out = np.empty(shape, dtype=dtype)
    if out.nbytes:
        _lib().check(_lib().load().anr_device_copy(0, out.ctypes.data, C.c_void_p(ptr + offset_bytes), out.nbytes, 1),
                     "anr_device_copy")
    return out


class World:
    """one handle's postings, device handle, batch and reference rows — made once, shared, left unchanged"""

    def __init__(self, name, variant):
        self.name, self.variant = name, variant
        self.post = br.handle_postings(name, variant)
        self.n = self.post.n_docs
        batch = br.query_batch(self.post)
        self.names = [k for k, _ in batch]
        self.queries = [q for _, q in batch]
        self.lib = _lib().load()
        h = C.c_void_p()
        p = self.post
        _lib().check(self.lib.anr_bm25_create(0, p.n_docs, p.n_terms, p.indptr.ctypes.data, p.docs.ctypes.data,
                                              p.weights.ctypes.data, C.byref(h)), "anr_bm25_create")
        self.h = h
        self._ref = {}

    def ref(self, normalize):
        """([nq, n_docs] reference rows, [nq] reference maxima)"""
        if normalize not in self._ref:
            rows = np.empty((len(self.queries), self.n), dtype=np.float64)
            mx = np.empty(len(self.queries), dtype=np.float64)
            for i, q in enumerate(self.queries):
                rows[i], mx[i] = self.post.scores(q, normalize)
            rows.flags.writeable = False
            mx.flags.writeable = False
            self._ref[normalize] = (rows, mx)
        return self._ref[normalize]

    def scores_host(self, queries, normalize):
        qi, qt = br.csr_queries(queries)
        out = np.full((len(queries), self.n), np.nan)
        _lib().check(self.lib.anr_bm25_scores(self.h, len(queries), qi.ctypes.data, qt.ctypes.data, normalize,
                                              out.ctypes.data), "anr_bm25_scores")
        return out

    def scores_dev(self, queries, normalize, with_max=True):
        from anorag_hip.fusion import DeviceArray
        qi, qt = br.csr_queries(queries)
        nq = len(queries)
        out = DeviceArray.from_numpy(np.full((nq, self.n), np.nan))
        mx = DeviceArray.from_numpy(np.full((nq, 1), np.nan))
        try:
            _lib().check(self.lib.anr_bm25_scores_dev(self.h, nq, qi.ctypes.data, qt.ctypes.data, normalize,
                                                      C.c_void_p(out.ptr), C.c_void_p(mx.ptr) if with_max else None),
                         "anr_bm25_scores_dev")
            return out.numpy(), mx.numpy().reshape(-1)
        finally:
            out.free()
            mx.free()

    def close(self):
        if self.h:
            self.lib.anr_bm25_destroy(self.h)
            self.h = None


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name, variant) -> World:
        if (name, variant) not in made:
            made[(name, variant)] = World(name, variant)
        return made[(name, variant)]

    yield get
    for w in made.values():
        w.close()


def _assert_rows(got, exp, names, what):
    assert got.shape == exp.shape, what
    if got.tobytes() == exp.tobytes():
        return
    bad = [(names[i], int(np.sum(got[i].view(np.int64) != exp[i].view(np.int64)))) for i in range(len(exp))
           if got[i].tobytes() != exp[i].tobytes()]
    raise AssertionError(f"{what}: rows differ from the reference (query, documents that differ): {bad}")


def _assert_max(got, exp, names, what):
    bad = [(names[i], float(got[i]), float(exp[i])) for i in range(len(exp)) if got[i].tobytes() != exp[i].tobytes()]
    assert not bad, f"{what}: row maxima differ from the reference (query, got, expected): {bad}"


def _check_dense(w, idx, normalize, what):
    """anr_bm25_scores, anr_bm25_scores_dev with and without max_dev, for the queries idx of the batch in one call"""
    rows, mx = w.ref(normalize)
    queries = [w.queries[i] for i in idx]
    names = [w.names[i] for i in idx]
    exp, exp_mx = rows[idx], mx[idx]
    _assert_rows(w.scores_host(queries, normalize), exp, names, f"{what} anr_bm25_scores")
    got, got_mx = w.scores_dev(queries, normalize)
    _assert_rows(got, exp, names, f"{what} anr_bm25_scores_dev")
    _assert_max(got_mx, exp_mx, names, f"{what} anr_bm25_scores_dev")
    got, got_mx = w.scores_dev(queries, normalize, with_max=False)   # normalize = 0: the early return after the additions
    _assert_rows(got, exp, names, f"{what} anr_bm25_scores_dev(max_dev = NULL)")
    assert np.all(np.isnan(got_mx))                                   # (never handed over: still the sentinel)


@pytest.mark.parametrize("normalize", (0, 1))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(br.HANDLES))
def test_dense_scores_equal_the_reference(worlds, name, variant, normalize):
    w = worlds(name, variant)
    nb = len(w.queries)
    # A: R = 1 (k_bm25).  B: nb = 25 -> R = 3.  C: nb = 53 -> R = ceil(1024 / 53) = 20
    assert nb == {"A": 21, "B": 25, "C": 53}[name]
    _check_dense(w, list(range(nb)), normalize, f"{name}/{variant} whole batch")
    if name == "C":   # halves of 26 and 27 queries: ceil(1024 / 27) = 38 -> R = 32, the bounds the EDGE terms sit on
        _check_dense(w, list(range(nb // 2)), normalize, "C first half (R = 32)")
        _check_dense(w, list(range(nb // 2, nb)), normalize, "C second half (R = 32)")
    if name == "B":   # nq = 400: ceil(1024 / 400) = 3 -> R = 3;  nq = 512: ceil(1024 / 512) = 2 -> R = 2
        rows, mx = w.ref(normalize)
        for nq in (400, 512):
            idx = [(7 * i) % nb for i in range(nq)]
            got, got_mx = w.scores_dev([w.queries[i] for i in idx], normalize)
            names = [f"{w.names[i]}@{k}" for k, i in enumerate(idx)]
            _assert_rows(got, rows[idx], names, f"B nq = {nq}")
            _assert_max(got_mx, mx[idx], names, f"B nq = {nq}")


@pytest.mark.parametrize("normalize", (0, 1))
@pytest.mark.parametrize("variant", VARIANTS)
def test_single_workgroup_kernel_above_8192_documents(worlds, monkeypatch, variant, normalize):
    """ANORAG_BM25_ONE_WG (read per call) sends handle B's batch through k_bm25"""
    w = worlds("B", variant)
    monkeypatch.setenv("ANORAG_BM25_ONE_WG", "1")
    _check_dense(w, list(range(len(w.queries))), normalize, f"B/{variant} one workgroup")


@pytest.mark.parametrize("normalize", (0, 1))
@pytest.mark.parametrize("cap", (6144, 7168, 65536))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(br.HANDLES))
def test_sparse_rows_equal_the_reference(worlds, name, variant, cap, normalize):
    """cap 6144: the LDS hash table (rows unordered); 7168 and 65536: document-range slices (rows ascending by id)"""
    from anorag_hip.fusion import SparseRows
    w = worlds(name, variant)
    rows, mx = w.ref(normalize)
    nq = len(w.queries)
    qi, qt = br.csr_queries(w.queries)
    sp = SparseRows(nq, w.n, cap, 0)
    cnt_host = np.full(nq, -7, dtype=np.int32)
    try:
        _lib().check(w.lib.anr_bm25_sparse_dev(w.h, nq, qi.ctypes.data, qt.ctypes.data, normalize, cap,
                                               C.c_void_p(sp.ids_ptr), C.c_void_p(sp.scores_ptr), C.c_void_p(sp.count_ptr),
                                               C.c_void_p(sp.max_ptr), cnt_host.ctypes.data), "anr_bm25_sparse_dev")
        ids = _read(sp.ids_ptr, (nq, cap), np.uint32)
        val = _read(sp.scores_ptr, (nq, cap), np.float64)
        cnt = _read(sp.count_ptr, (nq,), np.int32)
        got_mx = _read(sp.max_ptr, (nq,), np.float64)
    finally:
        sp.free()
    assert cnt.tolist() == cnt_host.tolist()
    why = [w.post.sparse_refusal(q, cap) for q in w.queries]
    for i, q in enumerate(w.queries):
        what = f"{name}/{variant} cap {cap} query {w.names[i]}"
        touched = w.post.touched(q)
        if why[i] is not None:
            assert cnt[i] == -1 and np.isnan(got_mx[i]), f"{what}: cannot be held ({why[i]}), count {cnt[i]}"
            continue
        assert cnt[i] == len(touched), what
        got_ids = ids[i, :cnt[i]].astype(np.int64)
        if cap > br.HASH_CAP:
            assert np.all(np.diff(got_ids) > 0), f"{what}: ids not strictly ascending on the device"
        assert len(np.unique(got_ids)) == len(got_ids) and np.sort(got_ids).tolist() == touched.tolist(), what
        assert val[i, :cnt[i]].tobytes() == rows[i][got_ids].tobytes(), f"{what}: values differ from the reference row"
        assert got_mx[i].tobytes() == mx[i].tobytes(), f"{what}: maximum {got_mx[i]} != {mx[i]}"
    held = sum(x is None for x in why)
    assert held * 4 >= 3 * nq
    if cap > br.HASH_CAP:
        assert all(why[w.names.index(k)] is None for k in ("short513", "short1100", "short600_L1025"))
    if name == "C" and cap == 7168:   # each refusal of the sliced form occurs
        assert {"sum", "slice", "count"} <= set(why)


@pytest.mark.parametrize("normalize", (0, 1))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(br.HANDLES))
def test_nonzero_compaction_equals_the_reference(worlds, name, variant, normalize):
    w = worlds(name, variant)
    rows, _ = w.ref(normalize)
    nq, cap = len(w.queries), w.n
    qi, qt = br.csr_queries(w.queries)
    docs = np.full((nq, cap), -7, dtype=np.int32)
    sc = np.full((nq, cap), np.nan)
    cnt = np.full(nq, -7, dtype=np.int32)
    _lib().check(w.lib.anr_bm25_nonzero(w.h, nq, qi.ctypes.data, qt.ctypes.data, normalize, cap, docs.ctypes.data,
                                        sc.ctypes.data, cnt.ctypes.data), "anr_bm25_nonzero")
    for i in range(nq):
        nz = np.nonzero(rows[i])[0]
        assert cnt[i] == len(nz), w.names[i]
        d = docs[i, :cnt[i]].astype(np.int64)
        assert np.sort(d).tolist() == nz.tolist(), w.names[i]
        assert sc[i, :cnt[i]].tobytes() == rows[i][d].tobytes(), w.names[i]
    # a cap below the count: the count is reported in full, the cap entries returned are distinct and right
    k = w.names.index("L2047")
    qi, qt = br.csr_queries([w.queries[k]])
    docs = np.full((1, 100), -7, dtype=np.int32)
    sc = np.full((1, 100), np.nan)
    cnt = np.full(1, -7, dtype=np.int32)
    _lib().check(w.lib.anr_bm25_nonzero(w.h, 1, qi.ctypes.data, qt.ctypes.data, normalize, 100, docs.ctypes.data,
                                        sc.ctypes.data, cnt.ctypes.data), "anr_bm25_nonzero")
    assert cnt[0] == 2047 == np.count_nonzero(rows[k])
    d = docs[0].astype(np.int64)
    assert len(set(d.tolist())) == 100 and d.min() >= 0 and d.max() < w.n and np.all(rows[k][d] != 0.0)
    assert sc[0].tobytes() == rows[k][d].tobytes()


def test_nonzero_with_no_documents_or_no_queries_writes_nothing(worlds):
    lib = _lib().load()
    indptr = np.zeros(3, dtype=np.int64)
    h = C.c_void_p()
    _lib().check(lib.anr_bm25_create(0, 0, 2, indptr.ctypes.data, None, None, C.byref(h)), "anr_bm25_create")
    try:
        qi, qt = br.csr_queries([[0, 1], [], [1]])
        docs = np.full((3, 4), -7, dtype=np.int32)
        sc = np.full((3, 4), -7.0)
        cnt = np.full(3, -7, dtype=np.int32)
        assert lib.anr_bm25_nonzero(h, 3, qi.ctypes.data, qt.ctypes.data, 1, 4, docs.ctypes.data, sc.ctypes.data,
                                    cnt.ctypes.data) == 0
        assert cnt.tolist() == [0, 0, 0] and np.all(docs == -7) and np.all(sc == -7.0)
        out = np.full(5, -7.0)
        assert lib.anr_bm25_scores(h, 3, qi.ctypes.data, qt.ctypes.data, 1, out.ctypes.data) == 0 and np.all(out == -7.0)
    finally:
        lib.anr_bm25_destroy(h)
    w = worlds("A", "pos")
    qi, qt = br.csr_queries([])
    docs = np.full((1, 4), -7, dtype=np.int32)
    sc = np.full((1, 4), -7.0)
    cnt = np.full(1, -7, dtype=np.int32)
    assert lib.anr_bm25_nonzero(w.h, 0, qi.ctypes.data, qt.ctypes.data, 1, 4, docs.ctypes.data, sc.ctypes.data,
                                cnt.ctypes.data) == 0
    assert cnt.tolist() == [-7] and np.all(docs == -7) and np.all(sc == -7.0)
    out = np.full(5, -7.0)
    assert lib.anr_bm25_scores(w.h, 0, qi.ctypes.data, qt.ctypes.data, 1, out.ctypes.data) == 0 and np.all(out == -7.0)


# ---- the field combiner -----------------------------------------------------------------------------------------------
def _field_rows(n_fields, weights, nq=5, n=3001):
    """random float64 field rows [n_fields][nq][n]; query 3 combines to an all-negative row, query 4 to all zeros"""
    rng = np.random.default_rng(100 + n_fields)
    f = np.ldexp(1.0 + rng.random((n_fields, nq, n)), rng.integers(-30, 31, size=(n_fields, nq, n)))
    f *= np.where(rng.random(f.shape) < 0.5, -1.0, 1.0)
    for k, wk in enumerate(weights):
        f[k, 3] = -np.abs(f[k, 3]) if wk > 0 else np.abs(f[k, 3])
    f[:, 4] = 0.0
    return f


@pytest.mark.parametrize("normalize", (0, 1))
@pytest.mark.parametrize("n_fields", (1, 3, 8))
def test_field_combiner_equals_the_reference_also_in_place(n_fields, normalize):
    from anorag_hip.fusion import DeviceArray
    lib = _lib().load()
    nq, n = 5, 3001   # 3001: not a multiple of the 1024 threads
    weights = {1: [2.0], 3: [2.0, 1.5, 1.0], 8: [2.0, 1.5, 1.0, 0.75, -1.25, 3.0, 0.5, 1e-3]}[n_fields]
    f = _field_rows(n_fields, weights)
    exp = np.empty((nq, n))
    exp_mx = np.empty(nq)
    for q in range(nq):
        exp[q], exp_mx[q] = br.combine([f[k, q] for k in range(n_fields)], weights, normalize)
    assert exp[3].max() < 0 and exp_mx[3] == exp[3].max() and not exp[4].any() and exp_mx[4] == 0.0
    wa = np.asarray(weights, dtype=np.float64)
    names = [f"query {q}" for q in range(nq)]
    for aliased in (False, True):
        fields = [DeviceArray.from_numpy(f[k]) for k in range(n_fields)]
        out = fields[0] if aliased else DeviceArray.from_numpy(np.full((nq, n), np.nan))
        mx = DeviceArray.from_numpy(np.full((nq, 1), np.nan))
        ptrs = (C.c_void_p * n_fields)(*[a.ptr for a in fields])
        try:
            _lib().check(lib.anr_bm25_combine_fields(0, n_fields, ptrs, wa.ctypes.data, nq, n, normalize,
                                                     C.c_void_p(out.ptr), C.c_void_p(mx.ptr)), "anr_bm25_combine_fields")
            _assert_rows(out.numpy(), exp, names, f"{n_fields} fields, aliased={aliased}")
            _assert_max(mx.numpy().reshape(-1), exp_mx, names, f"{n_fields} fields, aliased={aliased}")
            if not aliased:   # max_dev = NULL: the same rows
                out2 = DeviceArray.from_numpy(np.full((nq, n), np.nan))
                _lib().check(lib.anr_bm25_combine_fields(0, n_fields, ptrs, wa.ctypes.data, nq, n, normalize,
                                                         C.c_void_p(out2.ptr), None), "anr_bm25_combine_fields")
                _assert_rows(out2.numpy(), exp, names, f"{n_fields} fields, max_dev = NULL")
                out2.free()
        finally:
            for a in fields:
                a.free()
            if not aliased:
                out.free()
            mx.free()


def test_field_combiner_refuses_bad_field_counts_and_null_fields():
    from anorag_hip.fusion import DeviceArray
    lib = _lib().load()
    a = DeviceArray.from_numpy(np.ones((2, 8)))
    out = DeviceArray.from_numpy(np.full((2, 8), 7.0))
    w = np.ones(9)
    try:
        ptrs = (C.c_void_p * 9)(*[a.ptr] * 9)
        for nf in (0, 9, -1):
            assert lib.anr_bm25_combine_fields(0, nf, ptrs, w.ctypes.data, 2, 8, 1, C.c_void_p(out.ptr), None) == EINVAL
        assert lib.anr_bm25_combine_fields(0, 3, None, w.ctypes.data, 2, 8, 1, C.c_void_p(out.ptr), None) == EINVAL
        ptrs[1] = None
        assert lib.anr_bm25_combine_fields(0, 3, ptrs, w.ctypes.data, 2, 8, 1, C.c_void_p(out.ptr), None) == EINVAL
        assert lib.anr_bm25_combine_fields(0, 1, ptrs, w.ctypes.data, 2, 8, 1, None, None) == EINVAL
        assert np.all(out.numpy() == 7.0)                          # nothing was written by a refused call
        assert lib.anr_bm25_combine_fields(0, 1, ptrs, w.ctypes.data, 2, 8, 1, C.c_void_p(out.ptr), None) == 0
        assert np.all(out.numpy() == 1.0)
    finally:
        a.free()
        out.free()


# ---- the second chunk of anr_bm25_scores, the second sub-batch of slices ------------------------------------------------
def test_second_chunk_of_host_scores(worlds):
    """131 072 documents: a chunk is 2^30 / (131072 * 8) = 1024 queries, so the last six of 1030 are scored by a second
    score_chunk call whose offsets are made relative by upload_queries.  Every query is another pair of SHORT terms: a
    misplaced offset scores the wrong terms.  (The first chunk has nq = 1024 -> R = 1, the second nq = 6 -> R = 32.)"""
    w = worlds("C", "pos")
    nq = 1030
    sh = w.post.short
    queries = [[sh[k], sh[(7 * k + 3) % br.N_SHORT]] for k in range(nq)]
    assert len({tuple(q) for q in queries}) == nq and all(a != b for a, b in queries)
    qi, qt = br.csr_queries(queries)
    out = np.empty((nq, w.n), dtype=np.float64)    # 1.08 GB: what reaching a second chunk costs
    _lib().check(w.lib.anr_bm25_scores(w.h, nq, qi.ctypes.data, qt.ctypes.data, 1, out.ctypes.data), "anr_bm25_scores")
    bad = []
    for k, q in enumerate(queries):
        ids, vals, _ = w.post.sparse_scores(q, 1)
        if out[k, ids].tobytes() != vals.tobytes() or np.count_nonzero(out[k]) != np.count_nonzero(vals):
            bad.append(k)
    assert not bad, f"queries that differ from the reference: {bad}"


def test_second_sub_batch_of_slices(worlds):
    """cap 65536, four tokens of {EVEN, ODD, LOW} (65 536 postings each): a posting sum of 262 144 = 4 cap, 128 slices per
    query; 129 queries are 16 512 slices > 16 384, so the last query runs in a second sub-batch of sparse_sliced"""
    from anorag_hip.fusion import SparseRows
    w = worlds("C", "pos")
    cap, nq, normalize = 65536, 129, 1
    three = [w.post.term["EVEN"], w.post.term["ODD"], w.post.term["LOW"]]
    queries = [[three[(i % 81) // 3 ** p % 3] for p in (3, 2, 1, 0)] for i in range(nq)]
    queries[-1] = [three[2]] * 4                                   # LOW four times: held, and not the first query's row
    assert all(w.post.posting_sum(q) == 4 * cap for q in queries) and queries[0] == [three[0]] * 4
    assert all(queries[i] != queries[i + 1] for i in range(nq - 1))
    why = [w.post.sparse_refusal(q, cap) for q in queries]
    held = [i for i in range(nq) if why[i] is None]
    assert held == [0, 40, 80, 81, 121, 128]                       # one term only; a mix touches more than cap documents
    qi, qt = br.csr_queries(queries)
    sp = SparseRows(nq, w.n, cap, 0)
    try:
        _lib().check(w.lib.anr_bm25_sparse_dev(w.h, nq, qi.ctypes.data, qt.ctypes.data, normalize, cap,
                                               C.c_void_p(sp.ids_ptr), C.c_void_p(sp.scores_ptr), C.c_void_p(sp.count_ptr),
                                               C.c_void_p(sp.max_ptr), None), "anr_bm25_sparse_dev")
        cnt = _read(sp.count_ptr, (nq,), np.int32)
        got_mx = _read(sp.max_ptr, (nq,), np.float64)
        assert cnt.tolist() == [65536 if i in held else -1 for i in range(nq)]
        assert np.isnan(got_mx).tolist() == [i not in held for i in range(nq)]
        for i in (0, 40, 80, 126, 127, 128):                       # the last three rows and three others
            if i not in held:
                continue
            ids = _read(sp.ids_ptr, (cap,), np.uint32, i * cap * 4).astype(np.int64)
            val = _read(sp.scores_ptr, (cap,), np.float64, i * cap * 8)
            t, v, m = w.post.sparse_scores(queries[i], normalize)
            assert ids.tolist() == t.tolist(), f"row {i}: ids"
            assert val.tobytes() == v.tobytes(), f"row {i}: values"
            assert got_mx[i] == m == 1.0
    finally:
        sp.free()

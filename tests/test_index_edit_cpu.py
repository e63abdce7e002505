"""CPU tests of the in-place index edits: the source map the compaction kernel evaluates (restated in
tests/index_edit_ref.py) is the numbering numpy's delete gives, and the C entry points validate their arguments before any
device work."""
import ctypes as C

import numpy as np
import pytest

import index_edit_ref as ref


def _gone_sets(n):
    rng = np.random.default_rng(100 + n)
    sets = [np.zeros(0, np.int64), np.arange(n), np.array([0]), np.array([n - 1])]
    for frac in (0.1, 0.5, 0.9):
        sets.append(np.sort(rng.choice(n, max(1, int(n * frac)), replace=False)))
    for _ in range(5):
        sets.append(np.flatnonzero(rng.random(n) < rng.random()))
    return sets


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_source_map_is_numpy_delete(n):
    for gone in _gone_sets(n):
        gone = np.asarray(gone, dtype=np.int64)
        got = ref.source_map(n, gone)
        assert np.array_equal(got, np.delete(np.arange(n), gone)), (n, gone)
        assert np.all(got >= np.arange(len(got)))       # a destination never lies above its source


def test_valid_gone_ignores_duplicates_and_rows_outside():
    assert ref.valid_gone([5, 5, -1, 10, 3, 11, 2**40], 10).tolist() == [3, 5]
    assert ref.valid_gone([], 10).size == 0 and ref.valid_gone([-3, 10, 10], 10).size == 0


def test_edit_entry_points_validate_before_any_device_work():
    from anorag_hip import _lib
    lib = _lib.load()
    rows = np.array([0], dtype=np.int64)
    x = np.zeros((1, 8), dtype=np.float32)
    n_removed = C.c_int64(7)
    assert lib.anr_index_remove(None, rows.ctypes.data, 1, C.byref(n_removed)) == -1
    assert n_removed.value == 0
    assert lib.anr_index_update(None, rows.ctypes.data, x.ctypes.data, 1) == -1
    # null rows / vectors with n > 0, negative n: refused on the arguments alone — the handle is never looked at, so a
    # block of zero bytes can stand in for one on a machine without a device
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert lib.anr_index_remove(h, None, 1, None) == -1
    assert lib.anr_index_update(h, None, x.ctypes.data, 1) == -1
    assert lib.anr_index_update(h, rows.ctypes.data, None, 1) == -1
    assert lib.anr_index_remove(h, rows.ctypes.data, -1, None) == -1
    assert lib.anr_index_update(h, rows.ctypes.data, x.ctypes.data, -1) == -1
    assert b"bad argument" in lib.anr_last_error()
    assert _lib.OPT_EDIT_CHUNK_ROWS == 15

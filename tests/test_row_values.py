"""CPU suite: the numpy restatement of the row-constant detection (h2gcn_amd/csrc/h2gcn_capi.hip, row_values_kernel) on hand-built
arrays.  A hop is ROW-CONSTANT when every stored value of each row carries the BITS of the row's first stored value; the plan then
keeps that value per row (0 for an empty row) and forward launches do not read the value array.  tests/test_row_values_gpu.py
checks ``HopPlan.row_constant`` and the launches against this restatement."""
import numpy as np

F32 = np.float32


def row_values_np(indptr, data):
    """(row_constant, rowval bits): the detection restated -- uint32 view, every entry compared with its row's first one."""
    indptr = np.asarray(indptr, dtype=np.int64)
    bits = np.ascontiguousarray(np.asarray(data, dtype=F32)).view(np.uint32)
    lengths = np.diff(indptr)
    first = np.zeros(len(lengths), dtype=np.uint32)
    first[lengths > 0] = bits[indptr[:-1][lengths > 0]]
    return bool((bits == np.repeat(first, lengths)).all()), first


def row_constant_np(indptr, data):
    return int(row_values_np(indptr, data)[0])


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(F32)


def test_constant_rows_empty_rows_and_single_entries():
    indptr = [0, 0, 3, 4, 4, 6, 6]                  # empty first, in the middle and last; a single-entry row
    data = np.array([0.5, 0.5, 0.5, -2.0, 7.0, 7.0], dtype=F32)
    ok, first = row_values_np(indptr, data)
    assert ok
    assert first.view(F32).tolist() == [0.0, 0.5, -2.0, 0.0, 7.0, 0.0]
    assert first[[0, 3, 5]].tolist() == [0, 0, 0]   # +0.0 bits, not -0.0
    # rows of ONE entry are constant whatever they hold
    assert row_constant_np([0, 1, 2, 3], _bits(0x7fc00001, 0x80000000, 0x00000001))


def test_a_hop_without_nonzeros_and_without_rows():
    assert row_constant_np([0, 0, 0, 0], np.zeros(0, F32)) == 1
    assert row_values_np([0, 0, 0, 0], np.zeros(0, F32))[1].tolist() == [0, 0, 0]
    assert row_constant_np([0], np.zeros(0, F32)) == 1


def test_one_differing_entry_anywhere_clears_it():
    indptr = [0, 4, 4, 7]
    base = np.array([0.25] * 4 + [3.0] * 3, dtype=F32)
    assert row_constant_np(indptr, base)
    for at in range(len(base)):                     # first / middle / last of a row, the last row
        data = base.copy()
        data[at] = np.nextafter(data[at], F32(10))  # the last mantissa bit
        assert (data.view(np.uint32)[at] ^ base.view(np.uint32)[at]) == 1
        assert not row_constant_np(indptr, data), at


def test_the_comparison_is_on_bits():
    indptr = [0, 3]
    assert not row_constant_np(indptr, np.array([0.0, -0.0, 0.0], dtype=F32))          # equal as numbers, not as bits
    assert not row_constant_np(indptr, np.array([-0.0, -0.0, 0.0], dtype=F32))
    assert row_constant_np(indptr, np.array([-0.0, -0.0, -0.0], dtype=F32))
    assert row_values_np(indptr, np.array([-0.0] * 3, dtype=F32))[1].tolist() == [0x80000000]
    assert row_constant_np(indptr, _bits(0x7fc00000, 0x7fc00000, 0x7fc00000))          # one NaN payload: unequal as numbers, equal as bits
    assert not row_constant_np(indptr, _bits(0x7fc00000, 0x7fc00001, 0x7fc00000))      # two payloads
    assert not row_constant_np(indptr, _bits(0x7fc00000, 0xffc00000, 0x7fc00000))      # the NaN's sign
    assert row_constant_np(indptr, np.array([np.inf] * 3, dtype=F32))
    assert not row_constant_np(indptr, np.array([np.inf, -np.inf, np.inf], dtype=F32))
    assert row_constant_np(indptr, _bits(1, 1, 1)) and not row_constant_np(indptr, _bits(1, 2, 1))   # subnormals


def test_rows_may_differ_from_each_other():
    rng = np.random.default_rng(0)
    lengths = rng.integers(0, 9, 50)
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    per_row = rng.uniform(-1, 1, 50).astype(F32)
    ok, first = row_values_np(indptr, np.repeat(per_row, lengths))
    assert ok
    assert np.array_equal(first.view(F32)[lengths > 0], per_row[lengths > 0]) and not first[lengths == 0].any()

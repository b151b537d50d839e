"""CPU tests of tests/support.py: every asserting helper accepts what it must accept and rejects what
it must reject, on the smallest arrays that tell the two apart (B = 2 instances, N = 1)."""
import numpy as np
import pytest

from support import (IT_FILL, ST_FILL, assert_due_result, assert_same, assert_same_bits, assert_swing_zero, bits,
                     row_by_row, rows_of, sentinel_forces)

B, COLS = 2, 12


def solve_result():
    """(forces, status, iters) as a solve of two instances at N = 1 leaves them."""
    f = np.linspace(-30.0, 90.0, B * COLS, dtype=np.float32).reshape(B, COLS)
    return f, np.zeros(B, np.uint8), np.array([3, 5], np.int32)


def flipped(f, i, j, bit=0):
    """A copy of the forces with one bit of word (i, j) flipped (bit 0: the last mantissa bit)."""
    out = f.copy()
    out.view(np.uint32)[i, j] ^= np.uint32(1 << bit)
    return out


def test_sentinel_forces_words():
    s = sentinel_forces(2, 12)
    assert s.shape == (2, 12) and s.dtype == np.float32
    assert np.isfinite(s).all()
    assert len(np.unique(s)) == 24
    np.testing.assert_array_equal(s.view(np.uint32).reshape(-1), 0x4B000000 + np.arange(24, dtype=np.uint32))
    assert (ST_FILL, IT_FILL) == (0xAB, -7)


@pytest.mark.parametrize("compare", [assert_same_bits, assert_same], ids=["assert_same_bits", "assert_same"])
def test_bitwise_comparers(compare):
    f, st, it = solve_result()
    compare((f, st, it), (f.copy(), st.copy(), it.copy()))
    with pytest.raises(AssertionError):
        compare((flipped(f, 1, 7), st, it), (f, st, it))           # one mantissa bit
    zero = f.copy()
    zero[0, 3] = 0.0
    neg = zero.copy()
    neg[0, 3] = -0.0
    assert np.array_equal(zero, neg)                                # equal as numbers
    with pytest.raises(AssertionError):
        compare((neg, st, it), (zero, st, it))                      # +0.0 against -0.0
    with pytest.raises(AssertionError):
        compare((f, st, it), (f, st, it + np.array([0, 1], np.int32)))
    with pytest.raises(AssertionError):
        compare((f, np.array([0, 4], np.uint8), it), (f, st, it))


def test_assert_same_rows_and_message():
    f, st, it = solve_result()
    bad = flipped(f, 1, 0)
    assert_same((bad, st, it), (f, st, it), rows=np.array([True, False]))   # the differing row is not selected
    with pytest.raises(AssertionError, match=r"here: forces differ in 1 rows \(first of the selection: \[1\]\)"):
        assert_same((bad, st, it), (f, st, it), label="here")
    with pytest.raises(AssertionError, match="status differ in 1 rows"):
        assert_same((f, np.array([0, 4], np.uint8), it), (f, st, it), rows=np.array([False, True]))


class _Gait:
    """unpack_gait of the two records: instance 0 has legs 0 and 3 in stance, instance 1 leg 2."""

    @staticmethod
    def unpack_gait(recs, N):
        return np.array([[1, 0, 0, 1], [0, 0, 1, 0]], np.uint8)


def test_assert_swing_zero():
    stance = np.repeat(_Gait.unpack_gait(None, 1) != 0, 3, axis=1)
    f = np.where(stance, np.float32(20.0), np.float32(0.0)).astype(np.float32)
    assert_swing_zero(_Gait, None, 1, f)
    f[1, 4] = -0.0                                                  # a signed zero is still zero here
    assert_swing_zero(_Gait, None, 1, f)
    f[1, 4] = 1e-30                                                 # leg 1 of instance 1 swings
    with pytest.raises(AssertionError, match=r"1 nonzero force words on swing legs.*\[\[1, 4\]\]"):
        assert_swing_zero(_Gait, None, 1, f)


def test_assert_due_result():
    ref = solve_result()
    due = np.array([0, 1], np.uint8)
    m = due != 0
    got = (np.where(m[:, None], ref[0], sentinel_forces(B, COLS)), np.where(m, ref[1], ST_FILL).astype(np.uint8),
           np.where(m, ref[2], IT_FILL).astype(np.int32))
    assert_due_result(got, ref, due, COLS)
    assert_due_result(ref, ref, np.array([1, 255], np.uint8), COLS)        # any nonzero byte is due
    with pytest.raises(AssertionError):                                     # a row that is not due lost a force sentinel
        assert_due_result((flipped(got[0], 0, 11), got[1], got[2]), ref, due, COLS)
    with pytest.raises(AssertionError, match="lost their sentinels: status at rows \\[0\\]"):
        assert_due_result((got[0], np.array([0, 0], np.uint8), got[2]), ref, due, COLS)
    with pytest.raises(AssertionError, match="lost their sentinels.*iters at rows \\[0\\]"):
        assert_due_result((got[0], got[1], np.array([0, 5], np.int32)), ref, due, COLS)
    with pytest.raises(AssertionError):                                     # a due row with a wrong status
        assert_due_result((got[0], np.array([ST_FILL, 2], np.uint8), got[2]), ref, due, COLS)
    with pytest.raises(AssertionError):                                     # a due row one mantissa bit off
        assert_due_result((flipped(got[0], 1, 2), got[1], got[2]), ref, due, COLS)
    with pytest.raises(AssertionError, match="the comparator did not write every row"):
        assert_due_result(got, (ref[0], np.array([0, ST_FILL], np.uint8), ref[2]), due, COLS)


class _Handle:
    """What row_by_row needs of a handle: ``close``; ``k`` is its combo, None under the table."""

    def __init__(self, k, log):
        self.k, self.log = k, log

    def close(self):
        self.log.append(("closed", self.k))


def test_row_by_row():
    ids = np.array([1, 0])
    log = []

    def op(table_rows):
        def run(s):   # combo k's row i is (10 k + i, 10 k + i + 0.5); the table handle gives table_rows
            k = np.asarray(table_rows if s.k is None else [s.k] * B, np.float32)
            x = 10 * k + np.arange(B, dtype=np.float32)
            return np.stack([x, x + 0.5], 1), x.astype(np.int32)
        return run

    got, want, outs = row_by_row(op(ids), lambda k: _Handle(k, log), lambda: _Handle(None, log), ids, 2)
    assert log == [("closed", 0), ("closed", 1), ("closed", None)]          # every handle, the table's last
    assert len(outs) == 2 and isinstance(want, tuple)
    np.testing.assert_array_equal(want[0], np.float32([[10, 10.5], [1, 1.5]]))
    np.testing.assert_array_equal(want[1], [10, 1])
    assert_same_bits(got, want)
    got, want, _ = row_by_row(op([1, 1]), lambda k: _Handle(k, log), lambda: _Handle(None, log), ids, 2)
    with pytest.raises(AssertionError):                                      # row 1 took combo 1's values, not combo 0's
        assert_same_bits(got, want)
    with pytest.raises(AssertionError, match="rows_of: 3 ids"):             # one id per row
        rows_of(outs, np.array([1, 0, 1]))
    np.testing.assert_array_equal(bits(rows_of([o[0] for o in outs], ids)), bits(want[0]))   # an array per combo

"""tests/guard.py on numpy alone: a stand-in "launch" that keeps the operator contract passes check(), and each of the three ways a
tile kernel breaks it -- a store to row M of a column, to column N, to the word in front of the buffer -- makes check() fail with the
offending position. (What the guard is for on the device: tests/test_gpu_op_contract.py.)"""
import numpy as np
import pytest

import guard

M, N = 37, 5                      # dst[n * ldd + m]: N columns of M rows, so the guard's "rows" are the N columns
VAL = np.float32(2.5)


def _launch(buf, off, ldd, rows_m, cols_n):
    """a tile kernel's store loop WITHOUT its `if (n < N && m < M)`: it writes rows [0, rows_m) of columns [0, cols_n)"""
    for n in range(cols_n):
        for m in range(rows_m):
            buf[off + n * ldd + m] = (VAL + np.float32(n * 1000 + m)).view(np.uint32)


def _run(ldd, rows_m=M, cols_n=N, before=False):
    gd = guard.Guard(N, M, ldd)
    buf = gd.image()
    assert buf.size == guard.FRONT + N * ldd + (128 - N) * ldd + 128
    _launch(buf, gd.offset, ldd, rows_m, cols_n)
    if before:
        buf[gd.offset - 1] = VAL.view(np.uint32)
    return gd, buf


@pytest.mark.parametrize("ldd", [M, M + 67])
def test_a_launch_that_keeps_the_contract_passes(ldd):
    gd, buf = _run(ldd)
    got = gd.check(buf)
    assert got.shape == (N, M) and got.dtype == np.float32
    assert np.array_equal(got, VAL + (np.arange(N, dtype=np.float32)[:, None] * 1000 + np.arange(M, dtype=np.float32)[None, :]))


def test_a_store_to_row_M_is_caught():
    gd, buf = _run(M + 67, rows_m=M + 1)
    with pytest.raises(guard.GuardError, match=r"\(row 0, column 37\)"):
        gd.check(buf)
    # ldd == M: rows M of columns 0 .. N-2 land on the next column's payload (its owner overwrote them: nothing to see there),
    # the last column's lands in the back guard
    gd, buf = _run(M, rows_m=M + 1)
    with pytest.raises(guard.GuardError, match=r"\(row 5, column 0\)"):
        gd.check(buf)


@pytest.mark.parametrize("ldd", [M, M + 67])
def test_a_store_to_column_N_is_caught(ldd):
    gd, buf = _run(ldd, cols_n=N + 1)
    with pytest.raises(guard.GuardError, match=r"\(row 5, column 0\)"):
        gd.check(buf)


@pytest.mark.parametrize("ldd", [M, M + 67])
def test_a_store_in_front_of_the_buffer_is_caught(ldd):
    gd, buf = _run(ldd, before=True)
    with pytest.raises(guard.GuardError, match=r"\(row -1, column %d\)" % (ldd - 1)):
        gd.check(buf)


def test_fill_patterns():
    """outputs: a NaN compared by its bits (NaN != NaN as floats); inputs: 1e30, finite, so that fmaxf keeps it"""
    assert np.isnan(np.array([guard.NAN_BITS], np.uint32).view(np.float32)[0])
    gd = guard.Guard(3, 4, 9)
    assert np.isnan(gd.check(gd.image())).all()              # an untouched output: all NaN, and no guard error
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    gi = guard.Guard(3, 4, 9, guard.GAP_IN_BITS, x)
    im = gi.image()
    assert np.array_equal(gi.check(im), x)
    body = im[guard.FRONT:guard.FRONT + 27].reshape(3, 9).view(np.float32)
    assert (body[:, 4:] == np.float32(1e30)).all() and im.view(np.float32)[0] == np.float32(1e30)
    # a store of the fill VALUE into a gap is not a change; any other NaN is
    im2 = gd.image()
    im2[guard.FRONT + 5] = np.uint32(0x7FC00000)
    with pytest.raises(guard.GuardError, match=r"\(row 0, column 5\)"):
        gd.check(im2)

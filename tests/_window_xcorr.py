"""Shared by the window cross-correlation tests: rows that have a lead/lag structure, the scale,
and the exact comparison against rocmdash.ops.window_xcorr.window_xcorr_reference."""

import numpy as np

AXIS = 100.0


def scale(S):
    return np.full(S, np.float32(4095.0 / AXIS), np.float32)


def rows(seed, S, n, nan=0.0):
    """[S, n] float32: one noisy square wave (period 23) between about 20 and 80 of an axis of
    100, series s delayed by 3 s rows and every third series inverted, a few samples below 0 and
    above the axis, ``nan`` of them NaN."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.stack([np.where(((t - 3 * s) % 23) < 13, 80.0, 20.0) for s in range(S)]).astype(np.float32)
    x[2::3] = np.float32(AXIS) - x[2::3]
    x += rng.normal(0, 9, (S, n)).astype(np.float32)
    x[rng.random((S, n)) < 0.01] = np.float32(-3.5)
    x[rng.random((S, n)) < 0.01] = np.float32(117.25)
    if nan:
        x[rng.random((S, n)) < nan] = np.nan
    return x


def assert_xcorr(got, x, pairs, sc, L, span=None, what=""):
    """``got`` [K, 2L + 1, 6] equals the reference over the rows ``x`` [S, n], exactly, and no word
    was left at the -1 the buffer was filled with. Returns the reference."""
    from rocmdash.ops.window_xcorr import window_xcorr_reference

    want = window_xcorr_reference(np.ascontiguousarray(x.T), pairs, sc, L, span)
    assert got.shape == want.shape and got.dtype == np.int64, what
    assert (got >= 0).all(), f"{what}: {np.count_nonzero(got < 0)} words unwritten or negative"
    bad = np.argwhere(got != want)
    assert not len(bad), (f"{what}: {len(bad)} words differ, first (pair, index, word) = {bad[0].tolist()}: "
                          f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
    return want


def assert_mirror(ab, ba, what=""):
    """(b, a) at lag k is (a, b) at lag -k with Sx <-> Sy and Sxx <-> Syy."""
    np.testing.assert_array_equal(ba, ab[::-1][:, [0, 2, 1, 3, 5, 4]], err_msg=what)

"""Shared by the window period trend's tests: the data generator of the autocorrelation tests,
the scale, and the exact comparison against the reference."""

import numpy as np

AXIS = 100.0


def rows(seed, S, n, nan=0.0):
    """[S, n] float32: a noisy square wave per series (period 7 + 6 s) between about 20 and 80 of
    an axis of 100, a few samples below 0 and above the axis, ``nan`` of them NaN."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.stack([np.where((t % (7 + 6 * s)) < 0.6 * (7 + 6 * s), 80.0, 20.0) for s in range(S)]).astype(np.float32)
    x += rng.normal(0, 9, (S, n)).astype(np.float32)
    x[rng.random((S, n)) < 0.01] = np.float32(-3.5)
    x[rng.random((S, n)) < 0.01] = np.float32(117.25)
    if nan:
        x[rng.random((S, n)) < nan] = np.nan
    return x


def scale(S):
    return np.full(S, np.float32(4095.0 / AXIS), np.float32)


def assert_periods(got, x, head, window, P, L, span, what=""):
    """``got`` [S, P + 1, L + 1, 4] against the reference over ``x`` [S, n], rows ``head - n ..
    head - 1``; returns the reference."""
    from rocmdash.ops.window_periods import window_periods_reference

    got = np.asarray(got)
    want = window_periods_reference(x.T, scale(len(x)), head, window, P, L, span)
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, got.dtype, want.shape)
    if not np.array_equal(got, want):
        s, j, k, i = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError(f"{what} n {x.shape[1]} head {head} P {P} L {L} span {span}: {np.count_nonzero(got != want)} "
                             f"words differ, first series {s} slot {j} lag {k} word {i}: {got[s, j, k, i]} != {want[s, j, k, i]}")
    return want

"""The exact sorted-fp32 oracle (tests/_exact.py) itself: it repeats the host-compiled rules
bit for bit, it is numpy's 'linear' percentile, a rank shifted by one fails it where the
suite's older ``rtol=1e-5, atol=1e-4`` does not, and the host models that mirror the
kernels satisfy it on the inputs of their own tests."""

import numpy as np
import pytest

import _exact
from _exact import assert_exact, exact_stats, expected_comparisons

TRIOS = [(50, 90, 99), (0, 100, 50), (0.1, 99.9, 37.5), (5, 25, 75)]


@pytest.fixture(scope="module")
def nat():
    from rocmdash.runtime import native

    return native.load(with_torch=False)  # a build that does not load is an error here, not a skip


# ---- agreement with the host rules ---------------------------------------------------------
@pytest.mark.parametrize("trio", TRIOS)
def test_positions_and_values_equal_the_host_rules(nat, trio):
    rng = np.random.default_rng(3)
    compared = 0
    for nv in list(range(1, 131)) + [1000, 4097, 32768, 1 << 20]:
        pos, frac = _exact.positions(nv, trio)
        idx, hfrac = nat.ws_wanted_positions(nv, [float(p) for p in trio])
        assert idx[0] == 0 and idx[1] == nv - 1
        assert list(idx[2:]) == pos, (nv, trio)
        assert np.array_equal(np.array(hfrac, np.float32).view(np.uint32), frac.view(np.uint32)), (nv, trio)
        for gen in (lambda: rng.normal(100, 20, nv), lambda: rng.normal(0, 1, nv) * 10.0 ** rng.uniform(-30, 30, nv)):
            x = gen().astype(np.float32)[:, None]
            ex = exact_stats(x, trio)
            for q in range(3):
                host = np.float32(nat.ws_percentile_between(float(ex.x0[0, q]), float(ex.x1[0, q]), float(frac[q])))
                assert host.view(np.uint32) == ex.percentile[0, q].view(np.uint32), (nv, trio, q)
                compared += 1
    assert compared == 134 * 2 * 3


# ---- agreement with numpy ------------------------------------------------------------------
@pytest.mark.parametrize("trio", TRIOS)
def test_same_definition_as_numpy_linear(trio):
    """Within 2 fp32 ulp of np.percentile on the float64 copy, at the percentile the kernels
    are given (a float: 99.9 is 99.90000152...; numpy keeps the weight between the two
    order statistics in fp64, the kernels round it to fp32)."""
    rng = np.random.default_rng(17)
    for n in (1, 2, 3, 7, 64, 65, 1000, 4097, 32768):
        x = np.stack([rng.normal(100, 20, n), rng.normal(100, 0.01, n), rng.integers(0, 6, n).astype(float),
                      rng.normal(-3, 1, n), np.abs(rng.normal(0, 1, n)) * 10.0 ** rng.uniform(-30, 30, n)],
                     axis=1).astype(np.float32)
        x[rng.random(x.shape) < 0.03] = np.nan
        ex = exact_stats(x, trio)
        for s in range(x.shape[1]):
            v = x[:, s][~np.isnan(x[:, s])]
            if not len(v):
                continue
            ref = np.percentile(v.astype(np.float64), [float(np.float32(p)) for p in trio]).astype(np.float32)
            ulps = np.abs(ex.percentile[s].astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref))
            assert np.all(ulps <= 2), (n, s, trio, ex.percentile[s], ref)
            assert ex.min[s] == v.min() and ex.max[s] == v.max() and ex.count[s] == len(v)
            assert np.array_equal(ex.sorted[s], np.sort(v))


def test_key_order_and_edges():
    x = np.array([[0.0], [-0.0], [np.nan], [1.4e-45], [-1.4e-45], [np.inf], [-np.inf], [0.0], [-0.0]], np.float32)
    ex = exact_stats(x, (0, 50, 100))
    want = np.array([-np.inf, -1.4e-45, -0.0, -0.0, 0.0, 0.0, 1.4e-45, np.inf], np.float32)
    assert np.array_equal(ex.sorted[0].view(np.uint32), want.view(np.uint32))  # -0.0 before +0.0
    assert ex.nv[0] == 8 and np.signbit(ex.last[0]) and ex.min[0] == -np.inf and ex.max[0] == np.inf
    empty = exact_stats(np.full((5, 2), np.nan, np.float32), (50, 90, 99))
    got = np.full((2, 8), np.nan, np.float32)
    got[:, 7] = 0
    assert assert_exact(got, empty, (50, 90, 99), sum_group=1) == 16
    got[1, 1] = 0.0  # a statistic with no valid sample
    with pytest.raises(AssertionError):
        assert_exact(got, empty, (50, 90, 99), sum_group=1)


def test_assert_exact_counts_and_conditions():
    rng = np.random.default_rng(2)
    x = _exact.family_rows(rng, 0, 1000, 1000, blips=(5,))
    pct = (50, 90, 99)
    ex = exact_stats(x, pct)
    out = ex.output()
    assert assert_exact(out, x, pct, sum_group=1, skip_nonfinite=(_exact.INF_SERIES,)) == expected_comparisons(15, skipped=1)
    assert assert_exact(out, ex, pct, sum_group=8, last=False,
                        skip_nonfinite=(_exact.INF_SERIES,)) == expected_comparisons(15, last=False, skipped=1)
    # a series named in skip_nonfinite whose values are all finite is checked in full
    assert assert_exact(out[:4], exact_stats(x[:, :4], pct), pct, sum_group=1, skip_nonfinite=(0,)) == 32
    with pytest.raises(AssertionError):  # the +-inf series has no finite mean: not skipped, not passed
        assert_exact(out, ex, pct, sum_group=1)
    with pytest.raises(AssertionError):
        assert_exact(out, ex, (50, 90, 98), sum_group=1, skip_nonfinite=(_exact.INF_SERIES,))
    for col, s in ((0, 0), (1, 2), (6, 4), (7, 6), (6, 13)):  # min, max, last, count; last = NaN
        bad = out.copy()
        bad[s, col] = 1.0 if np.isnan(bad[s, col]) else np.nextafter(bad[s, col], np.float32(np.inf))
        with pytest.raises(AssertionError):
            assert_exact(bad, ex, pct, sum_group=1, skip_nonfinite=(_exact.INF_SERIES,))
    bad = out.copy()  # min / max / count of the +-inf series are still checked
    bad[_exact.INF_SERIES, 7] += 1
    with pytest.raises(AssertionError):
        assert_exact(bad, ex, pct, sum_group=1, skip_nonfinite=(_exact.INF_SERIES,))
    # the mean: the bound grows with sum_group, and is a bound
    s = _exact.FAMILIES.index("narrow")
    bad = out.copy()
    bad[s, 2] = np.float32(ex.mean[s] + 4 * 2.0 ** -24 * ex.mean_abs[s])
    assert_exact(bad, ex, pct, sum_group=8, skip_nonfinite=(_exact.INF_SERIES,))
    with pytest.raises(AssertionError):
        assert_exact(bad, ex, pct, sum_group=1, skip_nonfinite=(_exact.INF_SERIES,))
    # one ulp where the kernel interpolates, none where it cannot
    s = _exact.FAMILIES.index("wide")
    assert ex.frac[s, 0] != 0 and ex.x0[s, 0] != ex.x1[s, 0]
    bad = out.copy()
    bad[s, 3] = np.nextafter(out[s, 3], np.float32(np.inf))
    assert_exact(bad, ex, pct, sum_group=1, skip_nonfinite=(_exact.INF_SERIES,))
    bad[s, 3] = np.nextafter(bad[s, 3], np.float32(np.inf))
    with pytest.raises(AssertionError):
        assert_exact(bad, ex, pct, sum_group=1, skip_nonfinite=(_exact.INF_SERIES,))
    s = _exact.FAMILIES.index("ties")
    assert ex.x0[s, 0] == ex.x1[s, 0]
    bad = out.copy()
    bad[s, 3] = np.nextafter(out[s, 3], np.float32(np.inf))
    with pytest.raises(AssertionError):
        assert_exact(bad, ex, pct, sum_group=1, skip_nonfinite=(_exact.INF_SERIES,))


# ---- sensitivity ---------------------------------------------------------------------------
def _shifted_outputs(ex, s):
    """Every output in which ONE of series s's six ranks is off by one (inside the window)."""
    v, nv = ex.sorted[s], int(ex.nv[s])
    for r in range(6):
        for d in (-1, 1):
            p = int(ex.pos[s, r]) + d
            if not 0 <= p < nv:
                continue
            x0, x1 = ex.x0[s].copy(), ex.x1[s].copy()
            (x0 if r % 2 == 0 else x1)[r // 2] = v[p]
            out = ex.output()
            out[s, 3:6] = _exact.percentile_between(x0, x1, ex.frac[s])
            yield r, d, out


def _distinct_at_positions(ex, s):
    """The precondition under which a rank off by one is an error in the VALUE: no equal
    neighbours at or next to a percentile position, both order statistics weigh in, and the
    lighter weight times the smallest gap is over 2.5 fp32 ulp (the final rounding can hide
    half an ulp at either end, the oracle allows one)."""
    v = ex.sorted[s]
    for q in range(3):
        lo, hi = int(ex.pos[s, 2 * q]), int(ex.pos[s, 2 * q + 1])
        f = float(ex.frac[s, q])
        if hi != lo + 1 or lo < 1 or hi + 1 >= len(v) or not 0 < f < 1:
            return False
        w = v[lo - 1:hi + 2].astype(np.float64)
        if min(f, 1 - f) * np.diff(w).min() < 2.5 * np.spacing(np.abs(v[lo - 1:hi + 2])).max():
            return False
    return True


# (family, window, seed): the long window's continuous inputs at 65536. `narrow` is N(100, 0.01),
# ~1300 distinct fp32 values per sigma: 65536 samples tie at every percentile (a rank off by
# one is the same value there, to any oracle), so it is tried at 250 samples, where its
# neighbours are some ten ulp apart. Seeds: the first that meet the asserted precondition.
SENSITIVITY = [("wide", 65536, 0), ("normal", 65536, 0), ("inf", 65536, 2), ("ramp_up", 65536, 0), ("narrow", 250, 25)]


@pytest.mark.parametrize("name,W,seed", SENSITIVITY)
def test_a_rank_off_by_one_fails(name, W, seed):
    pct = (50, 90, 99)
    x = _exact.family(name, np.random.default_rng(seed), 0, W, W)[:, None]
    if name == "inf":  # the order statistics around its percentiles: the +-inf samples aside
        x = np.where(np.isinf(x), np.float32(np.nan), x)
    ex = exact_stats(x, pct)
    assert _distinct_at_positions(ex, 0), "precondition: pick a seed without near-equal neighbours at the positions"
    assert assert_exact(ex.output(), ex, pct, sum_group=8) == 8
    tried = 0
    for r, d, bad in _shifted_outputs(ex, 0):
        with pytest.raises(AssertionError):
            assert_exact(bad, ex, pct, sum_group=8)
        tried += 1
    assert tried == 12


def test_a_rank_off_by_one_passes_the_old_tolerance_at_2_20():
    """N(100, 20) at W = 2^20: every one of the twelve shifted outputs passes
    ``assert_allclose(rtol=1e-5, atol=1e-4)`` against the true one and fails the oracle."""
    pct = (50, 90, 99)
    W = 1 << 20
    x = np.random.default_rng(9).normal(100, 20, W).astype(np.float32)[:, None]
    ex = exact_stats(x, pct)
    assert _distinct_at_positions(ex, 0), "precondition: pick a seed without near-equal neighbours at the positions"
    good = ex.output()
    tried = 0
    for r, d, bad in _shifted_outputs(ex, 0):
        np.testing.assert_allclose(bad, good, rtol=1e-5, atol=1e-4)
        with pytest.raises(AssertionError):
            assert_exact(bad, ex, pct, sum_group=8)
        tried += 1
    assert tried == 12


# ---- the host models -------------------------------------------------------------------------
def _pad(cols):
    """Series of unequal lengths as one [n, S] array (NaN = no sample), newest last."""
    n = max(1, max(len(c) for c in cols))
    x = np.full((n, len(cols)), np.nan, np.float32)
    for s, c in enumerate(cols):
        if len(c):
            x[n - len(c):, s] = c
    return x


@pytest.mark.parametrize("case", ["steady", "nan_spikes_4", "nan_spikes_5", "incremental_telemetry",
                                  "incremental_mixed", "tied_boundary"])
def test_bracket_model_is_exact(case):
    """rocmdash/runtime/lw_brackets.py BracketModel on the inputs of tests/test_lw_brackets.py."""
    from rocmdash.runtime.lw_brackets import PCT, BracketModel

    incremental = case.startswith("incremental") or case == "tied_boundary"
    if case == "steady":
        rng = np.random.default_rng(1)
        W = 1 << 16
        x = rng.normal(50, 10, 3 * W).astype(np.float32)
        steps = [W] + [1, 3, 0, 100, 1, 7, 1, 1, 50, 1] * 2
    elif case.startswith("nan_spikes"):
        rng = np.random.default_rng(int(case[-1]))
        W = 4096
        x = rng.normal(0, 1, 6 * W).astype(np.float32)
        x[rng.random(x.size) < 0.01] = -1e6
        x[W:W + 700] = np.nan
        steps = [W] + list(rng.choice([0, 1, 5, 64, 257, 700], size=30))
    elif case == "tied_boundary":
        W = 1 << 18
        x = np.random.default_rng(3).integers(40, 56, W + 100 * 20).astype(np.float32)
        steps = [W] + [100] * 20
    else:
        rng = np.random.default_rng(9)
        W = 1 << 15
        x = (rng.integers(40, 56, 3 * W) if case.endswith("telemetry") else rng.normal(0, 10, 3 * W)).astype(np.float32)
        steps = [W] + [100] * 60
    m = BracketModel(incremental=incremental)
    t, hits, compared = 0, 0, 0
    for i, k in enumerate(steps):
        t += int(k)
        w = x[max(0, t - W):t]
        got, hit = m.refresh(w, entered=int(k) if i else None)
        compared += assert_exact(got[None, :], w[:, None], PCT, sum_group=1)
        hits += bool(hit)
    assert compared == 8 * len(steps)
    assert hits > 0 or case == "nan_spikes_5" or not incremental  # both of the model's paths were under the oracle


def test_adaptive_digit_model_is_exact():
    """The adaptive-digit model of tests/test_long_window_model.py on its own inputs: its
    six selected ranks, min and max make the oracle's output."""
    from test_long_window_model import _GENS, _keys, _select

    pct = (50, 90, 99)
    compared = 0
    for shape in sorted(_GENS):
        rng = np.random.default_rng(7)
        for trial in range(12):
            n = int(rng.integers(1, 3000))
            x = _GENS[shape](rng, n).astype(np.float32)
            x[rng.random(n) < 0.05] = np.nan
            v = x[~np.isnan(x)]
            if len(v) == 0:
                continue
            k = _keys(v)
            if trial % 3 == 0:
                pmin, pmax, plo = 0, 0xFFFFFFFF, 0
            else:
                pmin, pmax = int(k.min()), int(k.max())
                o = int(np.bitwise_or.reduce(k ^ k[0]))
                plo = (o & -o).bit_length() - 1 if o else 32
            pos, frac = _exact.positions(len(v), pct)
            sel, _ = _select(x, [0, len(v) - 1] + pos, pmin, pmax, plo, int(k[trial % len(k)]))
            out = np.full((1, 8), np.nan, np.float32)
            out[0, 0], out[0, 1] = sel[0], sel[1]
            out[0, 2] = np.float32(np.sum(v, dtype=np.float64) / len(v))
            out[0, 3:6] = _exact.percentile_between(sel[2::2], sel[3::2], frac)
            out[0, 6], out[0, 7] = x[-1], len(v)
            skip = (0,) if shape == "heavy_tail" else ()  # float32(cauchy * 1e6) may overflow to inf
            ex = exact_stats(x[:, None], pct)
            assert np.isfinite(ex.mean[0]) or skip
            compared += assert_exact(out, ex, pct, sum_group=1, skip_nonfinite=skip)
    assert compared >= 8 * 7 * 10


@pytest.mark.parametrize("N,W", [(8, 1000), (3, 4096), (8, 8192)])
def test_node_window_reference_is_exact(N, W):
    """``node_window_reference`` interpolates with numpy: the 1-ulp rule, on the inputs of
    test_node_select_kernel_matches_reference."""
    from rocmdash.parallel.node_window import node_window_reference

    rng = np.random.default_rng(N * W)
    S = 6
    node = np.full((N, S, W + 1), np.inf, np.float32)
    for i in range(N):
        for s in range(S):
            c = [0, W, 1, int(rng.integers(0, W)), W // 2, W][s] if i % 3 else W
            if s == 0 and i == 0:
                c = 0
            v = rng.integers(0, 20, c).astype(np.float32) if s % 2 else rng.normal(50 * (i + 1), 5, c).astype(np.float32)
            node[i, s, 0] = c
            node[i, s, 1: 1 + c] = np.sort(v)
    ref = node_window_reference(node).astype(np.float32)
    x = _pad([np.concatenate([node[i, s, 1: 1 + int(node[i, s, 0])] for i in range(N)]) for s in range(S)])
    assert assert_exact(ref, x, (50.0, 90.0, 99.0), sum_group=1, last=False) == expected_comparisons(S, last=False)
    assert np.isnan(ref[:, 6]).all()


@pytest.mark.parametrize("ranks", [1, 3, 8])
def test_node_radix_model_is_exact(ranks):
    """rocmdash.parallel.node_radix on the inputs of tests/test_node_radix.py."""
    from test_node_radix import PCT, _data, _run

    rng = np.random.default_rng(ranks)
    xs = _data(rng, ranks, 3000)
    out = _run(xs)[0]
    x = _pad([np.concatenate([x[s][~np.isnan(x[s])] for x in xs]) for s in range(7)])
    ex = exact_stats(x, PCT)
    skip = () if np.isfinite(ex.mean[4]) else (4,)  # the heavy tail may overflow float32
    assert assert_exact(out, ex, PCT, sum_group=1, last=False,
                        skip_nonfinite=skip) == expected_comparisons(7, last=False, skipped=len(skip))
    assert np.isnan(out[:, 6]).all()

"""The pure rules of the window-stats kernel (csrc/window_stats_rules.h): the incremental-step
predicate, the half rule, the changed span, the one-in/one-out mapping, the percentile
positions and the launch shape. Integer and fp64 arithmetic, checked here without a GPU
through thin bindings: the kernel and DeviceWindowSet run the same functions."""

import itertools

import numpy as np
import pytest

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def nat():
    from rocmdash.runtime import native

    return native.load(with_torch=False)  # a build that does not load is an error here, not a skip


# ---- incremental step: previous window [h0 - n0, h0) in half cur, this launch [h1 - n1, h1)
def _step(nat, h0=5000, n0=1000, cur=0, h1=5000, n1=1000, depth=2048, cap=1024):
    return nat.ws_incremental_step(h0, n0, cur, h1, n1, depth, cap)


def test_incremental_step_accepts_up_to_256_rows_either_end(nat):
    assert nat.MAX_INCREMENTAL == 256
    assert _step(nat, h1=5256, n1=1000) == (True, 256, 256)
    assert _step(nat, h1=5257, n1=1001) == (False, 0, 0)  # kadd 257, krem 256
    assert _step(nat, h1=5256, n1=999) == (False, 0, 0)  # kadd 256, krem 257
    assert _step(nat, h1=5256, n1=1024) == (True, 256, 232)
    assert _step(nat) == (True, 0, 0)
    for kadd, n1 in itertools.product(range(0, 257, 64), (990, 1000, 1010)):
        h0, n0, h1 = 5000, 1000, 5000 + kadd
        krem = (h1 - n1) - (h0 - n0)
        ok = 0 <= krem <= 256
        assert _step(nat, h1=h1, n1=n1) == ((True, kadd, krem) if ok else (False, 0, 0))


def test_incremental_step_refusals(nat):
    assert _step(nat, h1=4999, n1=999)[0] is False  # head moved backwards
    assert _step(nat, h1=5000, n1=1001)[0] is False  # window start moved backwards
    assert _step(nat, cur=2)[0] is False
    assert _step(nat, h0=900, n0=1000, h1=900, n1=900)[0] is False  # n0 > h0
    assert _step(nat, n0=1025, n1=1000, h1=5025)[0] is False  # n0 above sorted_cap
    assert _step(nat, n1=1025, h1=5025)[0] is False  # n1 above sorted_cap
    assert _step(nat, n0=1024, n1=1024) == (True, 0, 0)  # at the cap
    # the leaving rows must still be in the device ring: s0 + depth >= h1
    assert _step(nat, h1=5100, n1=1000, depth=1100) == (True, 100, 100)  # s0 + depth == h1
    assert _step(nat, h1=5100, n1=1000, depth=1099)[0] is False


def test_next_half(nat):
    assert [nat.ws_next_half(True, True, c) for c in (0, 1)] == [0, 1]  # incremental keeps cur
    assert [nat.ws_next_half(False, True, c) for c in (0, 1)] == [1, 0]  # a full sort takes the other
    assert [nat.ws_next_half(False, False, c) for c in (0, 1)] == [0, 0]  # no state: half 0


# ---- changed span and one-row mapping against brute force
def _upper(w, v):
    return sum(1 for x in w if x <= v)


def test_one_row_mapping_and_span_brute_force(nat):
    for n in range(0, 9):
        for old in itertools.combinations_with_replacement((0, 1, 2), n):
            old = list(old)
            for leave in [None] + sorted(set(old)):
                for enter in (None, -1, 0, 1, 2, 3):
                    kr, ka = int(leave is not None), int(enter is not None)
                    lpos = _upper(old, leave) - 1 if kr else 0  # the end of its run
                    ins = _upper(old, enter) if ka else 0
                    x, pn = nat.ws_one_row_map(kr, ka, lpos, ins)
                    nv = n - kr + ka
                    new = [enter if p == pn else old[nat.ws_one_row_src(x, pn, p)] for p in range(nv)]
                    rest = old[:lpos] + old[lpos + 1:] if kr else old
                    assert new == sorted(rest + ([enter] if ka else [])), (old, leave, enter)
                    lo, hi = nat.ws_changed_span(kr, ka, x, x, ins, ins, nv)
                    for p in range(min(n, nv)):
                        if not lo <= p < hi:
                            assert new[p] == old[p], (old, leave, enter, lo, hi, p)
                    if nv > n:  # the window grew: its new last position is inside the span
                        assert lo <= nv - 1 < hi


def test_changed_span_many_samples(nat):
    rng = np.random.default_rng(11)
    for _ in range(3000):
        n = int(rng.integers(0, 11))
        old = sorted(rng.integers(0, 4, n).tolist())
        kr = int(rng.integers(0, min(3, n) + 1))
        ka = int(rng.integers(0, 4))
        leaving = sorted(rng.choice(old, kr, replace=False).tolist()) if kr else []
        entering = sorted(rng.integers(-1, 5, ka).tolist())
        # leaving sample j of c equal ones sits at upper_bound - c + j: the end of its run
        prem = []
        for j, v in enumerate(leaving):
            c = sum(1 for u in leaving[j:] if u == v)
            prem.append(_upper(old, v) - c)
        qins = [_upper(old, v) for v in entering]
        kept = [v for i, v in enumerate(old) if i not in prem]
        new = sorted(kept + entering)
        assert sorted(old[i] for i in prem) == leaving
        nv = len(new)
        lo, hi = nat.ws_changed_span(kr, ka, prem[0] if kr else 0, prem[-1] if kr else 0, qins[0] if ka else 0,
                                     qins[-1] if ka else 0, nv)
        for p in range(nv):
            if p >= n or new[p] != old[p]:
                assert lo <= p < hi, (old, leaving, entering, lo, hi, p)
        if kr == ka:  # the tight bound: one past the last leaving position or the last insertion point
            want = max(prem[-1] + 1 if kr else 0, qins[-1] if ka else 0)
            assert hi == min(want, nv)
        else:
            assert hi == nv


# ---- positions and interpolation
def _close(got, ref, rtol=1e-5, atol=1e-4):
    return abs(got - ref) <= atol + rtol * abs(ref)


def test_positions_and_interpolation_match_numpy(nat):
    rng = np.random.default_rng(5)
    for nv in range(0, 10):
        x = np.sort(rng.normal(100, 20, nv).astype(np.float32))
        for trio in ((0, 1, 50), (90, 99, 100)):
            idx, frac = nat.ws_wanted_positions(nv, [float(p) for p in trio])
            if nv == 0:
                assert idx == [0] * 8
                continue
            assert idx[0] == 0 and idx[1] == nv - 1
            assert all(i < nv for i in idx)
            for q, pct in enumerate(trio):
                got = nat.ws_percentile_between(float(x[idx[2 + 2 * q]]), float(x[idx[3 + 2 * q]]), frac[q])
                ref = float(np.percentile(x.astype(np.float64), pct, method="linear"))
                assert _close(got, ref), (nv, pct, got, ref)


# ---- launch configuration: the two tables the launcher used to hold
STEADY_FEW = {512: (256, 2), 1024: (256, 4), 2048: (512, 4), 4096: (512, 8), 8192: (512, 16)}
STEADY_MORE = {512: (256, 2), 1024: (256, 4), 2048: (512, 4), 4096: (1024, 4), 8192: (1024, 8)}
PLAIN = {64: (64, 1), 128: (128, 1), 256: (256, 1), 512: (512, 1), 1024: (1024, 1), 2048: (1024, 2), 4096: (1024, 4),
         8192: (1024, 8), 16384: (1024, 16), 32768: (1024, 32)}


def test_launch_shape_tables(nat):
    small_k = 2
    for w, plain in PLAIN.items():
        assert nat.ws_launch_shape(w, False, 1, small_k) == plain
        assert nat.ws_launch_shape(w, False, NONE, small_k) == plain
        for rows in (0, 1, 2):
            assert nat.ws_launch_shape(w, True, rows, small_k) == STEADY_FEW.get(w, plain), (w, rows)
        for rows in (3, 10, 256, NONE):
            assert nat.ws_launch_shape(w, True, rows, small_k) == STEADY_MORE.get(w, plain), (w, rows)
        assert nat.ws_launch_shape(w, True, 3, 3) == STEADY_FEW.get(w, plain)  # the threshold moves with small_k
        for inc, rows in itertools.product((False, True), (1, 300)):
            nt, e = nat.ws_launch_shape(w, inc, rows, small_k)
            assert nt * e == w
    for w in (0, 1, 32, 63, 65, 96, 1000, 4097, 65536, 1 << 31):
        for inc in (False, True):
            assert nat.ws_launch_shape(w, inc, 1, small_k) == (0, 0), w
    assert nat.sort_width_for(1) == 64 and nat.sort_width_for(65) == 128 and nat.sort_width_for(32768) == 32768

"""Without a GPU: the inputs of test_gpu_window_heatmap_bounds.py and
test_gpu_window_joint_bounds.py need the walk. The two kernels (csrc/window_heatmap.hip,
csrc/window_joint.hip) hold private copies of the streaming le-bucket kernel's bin rule; the
GPU tests assert, launch by launch, that the walking bounds families of tests/_bucket_bounds.py
walk on the samples of the window itself. Here the same inputs are built and held to the same
preconditions, and the families to the fp32 model of the guess at the sizes those tests use."""

import numpy as np
import pytest

import _bucket_bounds as bb
from _bucket_bounds import _launch_inputs, _shifts, _walkers, _windows

WAVE_SLOT_FLOATS = 2048  # csrc/window_heatmap.hip kWaveSlotFloats: a larger slot takes eight waves
RINGS = sorted({(d, s, c) for d, s, c, _, _ in bb.HEATMAP_RINGS} | set(bb.JOINT_RINGS))


def test_heatmap_rings_reach_both_kernels():
    floats = [stride * c for _, stride, _, _, c in bb.HEATMAP_RINGS]
    assert [f <= WAVE_SLOT_FLOATS for f in floats] == [True, True, True, True, False, False]
    for depth, stride, cols, P, c in bb.HEATMAP_RINGS:
        assert P * c == depth and 1 <= cols <= stride <= 64
        kind, head, n = _windows(depth)[2]
        assert n == depth and head % c != 0  # the full window: P + 1 slots, the oldest and the newest partial


@pytest.mark.parametrize("depth,stride,cols", RINGS)
def test_every_launch_of_the_gpu_tests_needs_the_walk(depth, stride, cols):
    """Every (ring, B >= 16, launch, window of more than one row) of the two GPU tests: each
    walking family among the columns that visit every bin meets ``walks_enough`` on the window's
    own samples (``_walkers`` asserts it), over a ring's launches every walking family is met,
    neighbouring columns hold different families, and the NaN launches are every second one."""
    Bs = sorted({B for B in bb.HEATMAP_B if (depth, stride, cols) in {r[:3] for r in bb.HEATMAP_RINGS}} |
                {B for B in bb.JOINT_B if (depth, stride, cols) in bb.JOINT_RINGS})
    shifts = _shifts(cols)
    assert len(shifts) >= 2
    met = {((c + o) % bb.F, (c + s) % bb.NS) for o, s in shifts for c in range(cols)}
    assert len(met) == bb.F * bb.NS  # every bounds family meets every sample family
    for B in (B for B in Bs if B >= 16):
        walked = set()
        for i, (o, s) in enumerate(shifts):
            clean, rows, bounds, names = _launch_inputs(depth, stride, cols, B, i, o, s)
            assert cols == 1 or names[0][0] != names[1][0]
            added = np.isnan(rows) & ~np.isnan(clean)
            assert (rows[~added].view(np.uint32) == clean[~added].view(np.uint32)).all()
            for c, (_, kind) in enumerate(names):
                assert added[:, c].any() == (i % 2 == 1 and kind != "exact"), (i, c, kind)
            assert not added[:, cols:].any()
            for kind, head, n in _windows(depth):
                assert n == 1 or n >= 256
                if n > 1:
                    walked |= _walkers(clean, bounds, names, head, n)
        assert walked == set(bb.WALKS), (B, walked)


@pytest.mark.parametrize("B", [16, 31, 63])
@pytest.mark.parametrize("n", [256, 512, 1024])
def test_walking_families_walk_at_the_sizes_the_gpu_tests_use(n, B):
    """``_bucket_bounds.column`` at n rows: every walking family against ``hop``, ``stairs`` and
    ``beside``, over the whole column and over its newer half."""
    for name in bb.WALKS:
        for j, kind in enumerate(bb.VISIT_EVERY_BIN):
            b, x = bb.column(np.random.default_rng(n + B + j), name, kind, j, n, B)
            assert b.shape == (B,) and x.shape == (n,)
            for part in (x, x[n // 2:]):
                assert bb.walks_enough(name, part, b), (name, kind, len(part), bb.walk_reached(part, b))


@pytest.mark.parametrize("B", [1, 2, 3, 16, 31, 63])
def test_static_families_are_bounds_for_both_kernels(B):
    from rocmdash.ops.window_buckets import check_bounds
    from rocmdash.ops.window_joint import MAX_JOINT_BUCKETS, check_joint_bounds

    b = np.stack([f(B) for f in bb.STATIC.values()])
    np.testing.assert_array_equal(check_bounds(b, len(bb.STATIC)), b)
    if B <= MAX_JOINT_BUCKETS:
        np.testing.assert_array_equal(check_joint_bounds(b, len(bb.STATIC)), b)
    else:
        with pytest.raises(ValueError):
            check_joint_bounds(b, len(bb.STATIC))


def test_with_nans_replaces_a_share_and_nothing_else():
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, 4096).astype(np.float32)
    x[::7] = np.inf
    y = bb.with_nans(rng, x, 0.05)
    assert y is not x and y.dtype == np.float32 and not np.isnan(x).any()
    gone = np.isnan(y)
    assert 0.03 * len(x) < gone.sum() < 0.07 * len(x)
    np.testing.assert_array_equal(y[~gone], x[~gone])
    assert not np.isnan(bb.with_nans(rng, x, 0.0)).any()

"""The window period trend kernel (csrc/window_periods.hip) against the numpy reference of
rocmdash.ops.window_periods (itself checked against a triple loop in test_window_periods.py):
ring widths, lag counts and lag blocks in both epilogues, every slot edge, the ring wrap, NaN
patterns, the largest sums, the argument checks, and DeviceWindowSet / LongWindowSet through
GpuAgent.

The sums are integers: every comparison is exact equality. Every buffer is filled with -1 or
garbage before the call that writes it, so a word the kernel left out shows."""

import os

import numpy as np
import pytest

from _window_periods import assert_periods as _check, rows as _rows, scale as _scale

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURE = os.path.join(ROOT, "tests", "fixtures", "mi355x_capture.npz")


def _run(cuda, x, P, L, span, head=None, window=None, split=0, fill=-1):
    import torch

    from rocmdash.ops.window_periods import window_periods

    S = len(x)
    out = torch.full((S, P + 1, L + 1, 4), fill, dtype=torch.int64, device=cuda)
    got = window_periods(torch.from_numpy(x).to(cuda), _scale(S), P, L, span=span, head=head, window=window, out=out, split=split)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("cols,stride", [(1, 4), (5, 8), (16, 19), (61, 64)])
def test_widths(native, cuda, cols, stride):
    """1, 5, 16 and 61 series (a partial group, two full groups, seven and a part) in rings whose
    stride is larger, padding columns holding samples; c = 128, a wrapped window longer than the
    span, 1 % NaN at 5 series."""
    import torch

    span, P, L, W = 1024, 8, 64, 2048
    n = span + 37
    x = _rows(cols * 2000 + L, cols, n, nan=0.01 if cols == 5 else 0.0)
    depth, head = 2 * W, 3 * 2 * W + 500  # the rows wrap the ring
    ring = torch.full((depth, stride), 12345.0, dtype=torch.float32, device=cuda)
    slots = torch.arange(head - n, head, device=cuda, dtype=torch.int64) % depth
    ring[slots, :cols] = torch.from_numpy(x).to(cuda).t()
    sd = torch.from_numpy(_scale(cols)).to(cuda)
    out = torch.full((cols, P + 1, L + 1, 4), -1, dtype=torch.int64, device=cuda)
    native.periods_ring(ring.data_ptr(), stride, cols, depth, head, n, span, P, sd.data_ptr(), L, out.data_ptr(), 0,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check(out.cpu().numpy(), x, head, W, P, L, span, what=f"S {cols} stride {stride}")


@pytest.mark.parametrize("L", [1, 63, 255, 256, 300])
def test_lags_and_lag_blocks_in_both_modes(native, cuda, L):
    """No full tile of lags, a part of a block, one full block, one lag into the second, two
    blocks; c = 2048: two chunks per slot, owned by one workgroup and split between two."""
    span, P = 16384, 8
    x = _rows(L, 3, span - 100, nan=0.002)
    head = 5 * span + 777
    owned = _run(cuda, x, P, L, span, head=head, window=span, split=1)
    halves = _run(cuda, x, P, L, span, head=head, window=span, split=2)
    _check(owned, x, head, span, P, L, span, what="owned")
    np.testing.assert_array_equal(halves, owned)


@pytest.mark.parametrize("head_mod", ["0", "1", "L", "L+1", "c-1"])
def test_slot_edges(native, cuda, head_mod):
    """c = 1024 = the chunk. The newest slot full (the next one empty), of one row, of L rows and of
    L + 1, and one row short of full; for each, no row, one, a slot's worth less, equal and more one,
    the span less one, the span, and more than the span (only the newest span rows count)."""
    from rocmdash.ops.window_periods import periods_geometry

    span, P, L, W = 8192, 8, 70, 16384
    c = span // P
    hm = {"0": 0, "1": 1, "L": L, "L+1": L + 1, "c-1": c - 1}[head_mod]
    head = 4 * W + hm
    for n in (0, 1, c - 1, c, c + 1, span - 1, span, span + 300):
        x = _rows(n + hm, 3, n)
        want = _check(_run(cuda, x, P, L, span, head=head, window=W), x, head, W, P, L, span, what=f"head % c = {head_mod}")
        _, ranges = periods_geometry(head, n, P, span)
        assert int((ranges[:, 1] - ranges[:, 0]).sum()) == min(n, span)
        for j, (b, e) in enumerate(ranges):  # without NaNs n_k == rows_j - k
            assert (want[:, j, :, 0] == np.maximum(int(e - b) - np.arange(L + 1), 0)[None]).all(), (n, j)


@pytest.mark.parametrize("offset", ["c/2", "c", "2c+100", "1", "n-1"])
def test_wrap_position_in_the_rows(native, cuda, offset):
    """The ring wraps ``offset`` rows into the rows: the oldest slot begins half a column, a whole
    one, and 100 rows before the wrap, one row from either end. Columns are anchored to absolute
    rows and a ring at least a column deep wraps on a column boundary, so here the wrap is always a
    slot boundary: the rows before it are one slot's last and the halo of none. L = 200, c = 1024."""
    span, P, L = 8192, 8, 200
    c, n = span // P, span - 300
    o = {"c/2": c // 2, "c": c, "2c+100": 2 * c + 100, "1": 1, "n-1": n - 1}[offset]
    x = _rows(o, 3, n, nan=0.002)
    head = 2 * (2 * span) + n - o  # row 2 x depth is row `o` of x
    _check(_run(cuda, x, P, L, span, head=head, window=span), x, head, span, P, L, span, what=f"wrap at {offset}")


@pytest.mark.parametrize("head", [3 * 512 + 300, 3 * 512 + 1, 3 * 512 + 511, 4 * 512 + 100, 4 * 512])
def test_wrap_inside_a_slot(native, cuda, head):
    """A ring shallower than a column (depth 512, c = 1024) wraps inside a slot: in its middle, one
    row from either end of the rows, with the next slot begun after the wrap (the wrap lies in the
    rows the first slot's halo would reach, and they are not its own), and with no wrap."""
    import torch

    span, P, L, depth, S = 8192, 8, 200, 512, 3
    n = depth
    x = _rows(head, S, n, nan=0.004)
    ring = torch.full((depth, S), float("nan"), dtype=torch.float32, device=cuda)
    ring[torch.arange(head - n, head, device=cuda, dtype=torch.int64) % depth] = torch.from_numpy(x).to(cuda).t()
    sd = torch.from_numpy(_scale(S)).to(cuda)
    out = torch.full((S, P + 1, L + 1, 4), -1, dtype=torch.int64, device=cuda)
    native.periods_ring(ring.data_ptr(), S, S, depth, head, n, span, P, sd.data_ptr(), L, out.data_ptr(), 0,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check(out.cpu().numpy(), x, head, span, P, L, span, what=f"head {head}")


@pytest.mark.parametrize("kind", ["none", "one", "percent", "run", "series", "next_slot"])
def test_validity(native, cuda, kind):
    """No NaN (every chunk takes the prefix-sum path), one NaN and 1 % NaN, a NaN run across a slot
    boundary longer than L, one series all NaN beside valid ones, and a NaN in the first L rows of
    the next slot: it lies in the rows the slot before would load as its halo, is not that slot's,
    and must leave that slot's block what it is without it. L = 300: two lag blocks."""
    from rocmdash.ops.window_periods import periods_geometry

    span, P, L = 8192, 8, 300
    c, n, head = span // P, span, 8 * span + 11
    first = head - n
    edge = (head // c - 3) * c - first  # index of a slot's first row, three slots from the newest
    x = _rows(len(kind), 3, n, nan=0.01 if kind == "percent" else 0.0)
    clean = x.copy()
    if kind == "one":
        x[1, edge + c // 2] = np.nan
    elif kind == "run":
        x[0, edge - 100:edge + L + 57] = np.nan
    elif kind == "series":
        x[1] = np.nan
    elif kind == "next_slot":
        x[2, edge + 5] = np.nan
    got = _run(cuda, x, P, L, span, head=head, window=span)
    want = _check(got, x, head, span, P, L, span, what=kind)
    assert (want[:, :, 0, 0].sum(axis=1) == np.count_nonzero(~np.isnan(x), axis=1)).all()
    if kind == "series":
        assert (want[1] == 0).all() and want[0, 1:, 0].all()
    if kind == "next_slot":
        _, ranges = periods_geometry(head, n, P, span)
        j = int(np.nonzero(ranges[:, 1] == first + edge)[0][0])  # the slot that ends where the NaN's begins
        without = _run(cuda, clean, P, L, span, head=head, window=span)
        np.testing.assert_array_equal(got[:, j], without[:, j])
        assert (got[2, j + 1] != without[2, j + 1]).any()


@pytest.mark.parametrize("split", [1, 8])
def test_largest_sums(native, cuda, split):
    """One series with every sample at or above the axis (q = 4095), columns of 65536 rows: the
    largest sums there are, owned and shared by 8 workgroups, against the closed form."""
    from rocmdash.ops.window_periods import periods_geometry

    span, P, L = 1 << 20, 16, 8
    x = np.full((1, span), np.float32(100.0), np.float32)
    x[0, ::3] = np.inf
    x[0, 1::3] = np.float32(1e30)
    head = 3 * span + 100
    got = _run(cuda, x, P, L, span, head=head, window=span, split=split)
    _, ranges = periods_geometry(head, span, P, span)
    rows_j = (ranges[:, 1] - ranges[:, 0]).astype(np.int64)
    assert rows_j.tolist() == [65536 - 100] + [65536] * 15 + [100]
    nk = np.maximum(rows_j[:, None] - np.arange(L + 1, dtype=np.int64)[None], 0)
    want = np.stack([nk, 4095 * nk, 4095 * nk, 4095 * 4095 * nk], axis=2)[None]
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("split", [1, 2])
def test_overwrites_garbage_and_repeats(native, cuda, split):
    """A destination full of garbage has every word overwritten, and two runs give the same bits."""
    S, span, P, L = 12, 1 << 14, 8, 128
    x = _rows(99, S, span, nan=0.01)
    head = 5 * span - 77
    a = _run(cuda, x, P, L, span, head=head, window=span, split=split, fill=-0x0123456789ABCDEF)
    b = _run(cuda, x, P, L, span, head=head, window=span, split=split, fill=0x7FFFFFFFFFFFFFFF)
    want = _check(a, x, head, span, P, L, span)
    np.testing.assert_array_equal(b, want)


def test_entries_reject_before_launching(native, cuda):
    """Bad lags, columns, spans, column lengths, sizes, splits, ring conditions and pointers raise
    with nothing launched or written: the -1-filled buffer is untouched. A set without a refresh
    gives all zeroes."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    per = 9 * 17 * 4  # words of a series at P = 8, L = 16
    dst = torch.full((3 * 16 * per + 16,), -1, dtype=torch.int64, device=cuda)
    W = 512
    ring_mem = torch.zeros((2 * W, 4), device=cuda)
    sd = torch.ones(64, dtype=torch.float32, device=cuda)

    def one_shot(depth=2 * W, n=W, head=W, d=None, base=None, stride=4, cols=4, L=16, span=W, P=8, sc=None, split=0):
        nat.periods_ring(ring_mem.data_ptr() if base is None else base, stride, cols, depth, head, n, span, P,
                         sd.data_ptr() if sc is None else sc, L, dst.data_ptr() if d is None else d, split, stream)

    bad = [dict(L=0), dict(L=1025), dict(L=33), dict(P=4), dict(P=128), dict(P=12), dict(span=256), dict(span=768),
           dict(span=1 << 21), dict(span=0), dict(P=16), dict(span=1 << 20, P=8), dict(span=1 << 16, P=64, L=256), dict(sc=0),
           dict(d=0), dict(base=0), dict(d=dst.data_ptr() + 8), dict(d=dst.data_ptr() + 1), dict(n=2 * W + 1, head=4 * W),
           dict(n=W, head=W - 1), dict(stride=0), dict(stride=65, cols=65), dict(cols=5), dict(cols=0), dict(depth=96),
           dict(split=3), dict(split=2), dict(span=4096, split=8), dict(span=16384, split=3)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            one_shot(**kw)

    dws = nat.DeviceWindowSet(W, 0)
    lw = nat.LongWindowSet(1 << 10, 0)
    keep = []
    for ws, cap in ((dws, 8 * W), (lw, 1 << 11)):
        for w in (11, 5):
            keep.append(nat.SeriesRing(w, cap))
            ws.add_ring(keep[-1])
    s, d = sd.data_ptr(), dst.data_ptr()
    for ws in (dws, lw):
        for span, P, sc, L, dd in ((W, 8, s, 0, d), (W, 8, s, 1025, d), (W, 8, s, 33, d), (W, 4, s, 16, d), (W, 128, s, 16, d),
                                   (768, 8, s, 16, d), (256, 8, s, 16, d), (W, 16, s, 16, d), (2048, 8, s, 16, d),
                                   (1 << 16, 64, s, 256, d), (W, 8, 0, 16, d), (W, 8, s, 16, 0), (W, 8, s, 16, d + 8)):
            with pytest.raises(RuntimeError):
                ws.export_periods(span, P, sc, L, dd, stream)
    torch.cuda.synchronize()
    assert bool((dst == -1).all())  # nothing ran
    one_shot(n=0, head=0)  # a valid call: every word zero
    dws.export_periods(W, 8, s, 16, d + 8 * 4 * per, stream)  # no refresh yet: zeroes
    lw.export_periods(W, 8, s, 16, d + 8 * (4 + 16) * per, stream)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    used = (4 + 16 + 16) * per
    assert (got[:used] == 0).all() and (got[used:] == -1).all()


@pytest.mark.parametrize("long", [False, True])
def test_agent_window_periods_on_a_recording(native, cuda, long):
    """GpuAgent replaying the MI355X capture, short (DeviceWindowSet) and long (LongWindowSet, a
    2^16-row window) sets: window_periods() in stream order after refresh() equals the reference
    over window_host() of every ring at 0, 1 and 7 more samples; the buffer is reused; the block of
    a column that stayed full is bit-identical across the calls; and per series the slots' n_0 and
    Sxy_0 add up to window_autocorr's lag 0 over the same span."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.ops.window_periods import periods_geometry, window_periods_reference
    from rocmdash.runtime.agent import GpuAgent

    W = 1 << 16 if long else 512
    P, L, span = (8, 96, 1 << 12) if long else (8, 32, 512)
    c = span // P
    agent = GpuAgent(0, source="replay", replay=CAPTURE, cfg=SamplerConfig(window=W, ring_capacity=W if long else 2048))
    try:
        assert type(agent.dws).__name__ == ("LongWindowSet" if long else "DeviceWindowSet")
        agent.prefill(W + 44 if long else 700)
        scale = agent.default_autocorr_scale()
        first, seen, kept = None, {}, 0
        for more in (0, 1, 7):
            for _ in range(more):
                agent.sample()
            agent.refresh()
            a = agent.window_periods(P, L, span)
            torch.cuda.synchronize()
            got = a.cpu().numpy()
            whole = agent.window_autocorr(L, span).cpu().numpy()
            s = 0
            for i, r in enumerate(agent.rings):
                head = int(r.head)
                rows, _ = agent.window_host(i)
                rows = np.asarray(rows, np.float32).reshape(-1, r.width)
                want = window_periods_reference(rows, scale[s:s + r.width], head, W, P, L, span)
                np.testing.assert_array_equal(got[s:s + r.width], want, err_msg=f"ring {i}")
                _, ranges = periods_geometry(head, len(rows), P, span)
                for j, (b, e) in enumerate(ranges):
                    if e - b != c:
                        continue
                    block = got[s:s + r.width, j].copy()
                    if (i, int(b)) in seen:
                        np.testing.assert_array_equal(block, seen[i, int(b)], err_msg=f"ring {i} column at row {b}")
                        kept += 1
                    seen[i, int(b)] = block
                s += r.width
            assert 0 < got[:, :, 0, 0].sum(axis=1).max() <= span
            np.testing.assert_array_equal(got[:, :, 0, 0].sum(axis=1), whole[:, 0, 0])
            np.testing.assert_array_equal(got[:, :, 0, 3].sum(axis=1), whole[:, 0, 3])
            first = a if first is None else first
            assert a is first  # the buffer is reused
        assert kept > 0
    finally:
        agent.close()

"""The window cross-correlation kernel (csrc/window_xcorr.hip) against the numpy reference of
rocmdash.ops.window_xcorr (itself checked against a triple loop in test_window_xcorr.py): ring
widths, pairs across the groups of 8 columns and lag counts, lengths around the kernel's chunk,
the ring wrap at every place of a chunk, NaN patterns that take the prefix-sum path, the full
loop and both, the largest sums, the argument checks, and DeviceWindowSet / LongWindowSet
through GpuAgent.

The sums are integers: every comparison is exact equality. Every buffer is filled with -1 before
the call that writes it, so a word the kernel left out shows."""

import os

import numpy as np
import pytest

from _window_xcorr import AXIS, assert_mirror, assert_xcorr as _check, rows as _rows, scale as _scale

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURE = os.path.join(ROOT, "tests", "fixtures", "mi355x_capture.npz")


def _run(cuda, x, pairs, L, span=None, head=None, window=None):
    import torch

    from rocmdash.ops.window_xcorr import window_xcorr

    out = torch.full((len(pairs), 2 * L + 1, 6), -1, dtype=torch.int64, device=cuda)
    got = window_xcorr(torch.from_numpy(x).to(cuda), pairs, _scale(len(x)), L, span=span, head=head, window=window, out=out)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy()


# (columns, stride) -> pairs: a and b in different groups of 8 columns where the ring has them,
# series 0 in at least three pairs; 64 columns: K = 8 with (a, b) and (b, a) both present
WIDTHS = {
    (2, 4): [(0, 1), (1, 0)],
    (5, 8): [(0, 4), (4, 0), (1, 3), (0, 2), (0, 3)],
    (16, 19): [(0, 15), (9, 3), (0, 8), (0, 1)],
    (64, 64): [(0, 63), (63, 0), (60, 3), (0, 17), (0, 33), (8, 9), (25, 40), (3, 60)],
    (61, 64): [(0, 60), (60, 3), (0, 33), (0, 9), (17, 58)],
}


@pytest.mark.parametrize("L", [1, 63, 64, 256, 1024])
@pytest.mark.parametrize("cols,stride", list(WIDTHS))
def test_widths_and_lags(native, cuda, cols, stride, L):
    """2 to 64 series in rings whose stride is larger than their columns, 1 to 8 pairs (part
    of a workgroup's group of 4, a full group and a part, two full groups), 1 to 1024 lags (no full
    tile of lags, a block less a lag, a block less its last tile's end, one lag into the second
    block, five blocks), a wrapped span of a chunk and a part."""
    import torch

    from rocmdash.ops.window_autocorr import CHUNK

    pairs = WIDTHS[(cols, stride)]
    n, W = CHUNK + 37, 2048
    x = _rows(cols * 2000 + L, cols, n, nan=0.01 if cols == 5 else 0.0)
    depth, head = 2 * W, 3 * 2 * W + 500  # the span wraps the ring
    ring = torch.full((depth, stride), 12345.0, dtype=torch.float32, device=cuda)  # padding columns hold samples
    slots = torch.arange(head - n, head, device=cuda, dtype=torch.int64) % depth
    ring[slots, :cols] = torch.from_numpy(x).to(cuda).t()
    sd = torch.from_numpy(_scale(cols)).to(cuda)
    out = torch.full((len(pairs), 2 * L + 1, 6), -1, dtype=torch.int64, device=cuda)
    native.xcorr_ring(ring.data_ptr(), stride, cols, depth, head, n, 1 << 16, sd.data_ptr(), pairs, L, out.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _check(got, x, pairs, _scale(cols), L, what=f"S {cols} stride {stride}")
    for i, (a, b) in enumerate(pairs):
        if (b, a) in pairs:
            assert_mirror(got[i], got[pairs.index((b, a))], what=f"({a}, {b})")
    if cols == 64:
        assert len(pairs) == 8 and (63, 0) in pairs and (3, 60) in pairs


def _lengths():
    from rocmdash.ops.window_autocorr import CHUNK as T

    L = 70
    return [(n, L) for n in (0, 1, 2, L, L + 1, T - 1, T, T + 1, T + L, 2 * T + 1)] + [(T + 1024, 1024)]


@pytest.mark.parametrize("n,L", _lengths())
def test_lengths(native, cuda, n, L):
    """No row, fewer rows than lags, and every length at which a chunk ends or begins."""
    pairs = [(0, 2), (1, 0)]
    x = _rows(n + L, 3, n)
    want = _check(_run(cuda, x, pairs, L), x, pairs, _scale(3), L)
    assert (want[:, :, 0] == np.maximum(n - np.abs(np.arange(-L, L + 1)), 0)[None]).all()  # without NaNs n_k == N - |k|


def test_span_cuts_the_window(native, cuda):
    """n > span: only the newest span rows count."""
    pairs = [(0, 2), (2, 1)]
    x = _rows(5, 3, 1500)
    want = _check(_run(cuda, x, pairs, 40, span=64), x, pairs, _scale(3), 40, span=64)
    assert (want[:, 40, 0] == 64).all()
    want = _check(_run(cuda, x, pairs, 40, span=1024), x, pairs, _scale(3), 40, span=1024)
    assert (want[:, 40, 0] == 1024).all()


def _wraps():
    from rocmdash.ops.window_autocorr import CHUNK as T

    n = 2 * T + 300
    return [(n, o) for o in (T // 2, T, 2 * T, 2 * T + 100, 1, n - 1)]


@pytest.mark.parametrize("n,offset", _wraps())
def test_wrap_position(native, cuda, n, offset):
    """The ring wraps ``offset`` rows into the span: in the middle of a chunk, exactly on a chunk
    boundary, inside the halo of the last full chunk, one row from either end. L = 200: pairs of
    rows straddle the wrap and the chunk boundaries."""
    W = 4096
    pairs = [(0, 2), (1, 0)]
    x = _rows(offset, 3, n, nan=0.002)
    head = 2 * (2 * W) + n - offset  # row 2 x depth is span row `offset`
    _check(_run(cuda, x, pairs, 200, head=head, window=W), x, pairs, _scale(3), 200, what=f"wrap at {offset}")


VALIDITY = ["none", "x_only", "y_only", "y_halo", "percent", "run", "series"]


@pytest.mark.parametrize("kind", VALIDITY)
def test_validity(native, cuda, kind):
    """No NaN (every chunk takes the prefix-sum path), one NaN in x only, in y only, in y's halo
    only (the last chunk's own row, the halo of the one before), 1 % NaN in both (chunks of both
    kinds), a NaN run longer than L, and one series all NaN: its pairs are all zero and the other
    pairs are what they are without it. L = 300: two lag blocks."""
    from rocmdash.ops.window_autocorr import CHUNK as T

    n, L = 3 * T + 11, 300
    pairs = [(0, 1), (2, 3), (1, 2), (3, 0)]
    x = _rows(len(kind), 4, n, nan=0.01 if kind == "percent" else 0.0)
    if kind == "x_only":
        x[0, T + T // 2] = np.nan
    elif kind == "y_only":
        x[1, T + T // 2] = np.nan
    elif kind == "y_halo":
        x[1, 3 * T + 5] = np.nan
    elif kind == "run":
        x[0, T - 100:T + L + 57] = np.nan
    elif kind == "series":
        x[3] = np.nan
    want = _check(_run(cuda, x, pairs, L), x, pairs, _scale(4), L, what=kind)
    both = [np.count_nonzero(~np.isnan(x[a]) & ~np.isnan(x[b])) for a, b in pairs]
    assert (want[:, L, 0] == both).all()
    if kind == "series":
        assert (want[1] == 0).all() and (want[3] == 0).all() and want[0].all() and want[2].all()


@pytest.mark.parametrize("N,L", [(1 << 20, 8), (1 << 16, 1024)])
def test_largest_sums(native, cuda, N, L):
    """Two series with every sample at or above the axis (q = 4095): the largest sums there are,
    all six words against the closed form. A 32-bit prefix of q^2 fails here."""
    x = np.full((2, N), np.float32(AXIS), np.float32)
    x[0, ::3] = np.inf
    x[1, 1::3] = np.float32(1e30)
    got = _run(cuda, x, [(0, 1), (1, 0)], L, span=N)
    m = N - np.abs(np.arange(-L, L + 1, dtype=np.int64))
    want = np.stack([m, 4095 * m, 4095 * m, 4095 * 4095 * m, 4095 * 4095 * m, 4095 * 4095 * m], axis=1)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want)


def test_overwrites_garbage_and_repeats(native, cuda):
    """A destination full of garbage has every word overwritten, and two runs give the same bits
    (many workgroups add onto the same words)."""
    import torch

    from rocmdash.ops.window_xcorr import window_xcorr

    S, n, L = 12, 1 << 14, 128
    pairs = [(0, 11), (9, 2), (0, 5), (5, 0), (3, 4)]
    x = _rows(99, S, n, nan=0.01)
    xd = torch.from_numpy(x).to(cuda)
    a = torch.full((len(pairs), 2 * L + 1, 6), -0x0123456789ABCDEF, dtype=torch.int64, device=cuda)
    b = torch.full((len(pairs), 2 * L + 1, 6), 0x7FFFFFFFFFFFFFFF, dtype=torch.int64, device=cuda)
    window_xcorr(xd, pairs, _scale(S), L, head=5 * n - 77, window=n, out=a)
    window_xcorr(xd, pairs, _scale(S), L, head=5 * n - 77, window=n, out=b)
    torch.cuda.synchronize()
    want = _check(a.cpu().numpy(), x, pairs, _scale(S), L)
    np.testing.assert_array_equal(b.cpu().numpy(), want)


def test_entries_reject_before_launching(native, cuda):
    """Bad pairs, lags, spans, ring conditions and pointers raise with nothing launched or
    written: the -1-filled buffer is untouched. Then the valid n = 0 call and the export before a
    refresh write zeroes into exactly the words they own."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    dst = torch.full((8 * 2049 * 6 + 8,), -1, dtype=torch.int64, device=cuda)
    W = 64
    ring_mem = torch.zeros((2 * W, 4), device=cuda)
    sd = torch.ones(64, dtype=torch.float32, device=cuda)
    nine = [(0, 1)] * 9

    def one_shot(depth=2 * W, n=W, head=W, d=None, base=None, stride=4, cols=4, L=16, span=64, sc=None, pairs=((0, 1),)):
        nat.xcorr_ring(ring_mem.data_ptr() if base is None else base, stride, cols, depth, head, n, span,
                       sd.data_ptr() if sc is None else sc, list(pairs), L, dst.data_ptr() if d is None else d, stream)

    bad = [dict(L=0), dict(L=1025), dict(span=32), dict(span=96), dict(span=1 << 21), dict(span=0), dict(sc=0), dict(d=0),
           dict(base=0), dict(d=dst.data_ptr() + 4), dict(d=dst.data_ptr() + 1), dict(n=2 * W + 1, head=4 * W),
           dict(n=W, head=W - 1), dict(stride=0), dict(stride=65, cols=65), dict(cols=5), dict(cols=0), dict(depth=96),
           dict(pairs=[]), dict(pairs=nine), dict(pairs=[(0, 4)]), dict(pairs=[(4, 0)]), dict(pairs=[(2, 2)]),
           dict(pairs=[(0, 3)], cols=3)]
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
    ok, p, d = [(0, 1), (12, 11)], sd.data_ptr(), dst.data_ptr()
    for ws in (dws, lw):
        for pairs, span, sc, L, dd in ((ok, 64, p, 0, d), (ok, 64, p, 1025, d), (ok, 100, p, 16, d), (ok, 32, p, 16, d),
                                       (ok, 64, 0, 16, d), (ok, 64, p, 16, 0), (ok, 64, p, 16, d + 4), ([], 64, p, 16, d),
                                       (nine, 64, p, 16, d), ([(3, 3)], 64, p, 16, d), ([(0, 16)], 64, p, 16, d),
                                       ([(10, 11)], 64, p, 16, d), ([(12, 2)], 64, p, 16, d)):  # the last two: across rings
            with pytest.raises(RuntimeError):
                ws.export_xcorr(pairs, span, sc, L, dd, stream)
    torch.cuda.synchronize()
    assert bool((dst == -1).all())  # nothing ran
    one_shot(n=0, head=0)  # a valid call: every word zero
    first = 1 * 33 * 6
    dws.export_xcorr(ok, 64, p, 8, d + 8 * first, stream)  # no refresh yet: zeroes
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    used = first + 2 * 17 * 6
    assert (got[:used] == 0).all() and (got[used:] == -1).all()


@pytest.mark.parametrize("long", [False, True])
def test_agent_window_xcorr_on_a_recording(native, cuda, long):
    """GpuAgent replaying the MI355X capture, short (DeviceWindowSet) and long (LongWindowSet, a
    2^16-row window) sets: window_xcorr() in stream order after refresh() equals the reference
    over window_host() of every ring; the buffer is reused; after invalidate() a DeviceWindowSet
    gives all zeroes."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.ops.window_xcorr import window_xcorr_reference
    from rocmdash.runtime.agent import GpuAgent

    W = 1 << 16 if long else 256
    L, span = (96, 1 << 12) if long else (64, None)
    agent = GpuAgent(0, source="replay", replay=CAPTURE, cfg=SamplerConfig(window=W, ring_capacity=W if long else 1024))
    try:
        assert type(agent.dws).__name__ == ("LongWindowSet" if long else "DeviceWindowSet")
        agent.prefill(W + 44 if long else 300)
        scale = agent.default_autocorr_scale()
        pairs = agent.default_joint_pairs()
        assert 1 <= len(pairs) <= 8
        first = None
        for more in (0, 1, 7):
            for _ in range(more):
                agent.sample()
            agent.refresh()
            a = agent.window_xcorr(None, L, span)
            torch.cuda.synchronize()
            got = a.cpu().numpy()
            s = 0
            seen = 0
            for i, r in enumerate(agent.rings):
                mine = [k for k, (pa, _) in enumerate(pairs) if s <= pa < s + r.width]
                if mine:
                    rows, _ = agent.window_host(i)
                    rows = np.asarray(rows, np.float32).reshape(-1, r.width)
                    want = window_xcorr_reference(rows, [(pairs[k][0] - s, pairs[k][1] - s) for k in mine], scale[s:s + r.width],
                                                  L, span)
                    np.testing.assert_array_equal(got[mine], want, err_msg=f"ring {i}")
                    seen += len(mine)
                s += r.width
            assert seen == len(pairs)
            assert 0 < got[:, L, 0].max() <= min(W, span or W)
            first = a if first is None else first
            assert a is first  # the buffer is reused
        if not long:
            agent.dws.invalidate()
            a = agent.window_xcorr(None, L, span)
            torch.cuda.synchronize()
            assert bool((a == 0).all())
    finally:
        agent.close()

"""The window autocorrelation kernel (csrc/window_autocorr.hip) against the numpy reference of
rocmdash.ops.window_autocorr (itself checked against a triple loop in test_window_autocorr.py):
ring widths and lag counts, lengths around the kernel's chunk, the ring wrap at every place of a
chunk, NaN patterns that take the prefix-sum path, the full loop and both, the largest sums, the
argument checks, and DeviceWindowSet / LongWindowSet through GpuAgent.

The sums are integers: every comparison is exact equality. Every buffer is filled with -1 before
the call that writes it, so a word the kernel left out shows."""

import os

import numpy as np
import pytest

from _window_exports import _assert_autocorr as _check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURE = os.path.join(ROOT, "tests", "fixtures", "mi355x_capture.npz")
PCT = (50.0, 90.0, 99.0)
AXIS = 100.0


def _rows(seed, S, n, nan=0.0):
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


def _scale(S):
    return np.full(S, np.float32(4095.0 / AXIS), np.float32)


def _run(cuda, x, L, span=None, head=None, window=None):
    import torch

    from rocmdash.ops.window_autocorr import window_autocorr

    S = len(x)
    out = torch.full((S, L + 1, 4), -1, dtype=torch.int64, device=cuda)
    got = window_autocorr(torch.from_numpy(x).to(cuda), _scale(S), L, span=span, head=head, window=window, out=out)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy()


# (columns, stride): 1, 5 and 16 series in a ring whose stride is larger, the widest ring there is
# (64 = stride: eight full groups of series), and 61 of 64 (seven groups and a part)
WIDTHS = [(1, 4), (5, 8), (16, 19), (64, 64), (61, 64)]


@pytest.mark.parametrize("L", [1, 63, 64, 1024])
@pytest.mark.parametrize("cols,stride", WIDTHS)
def test_widths_and_lags(native, cuda, cols, stride, L):
    """1, 5, 16 and 64 series (one partial group, two full groups, eight), rings whose stride is
    larger than their columns, 1 to 1024 lags (no full tile of lags, one block, one lag into the
    second block, five blocks), a wrapped span of a chunk and a part."""
    import torch

    from rocmdash.ops.window_autocorr import CHUNK

    n, W = CHUNK + 37, 2048
    x = _rows(cols * 2000 + L, cols, n, nan=0.01 if cols == 5 else 0.0)
    depth, head = 2 * W, 3 * 2 * W + 500  # the span wraps the ring
    ring = torch.full((depth, stride), 12345.0, dtype=torch.float32, device=cuda)  # padding columns hold samples
    slots = torch.arange(head - n, head, device=cuda, dtype=torch.int64) % depth
    ring[slots, :cols] = torch.from_numpy(x).to(cuda).t()
    sd = torch.from_numpy(_scale(cols)).to(cuda)
    out = torch.full((cols, L + 1, 4), -1, dtype=torch.int64, device=cuda)
    native.autocorr_ring(ring.data_ptr(), stride, cols, depth, head, n, 1 << 16, sd.data_ptr(), L, out.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check(out.cpu().numpy(), x, _scale(cols), L, what=f"S {cols} stride {stride}")


def _lengths():
    from rocmdash.ops.window_autocorr import CHUNK as T

    L = 70
    return [(n, L) for n in (0, 1, 2, L, L + 1, T - 1, T, T + 1, T + L, 2 * T + 1)] + [(T + 1024, 1024)]


@pytest.mark.parametrize("n,L", _lengths())
def test_lengths(native, cuda, n, L):
    """No row, fewer rows than lags, and every length at which a chunk ends or begins."""
    x = _rows(n + L, 3, n)
    want = _check(_run(cuda, x, L), x, _scale(3), L)
    assert (want[:, :, 0] == np.maximum(n - np.arange(L + 1), 0)[None]).all()  # without NaNs n_k == N - k


def test_span_cuts_the_window(native, cuda):
    """n > span: only the newest span rows count."""
    x = _rows(5, 3, 1500)
    want = _check(_run(cuda, x, 40, span=64), x, _scale(3), 40, span=64)
    assert (want[:, 0, 0] == 64).all()
    want = _check(_run(cuda, x, 40, span=1024), x, _scale(3), 40, span=1024)
    assert (want[:, 0, 0] == 1024).all()


def _wraps():
    from rocmdash.ops.window_autocorr import CHUNK as T

    n = 2 * T + 300
    return [(n, o) for o in (T // 2, T, 2 * T, 2 * T + 100, 1, n - 1)]


@pytest.mark.parametrize("n,offset", _wraps())
def test_wrap_position(native, cuda, n, offset):
    """The ring wraps ``offset`` rows into the span: in the middle of a chunk, exactly on a chunk
    boundary, inside the halo of the last full chunk, one row from either end. L = 200: pairs
    straddle the wrap and the chunk boundaries."""
    W = 4096
    x = _rows(offset, 3, n, nan=0.002)
    head = 2 * (2 * W) + n - offset  # row 2 x depth is span row `offset`
    _check(_run(cuda, x, 200, head=head, window=W), x, _scale(3), 200, what=f"wrap at {offset}")


VALIDITY = ["none", "one", "percent", "run", "series", "halo", "far_halo"]


@pytest.mark.parametrize("kind", VALIDITY)
def test_validity(native, cuda, kind):
    """No NaN (every chunk takes the prefix-sum path), one NaN and 1 % NaN (chunks of both
    kinds), a NaN run longer than L, one series all NaN beside valid ones, and a NaN that lies
    only in a chunk's halo; ``far_halo``: a NaN that, of the first chunk's two lag blocks, only the
    second's halo reaches, so that series takes the prefix-sum path in one block and the full loop
    in the other. L = 300: two lag blocks."""
    from rocmdash.ops.window_autocorr import CHUNK as T, LAG_BLOCK

    n, L = 3 * T + 11, 300
    x = _rows(len(kind), 3, n, nan=0.01 if kind == "percent" else 0.0)
    if kind == "one":
        x[1, T + T // 2] = np.nan
    elif kind == "run":
        x[0, T - 100:T + L + 57] = np.nan
    elif kind == "series":
        x[1] = np.nan
    elif kind == "halo":
        x[2, 3 * T + 5] = np.nan  # the last chunk's own row, and the halo of the one before
    elif kind == "far_halo":
        x[0, T + LAG_BLOCK + 40] = np.nan  # block 0 of chunk 0 loads the rows below T + 272, block 1 those below T + 320
    want = _check(_run(cuda, x, L), x, _scale(3), L, what=kind)
    assert (want[:, 0, 0] == np.count_nonzero(~np.isnan(x), axis=1)).all()
    if kind == "series":
        assert (want[1] == 0).all() and want[0].all()


@pytest.mark.parametrize("N,L", [(1 << 20, 8), (1 << 16, 1024)])
def test_largest_sums(native, cuda, N, L):
    """One series with every sample at or above the axis (q = 4095): the largest sums there are."""
    x = np.full((1, N), np.float32(AXIS), np.float32)
    x[0, ::3] = np.inf
    x[0, 1::3] = np.float32(1e30)
    got = _run(cuda, x, L, span=N)
    k = np.arange(L + 1, dtype=np.int64)
    want = np.stack([N - k, 4095 * (N - k), 4095 * (N - k), 4095 * 4095 * (N - k)], axis=1)[None]
    np.testing.assert_array_equal(got, want)
    _check(got, x, _scale(1), L, span=N)


def test_overwrites_garbage_and_repeats(native, cuda):
    """A destination full of garbage has every word overwritten, and two runs give the same bits
    (many workgroups add onto the same words)."""
    import torch

    from rocmdash.ops.window_autocorr import window_autocorr

    S, n, L = 12, 1 << 14, 128
    x = _rows(99, S, n, nan=0.01)
    xd = torch.from_numpy(x).to(cuda)
    a = torch.full((S, L + 1, 4), -0x0123456789ABCDEF, dtype=torch.int64, device=cuda)
    b = torch.full((S, L + 1, 4), 0x7FFFFFFFFFFFFFFF, dtype=torch.int64, device=cuda)
    window_autocorr(xd, _scale(S), L, head=5 * n - 77, window=n, out=a)
    window_autocorr(xd, _scale(S), L, head=5 * n - 77, window=n, out=b)
    torch.cuda.synchronize()
    want = _check(a.cpu().numpy(), x, _scale(S), L)
    np.testing.assert_array_equal(b.cpu().numpy(), want)


def test_entries_reject_before_launching(native, cuda):
    """Bad lags, spans, ring conditions and pointers raise with nothing launched or written: the
    -1-filled buffer is untouched."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    dst = torch.full((16 * 1025 * 4 + 8,), -1, dtype=torch.int64, device=cuda)
    W = 64
    ring_mem = torch.zeros((2 * W, 4), device=cuda)
    sd = torch.ones(64, dtype=torch.float32, device=cuda)

    def one_shot(depth=2 * W, n=W, head=W, d=None, base=None, stride=4, cols=4, L=16, span=64, sc=None):
        nat.autocorr_ring(ring_mem.data_ptr() if base is None else base, stride, cols, depth, head, n, span,
                          sd.data_ptr() if sc is None else sc, L, dst.data_ptr() if d is None else d, stream)

    bad = [dict(L=0), dict(L=1025), dict(span=32), dict(span=96), dict(span=1 << 21), dict(span=0), dict(sc=0), dict(d=0),
           dict(base=0), dict(d=dst.data_ptr() + 4), dict(d=dst.data_ptr() + 1), dict(n=2 * W + 1, head=4 * W),
           dict(n=W, head=W - 1), dict(stride=0), dict(stride=65, cols=65), dict(cols=5), dict(cols=0), dict(depth=96)]
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
    for ws in (dws, lw):
        for span, sc, L, d in ((64, sd.data_ptr(), 0, dst.data_ptr()), (64, sd.data_ptr(), 1025, dst.data_ptr()),
                               (100, sd.data_ptr(), 16, dst.data_ptr()), (32, sd.data_ptr(), 16, dst.data_ptr()),
                               (64, 0, 16, dst.data_ptr()), (64, sd.data_ptr(), 16, 0), (64, sd.data_ptr(), 16, dst.data_ptr() + 4)):
            with pytest.raises(RuntimeError):
                ws.export_autocorr(span, sc, L, d, stream)
    torch.cuda.synchronize()
    assert bool((dst == -1).all())  # nothing ran
    one_shot(n=0, head=0)  # a valid call: every word zero
    dws.export_autocorr(64, sd.data_ptr(), 8, dst.data_ptr() + 8 * 4 * 17 * 4, stream)  # no refresh yet: zeroes
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    used = 4 * 17 * 4 + 16 * 9 * 4
    assert (got[:used] == 0).all() and (got[used:] == -1).all()


@pytest.mark.parametrize("long", [False, True])
def test_agent_window_autocorr_on_a_recording(native, cuda, long):
    """GpuAgent replaying the MI355X capture, short (DeviceWindowSet) and long (LongWindowSet, a
    2^16-row window) sets: window_autocorr() in stream order after refresh() equals the reference
    over window_host() of every ring; the buffer is reused; after invalidate() a DeviceWindowSet
    gives all zeroes."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.ops.window_autocorr import window_autocorr_reference
    from rocmdash.runtime.agent import GpuAgent

    W = 1 << 16 if long else 256
    L, span = (96, 1 << 12) if long else (64, None)
    agent = GpuAgent(0, source="replay", replay=CAPTURE, cfg=SamplerConfig(window=W, ring_capacity=W if long else 1024))
    try:
        assert type(agent.dws).__name__ == ("LongWindowSet" if long else "DeviceWindowSet")
        agent.prefill(W + 44 if long else 300)
        scale = agent.default_autocorr_scale()
        assert scale.dtype == np.float32 and scale.shape == (len(agent.series),)
        first = None
        for more in (0, 1, 7):
            for _ in range(more):
                agent.sample()
            agent.refresh()
            a = agent.window_autocorr(L, span)
            torch.cuda.synchronize()
            got = a.cpu().numpy()
            s = 0
            for i, r in enumerate(agent.rings):
                rows, _ = agent.window_host(i)
                rows = np.asarray(rows, np.float32).reshape(-1, r.width)
                want = window_autocorr_reference(rows, scale[s:s + r.width], L, span)
                np.testing.assert_array_equal(got[s:s + r.width], want, err_msg=f"ring {i}")
                s += r.width
            assert 0 < got[:, 0, 0].max() <= min(W, span or W)
            first = a if first is None else first
            assert a is first  # the buffer is reused
        if not long:
            agent.dws.invalidate()
            a = agent.window_autocorr(L, span)
            torch.cuda.synchronize()
            assert bool((a == 0).all())
    finally:
        agent.close()

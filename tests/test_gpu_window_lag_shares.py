"""The chunk loop of the two lag kernels (csrc/window_autocorr.hip, csrc/window_xcorr.hip): a
workgroup that walks more than one chunk. The launch rule gives every workgroup one chunk at every
shape the kernels' own tests use, so what a workgroup carries from chunk to chunk - the sums in
registers, the LDS words and the marks of the chunk before, the barrier at the loop's head, a
series that takes the prefix-sum path in one chunk and the full walks in the next, the last
workgroup's shorter share - runs here only: through the ``share`` override of the one-shot
entries (chunks per workgroup; 0 is the rule), and through the rule itself at the two smallest
closed-form shapes at which it shares.

The sums are integers: every comparison is exact equality, against the numpy references of
rocmdash.ops and against the ``share = 1`` launch of the same rows. Every buffer is filled with
-1 before the call that writes it, so a word the kernel left out shows."""

import numpy as np
import pytest

from _window_exports import _assert_autocorr
from _window_xcorr import AXIS, assert_mirror, assert_xcorr, rows as _rows, scale as _scale

pytestmark = pytest.mark.gpu

T = 1024  # rocmdash.ops.window_autocorr.CHUNK, asserted below
N = 5 * T + 11  # six chunks, the last of 11 rows
L = 300  # two lag blocks
W = 8192  # the window the rows are laid into: a ring of 2 W rows
WRAP = 2 * T + 300  # the span row that sits at slot 0 of the ring: inside chunk 2
SHARES = (1, 2, 4, 6)  # workgroups of 1 + 1 + 1 + 1 + 1 + 1, 2 + 2 + 2, 4 + 2 and 6 chunks
TARGET_GROUPS = 1024  # kTargetGroups, kXcorrTargetGroups: the workgroups the launch rule aims at

# span rows that are NaN, per kind. With L = 300 a chunk loads at most 1344 rows, so a NaN
# more than 320 rows into a chunk is in no other chunk's halo.
NAN_ROWS = {
    "clean": (),
    "first_chunk_only": (T // 2,),  # marked in chunk 0, clean from then on
    "last_chunk_only": (5 * T + 5,),  # clean, then marked: the 11-row chunk (and the halo of the one before)
    "alternate": (T + T // 2, 3 * T + T // 2),  # clean, marked, clean, marked, clean, clean
    "halo_only": (2 * T + 5,),  # chunk 2's own row and chunk 1's halo
}
KINDS = list(NAN_ROWS) + ["percent"]
AUTOCORR_SERIES = {"first_chunk_only": 0, "last_chunk_only": 0, "alternate": 1, "halo_only": 2}


def test_constants():
    from rocmdash.ops.window_autocorr import CHUNK

    assert CHUNK == T and -(-N // T) == 6 and N % T == 11 and 2 * T < WRAP < 3 * T and L // 256 + 1 == 2


def _put_nans(x, kind, series, seed):
    if kind == "percent":
        rng = np.random.default_rng(seed)
        for s in series:
            x[s, rng.random(x.shape[1]) < 0.01] = np.nan
    else:
        for s in series:
            x[s, list(NAN_ROWS[kind])] = np.nan


def _head(n):
    return 2 * (2 * W) + n - WRAP  # row 2 x depth is span row WRAP


def _autocorr(native, cuda, x, stride, L, share, span=None, head=None, window=None):
    """[S, L + 1, 4] of the rows x [S, n]: through rocmdash.ops where the ring's stride is its
    columns, else the native entry on a ring whose padding columns and unused slots hold samples."""
    import torch

    from rocmdash.ops.window_autocorr import DEFAULT_SPAN, window_autocorr

    S, n = x.shape
    out = torch.full((S, L + 1, 4), -1, dtype=torch.int64, device=cuda)
    if stride == S:
        got = window_autocorr(torch.from_numpy(x).to(cuda), _scale(S), L, span=span, head=head, window=window, out=out,
                              share=share)
        assert got is out
    else:
        depth = 2 * window
        ring = torch.full((depth, stride), 12345.0, dtype=torch.float32, device=cuda)
        slots = torch.arange(head - n, head, device=cuda, dtype=torch.int64) % depth
        ring[slots, :S] = torch.from_numpy(x).to(cuda).t()
        sd = torch.from_numpy(_scale(S)).to(cuda)
        native.autocorr_ring(ring.data_ptr(), stride, S, depth, head, n, span or DEFAULT_SPAN, sd.data_ptr(), L,
                             out.data_ptr(), torch.cuda.current_stream().cuda_stream, share=share)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _xcorr(cuda, x, pairs, L, share, span=None, head=None, window=None):
    import torch

    from rocmdash.ops.window_xcorr import window_xcorr

    out = torch.full((len(pairs), 2 * L + 1, 6), -1, dtype=torch.int64, device=cuda)
    got = window_xcorr(torch.from_numpy(x).to(cuda), pairs, _scale(len(x)), L, span=span, head=head, window=window, out=out,
                       share=share)
    assert got is out
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. autocorr, chunks shared -----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cols,stride", [(3, 3), (11, 16)])
def test_autocorr_chunks_shared(native, cuda, cols, stride, kind):
    """Six chunks, the last of 11 rows, two lag blocks, the ring wrap inside chunk 2; 3 columns,
    and 11 at stride 16 (two groups of series, the second partial, which get the same NaNs 8
    columns on); every NaN kind; 1, 2, 4 and 6 chunks per workgroup. Each result equals the
    reference and the ``share = 1`` result."""
    x = _rows(cols * 100 + KINDS.index(kind), cols, N)
    series = range(cols) if kind == "percent" else [s for s in (AUTOCORR_SERIES.get(kind, 0), AUTOCORR_SERIES.get(kind, 0) + 8)
                                                    if s < cols]
    _put_nans(x, kind, series, 7)
    got = {sh: _autocorr(native, cuda, x, stride, L, sh, head=_head(N), window=W) for sh in SHARES}
    want = _assert_autocorr(got[1], x, _scale(cols), L, what=f"{kind} S {cols} stride {stride} share 1")
    assert (got[1] >= 0).all()
    assert (want[:, 0, 0] == np.count_nonzero(~np.isnan(x), axis=1)).all()
    for sh in SHARES[1:]:
        bad = np.argwhere(got[sh] != want)
        assert not len(bad), (f"{kind} S {cols} stride {stride} share {sh}: {len(bad)} words differ, first (series, lag, word) "
                              f"= {bad[0].tolist()}: got {got[sh][tuple(bad[0])]}, want {want[tuple(bad[0])]}")
        np.testing.assert_array_equal(got[sh], got[1], err_msg=f"{kind} share {sh} against share 1")


# ---- 2. xcorr, chunks shared --------------------------------------------------------------------
XCORR_PAIRS = [(0, 1), (2, 3), (1, 2), (3, 0), (1, 0)]  # two pair groups, the second of one pair: (0, 1)'s mirror
SIDES = {"x": (0,), "y": (1,), "both": (0, 1)}  # of pair (0, 1); pair (2, 3) stays clean beside it


@pytest.mark.parametrize("side", list(SIDES))
@pytest.mark.parametrize("kind", KINDS)
def test_xcorr_chunks_shared(native, cuda, kind, side):
    """The same rows, lags, wrap, shares and NaN kinds, the NaNs in pair (0, 1)'s x only, y only
    and both, 4 series, 5 pairs. Each result equals the reference and the ``share = 1`` result,
    and (1, 0) mirrors (0, 1)."""
    x = _rows(1000 + KINDS.index(kind), 4, N)
    _put_nans(x, kind, SIDES[side], 11)
    got = {sh: _xcorr(cuda, x, XCORR_PAIRS, L, sh, head=_head(N), window=W) for sh in SHARES}
    want = assert_xcorr(got[1], x, XCORR_PAIRS, _scale(4), L, what=f"{kind} {side} share 1")
    both = [np.count_nonzero(~np.isnan(x[a]) & ~np.isnan(x[b])) for a, b in XCORR_PAIRS]
    assert (want[:, L, 0] == both).all()
    for sh in SHARES:
        what = f"{kind} {side} share {sh}"
        assert (got[sh] >= 0).all(), f"{what}: {np.count_nonzero(got[sh] < 0)} words unwritten or negative"
        bad = np.argwhere(got[sh] != want)
        assert not len(bad), (f"{what}: {len(bad)} words differ, first (pair, index, word) = {bad[0].tolist()}: "
                              f"got {got[sh][tuple(bad[0])]}, want {want[tuple(bad[0])]}")
        assert_mirror(got[sh][XCORR_PAIRS.index((0, 1))], got[sh][XCORR_PAIRS.index((1, 0))], what=what)
        np.testing.assert_array_equal(got[sh], got[1], err_msg=f"{what} against share 1")


# ---- 3. the largest sums through one thread's accumulators --------------------------------------
@pytest.mark.parametrize("L", [8, 300])
def test_autocorr_largest_sums_in_one_workgroup(native, cuda, L):
    """Every sample at or above the axis (q = 4095), six full chunks, one workgroup per (group,
    lag block): a thread's 64-bit sums take all six chunks' int32 partials."""
    n = 6 * T
    x = np.full((1, n), np.float32(AXIS), np.float32)
    x[0, ::3] = np.inf
    x[0, 1::3] = np.float32(1e30)
    got = _autocorr(native, cuda, x, 1, L, 6)
    k = np.arange(L + 1, dtype=np.int64)
    want = np.stack([n - k, 4095 * (n - k), 4095 * (n - k), 4095 * 4095 * (n - k)], axis=1)[None]
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("L", [8, 300])
def test_xcorr_largest_sums_in_one_workgroup(native, cuda, L):
    n = 6 * T
    x = np.full((2, n), np.float32(AXIS), np.float32)
    x[0, ::3] = np.inf
    x[1, 1::3] = np.float32(1e30)
    got = _xcorr(cuda, x, [(0, 1), (1, 0)], L, 6)
    m = n - np.abs(np.arange(-L, L + 1, dtype=np.int64))
    want = np.stack([m, 4095 * m, 4095 * m, 4095 * 4095 * m, 4095 * 4095 * m, 4095 * 4095 * m], axis=1)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want)


# ---- 4. the rule itself choosing share > 1 ------------------------------------------------------
def _rule(chunks, per_chunk):
    """run() of csrc/window_autocorr.hip, xcorr_share of csrc/window_xcorr_plan.h"""
    shares = min(chunks, max(1, TARGET_GROUPS // per_chunk))
    return -(-chunks // shares)


def _q(value, S=1):
    from rocmdash.ops.window_autocorr import quantise

    return int(quantise(np.full((1, S), value, np.float32), _scale(S))[0][0, 0])


def test_autocorr_rule_shares_chunks(native, cuda):
    """share = 0 on one constant series of 2^20 rows at L = 1024: 1024 chunks and five lag
    blocks, so the rule gives a workgroup 6 chunks and the last of the 171 only 4."""
    from rocmdash.ops.window_autocorr import CHUNK, LAG_BLOCK, SERIES_GROUP

    n, L = 1 << 20, 1024
    chunks = -(-n // CHUNK)
    share = _rule(chunks, -(-1 // SERIES_GROUP) * (L // LAG_BLOCK + 1))
    assert share >= 2 and chunks % share, f"the launch rule gives share {share} of {chunks} chunks: pick a shape that shares"
    assert (share, -(-chunks // share), chunks - (-(-chunks // share) - 1) * share) == (6, 171, 4)
    q = _q(37.0)
    assert 0 < q < 4095
    x = np.full((1, n), np.float32(37.0), np.float32)
    got = _autocorr(native, cuda, x, 1, L, 0, span=n)
    m = n - np.arange(L + 1, dtype=np.int64)
    np.testing.assert_array_equal(got, np.stack([m, q * m, q * m, q * q * m], axis=1)[None])


def test_xcorr_rule_shares_chunks(native, cuda):
    """share = 0 on two constant series of 102 T + 1 rows, 8 pairs (two pair groups) at L = 1024:
    103 chunks, ten workgroups a chunk, so the rule gives a workgroup 2 chunks and the last of
    the 52 the single 1-row chunk. All eight slots against the closed form."""
    from rocmdash.ops.window_autocorr import CHUNK
    from rocmdash.ops.window_xcorr import GROUP_PAIRS, LAG_BLOCK

    n, L = 102 * T + 1, 1024
    pairs = [(0, 1), (1, 0)] * 4
    chunks = -(-n // CHUNK)
    share = _rule(chunks, -(-len(pairs) // GROUP_PAIRS) * (L // LAG_BLOCK + 1))
    assert share >= 2 and chunks % share, f"the launch rule gives share {share} of {chunks} chunks: pick a shape that shares"
    assert (share, -(-chunks // share), chunks - (-(-chunks // share) - 1) * share) == (2, 52, 1)
    qa, qb = _q(37.0), _q(81.5)
    assert 0 < qa < qb < 4095
    x = np.stack([np.full(n, np.float32(37.0), np.float32), np.full(n, np.float32(81.5), np.float32)])
    got = _xcorr(cuda, x, pairs, L, 0, span=1 << 17)
    m = n - np.abs(np.arange(-L, L + 1, dtype=np.int64))
    ab = np.stack([m, qa * m, qb * m, qa * qb * m, qa * qa * m, qb * qb * m], axis=1)
    for i, p in enumerate(pairs):
        np.testing.assert_array_equal(got[i], ab if p == (0, 1) else ab[:, [0, 2, 1, 3, 5, 4]], err_msg=f"slot {i} pair {p}")


# ---- 5. rejects ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["autocorr", "xcorr"])
def test_share_out_of_range_is_refused_before_any_write(native, cuda, kernel):
    """More chunks per workgroup than the span has (the span, not the window, counts), and any
    share but 1 of no rows at all, raise with the -1-filled buffer untouched; share = 1 of no rows
    writes zeroes."""
    import torch

    from rocmdash.ops.window_autocorr import window_autocorr
    from rocmdash.ops.window_xcorr import window_xcorr

    L = 16
    shape = (3, L + 1, 4) if kernel == "autocorr" else (2, 2 * L + 1, 6)
    out = torch.full(shape, -1, dtype=torch.int64, device=cuda)

    def run(n, share, span=None):
        x = torch.from_numpy(_rows(3, 3, n)).to(cuda)
        if kernel == "autocorr":
            window_autocorr(x, _scale(3), L, span=span, out=out, share=share)
        else:
            window_xcorr(x, [(0, 2), (1, 0)], _scale(3), L, span=span, out=out, share=share)
        torch.cuda.synchronize()

    for n, share, span in ((3 * T + 1, 5, None), (3 * T + 1, 2, 1024), (T, 2, None), (0, 2, None)):
        with pytest.raises(RuntimeError):
            run(n, share, span)
        torch.cuda.synchronize()
        assert bool((out == -1).all()), f"n {n} share {share} span {span}: the refused call wrote"
    run(0, 1)
    assert bool((out == 0).all())
    out.fill_(-1)
    run(3 * T + 1, 4)  # the largest share there is: accepted
    assert bool((out >= 0).all()) and int(out[0, 0 if kernel == "autocorr" else L, 0]) == 3 * T + 1

"""Every selection path against the exact sorted-fp32 oracle (tests/_exact.py): the LDS window
kernel (csrc/window_stats.hip) one-shot and through DeviceWindowSet's incremental paths, the
long-window radix chain and bracket mode (csrc/long_window_radix.hip,
csrc/long_window_brackets.hip), their one-rank node mode, and the node selection over sorted
lists (csrc/node_window.hip). Each output must be the fp32 value the oracle names - equal, or
within one ulp and inside [x0, x1] where the kernel interpolates - on inputs where a rank off
by one is another value: a few ulp between neighbours, every exponent and sign, signed zeros
and denormals, tie boundaries, ramps, windows of 0..3 valid samples and +-inf."""

import numpy as np
import pytest

import _exact
from _exact import INF_SERIES, assert_exact, exact_stats, expected_comparisons

pytestmark = pytest.mark.gpu

TRIOS = [(50.0, 90.0, 99.0), (0.0, 100.0, 50.0), (0.1, 99.9, 37.5)]
LW_SUM_GROUP = _exact.long_window_sum_group()  # UG in csrc/long_window_pass.h


def _report(request, compared):
    print(f"[exact] {request.node.name}: {compared} output comparisons")


def _neighbours_apart(ex, s):
    """Where both order statistics of a percentile weigh in, they are over one ulp apart."""
    for q in range(3):
        if 0 < ex.frac[s, q] < 1:
            if not float(ex.x1[s, q]) - float(ex.x0[s, q]) > _exact.ulp32(ex.x1[s, q]):
                return False
    return True


@pytest.mark.parametrize("trio", TRIOS)
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1000, 4097, 32768])
def test_window_stats_exact(native, cuda, request, n, trio):
    import torch

    from rocmdash.ops.window_stats import window_stats

    rng = np.random.default_rng(n + 3)  # seeds that meet the precondition on `narrow` below
    x = _exact.family_rows(rng, 0, n, n, blips=(n // 2,))
    ex = exact_stats(x, trio)
    if n <= 1000:  # `narrow` is scaled for this: a rank off by one is another value
        assert _neighbours_apart(ex, _exact.FAMILIES.index("narrow"))
    got = window_stats(torch.from_numpy(np.ascontiguousarray(x.T)).to(cuda), pct=trio)
    torch.cuda.synchronize()
    compared = assert_exact(got.cpu().numpy(), ex, trio, sum_group=1, skip_nonfinite=(INF_SERIES,))
    assert compared == expected_comparisons(15, skipped=_skipped(ex, INF_SERIES))
    _report(request, compared)


class _Mirror:
    """Everything pushed, oldest first."""

    def __init__(self, width):
        self.rows = np.zeros((0, width), np.float32)

    def push(self, x):
        self.rows = np.concatenate([self.rows, x])

    def window(self, W):
        return self.rows[-W:]


def _skipped(ex, series):
    return int(not (np.isfinite(ex.mean[series]) and np.isfinite(ex.mean_abs[series])
                    and np.all(np.isfinite(ex.x0[series])) and np.all(np.isfinite(ex.x1[series]))))


def _has_run(seq, run):
    seq = list(seq)
    return any(seq[i:i + len(run)] == list(run) for i in range(len(seq)))


@pytest.mark.parametrize("trio", TRIOS)
@pytest.mark.parametrize("W", [64, 512, 4096, 32768])
def test_device_window_exact(native, cuda, request, W, trio):
    """DeviceWindowSet through SeriesRing in pull mode: a full sort, then the incremental
    paths (one row, few rows, 255 / 256 rows, a 257-row fall-back), exact after every
    refresh; the resident window ends as the oracle's sorted samples."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    nat.set_pull_mode(True)
    ring = nat.SeriesRing(15, 8 * W)
    dws = nat.DeviceWindowSet(W, 0)
    dws.add_ring(ring)
    m = _Mirror(15)
    out = torch.empty((15, 8), device=cuda)
    exp = torch.empty((15, 1 + W), device=cuda)
    rng = np.random.default_rng(W)
    stream = torch.cuda.current_stream().cuda_stream
    blip = _exact.FAMILIES.index("blip")
    t, compared, want, blip_nv = 0, 0, 0, []
    for it, add in enumerate([W + 3, 1, 1, 0, 2, 17, 255, 256, 257, 1, 64, 5, 1, 0]):
        if add:
            x = _exact.family_rows(rng, t, add, W, blips=(3, W + 5))
            ring.push_many(x, np.arange(t + 1, t + 1 + add, dtype=np.uint64))
            m.push(x)
            t += add
        dws.refresh(out.data_ptr(), stream, trio[0], trio[1], trio[2])
        torch.cuda.synchronize()
        ex = exact_stats(m.window(W), trio)
        compared += assert_exact(out.cpu().numpy(), ex, trio, sum_group=1, skip_nonfinite=(INF_SERIES,))
        want += expected_comparisons(15, skipped=_skipped(ex, INF_SERIES))
        blip_nv.append(int(ex.nv[blip]))
    assert compared == want
    # the blip series lost its one valid sample and got one again (small windows: and lost it)
    assert _has_run(blip_nv, [1, 0]) and _has_run(blip_nv, [0, 1]), blip_nv
    if W <= 512:
        assert blip_nv[-1] == 0, blip_nv
    assert dws.stats()["incremental_launches"] >= 7, dws.stats()
    dws.export_sorted(exp.data_ptr(), stream)
    torch.cuda.synchronize()
    got = exp.cpu().numpy()
    for s in range(15):
        assert int(got[s, 0]) == int(ex.nv[s]), s
        # as values: the LDS kernel does not order signed zeros
        np.testing.assert_array_equal(got[s, 1:1 + int(ex.nv[s])], ex.sorted[s], err_msg=f"series {s}")
    _report(request, compared)


def _lw_fill(W, cap):
    """The fill in capacity-sized pushes: W + 5 rows in all."""
    fill, left = [], W + 5
    while left:
        fill.append(min(cap, left))
        left -= fill[-1]
    return fill


LW_STEPS = [1, 0, 3, 100, 100, 100, 256, 257, 100, 100, 1, 700, 100, 100, 100, 100]


class _LwRings:
    """Two rings of 8 and 13 series (two segments, unaligned rows) fed the 21 families."""

    def __init__(self, nat, W, cap, seed):
        self.W = W
        self.ra, self.rb = nat.SeriesRing(8, cap), nat.SeriesRing(13, cap)
        self.m = _Mirror(21)
        self.rng = np.random.default_rng(seed)
        self.t = 0

    def add_to(self, s):
        s.add_ring(self.ra)
        s.add_ring(self.rb)

    def push(self, k):
        if not k:
            return
        x = _exact.family_rows(self.rng, self.t, k, self.W, width=21, blips=(5, self.W + 8))
        ts = np.arange(self.t, self.t + k, dtype=np.uint64)
        self.ra.push_many(np.ascontiguousarray(x[:, :8]), ts)
        self.rb.push_many(np.ascontiguousarray(x[:, 8:]), ts)
        self.m.push(x)
        self.t += k


@pytest.mark.parametrize("trio", TRIOS)
@pytest.mark.parametrize("W,chunk_rows", [(1024, 0), (2048, 0), (65536, 256)])
def test_long_window_exact(native, cuda, request, W, chunk_rows, trio):
    """LongWindowSet: the default (brackets, direct launches), the radix chain alone and graph
    launches side by side on the same rings (W = 65536: 256 chunks of 256 rows, and the
    default plan beside them), exact after every refresh of every set; the default set
    resolved refreshes by its brackets and by the chain, so both were under the oracle."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    cap = 1 << 14
    rings = _LwRings(nat, W, cap, seed=W)
    lw = nat.LongWindowSet(W, 0, chunk_rows=chunk_rows)
    lwr = nat.LongWindowSet(W, 0, chunk_rows=chunk_rows)
    lwr.brackets = False  # the radix chain alone
    lwg = nat.LongWindowSet(W, 0, use_graph=True, chunk_rows=chunk_rows)
    sets = [lw, lwr, lwg]
    if chunk_rows:
        sets.append(nat.LongWindowSet(W, 0))  # the default plan
    for s in sets:
        rings.add_to(s)
    outs = [torch.empty((21, 8), device=cuda) for _ in sets]
    stream = torch.cuda.current_stream().cuda_stream
    blip = _exact.FAMILIES.index("blip")
    compared, want, blip_nv = 0, 0, []
    steps = _lw_fill(W, cap) + LW_STEPS
    for k in steps:
        rings.push(k)
        for s, o in zip(sets, outs):
            s.refresh(o.data_ptr(), stream, trio[0], trio[1], trio[2])
        torch.cuda.synchronize()
        ex = exact_stats(rings.m.window(W), trio)
        for o in outs:
            compared += assert_exact(o.cpu().numpy(), ex, trio, sum_group=LW_SUM_GROUP, skip_nonfinite=(INF_SERIES,))
            want += expected_comparisons(21, skipped=_skipped(ex, INF_SERIES))
        blip_nv.append(int(ex.nv[blip]))
    assert compared == want
    assert _has_run(blip_nv, [1, 0]) and _has_run(blip_nv, [0, 1]), blip_nv
    if W <= 2048:
        assert blip_nv[-1] == 0, blip_nv
    if chunk_rows:
        assert lw.chunk_plan == [(256, W // 256)] * 2
    st = lw.stats()
    assert st["rows_lost"] == 0 and st["bracket_refreshes"] >= 1 and st["chain_refreshes"] >= 1, st
    assert sum(x[1] for x in lw.bracket_stats()) >= 1, lw.bracket_stats()  # series resolved by their brackets
    assert all(x[0] == 0 for x in lwr.bracket_stats())
    _report(request, compared)


@pytest.mark.parametrize("trio", TRIOS)
def test_long_window_node_one_rank_exact(native, cuda, request, trio):
    """``refresh_node`` without a communicator: the node-mode kernels (prediction record,
    node bracket records, the per-rank partial reduction) at W = 65536, last = NaN."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    W, cap = 1 << 16, 1 << 14
    rings = _LwRings(nat, W, cap, seed=21)
    lwn = nat.LongWindowSet(W, 0)
    rings.add_to(lwn)
    out = torch.empty((21, 8), device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    compared, want = 0, 0
    steps = _lw_fill(W, cap) + LW_STEPS
    for k in steps:
        rings.push(k)
        lwn.refresh_node(out.data_ptr(), stream, trio[0], trio[1], trio[2], None, False)
        torch.cuda.synchronize()
        ex = exact_stats(rings.m.window(W), trio)
        got = out.cpu().numpy()
        compared += assert_exact(got, ex, trio, sum_group=LW_SUM_GROUP, last=False, skip_nonfinite=(INF_SERIES,))
        want += expected_comparisons(21, last=False, skipped=_skipped(ex, INF_SERIES))
        assert np.isnan(got[:, 6]).all()
    assert compared == want
    st = lwn.stats()
    assert st["node_refreshes"] == len(steps) and st["rows_lost"] == 0, st
    assert sum(x[1] for x in lwn.bracket_stats(1)) >= 1, lwn.bracket_stats(1)  # node brackets resolved refreshes too
    _report(request, compared)


def _node_lists(rng, N, W):
    """[N][S] sorted lists: what goes wrong in a merge of sorted lists."""

    def count(i, kind):
        if kind == "full":
            return W
        if kind == "one":
            return 1
        if kind == "mixed":  # empty, one-sample, full and in between
            return [0, 1, W, int(rng.integers(0, W + 1))][i % 4]
        return int(rng.integers(0, W + 1))

    lists = []
    for i in range(N):
        row = [
            rng.choice(np.array([6.0, 7.0, 7.0, 7.0, 8.0], np.float32), W),  # tied across every list and within
            # -0.0 in one list, +0.0 in another
            rng.choice(np.array([-1.0, -0.0, 2.0] if i % 2 == 0 else [-1.0, 0.0, 2.0], np.float32), count(i, "any")),
            np.zeros(0, np.float32),  # every list empty
            rng.normal(100, 0.01, [0, 1][i % 2]).astype(np.float32),  # empty and one-sample lists
            rng.normal(100, 0.01, W).astype(np.float32),  # full lists, neighbours a few ulp apart
            rng.normal(0, 1, count(i, "mixed")).astype(np.float32),  # unequal counts
            rng.integers(0, 6, count(i, "any")).astype(np.float32),
            (rng.normal(0, 1, W) * 10.0 ** rng.uniform(-30, 30, W)).astype(np.float32)[:count(i, "any")],
            rng.normal(50, 10, 1).astype(np.float32),  # one sample in every list
        ]
        lists.append([np.sort(v) for v in row])
    return lists


@pytest.mark.parametrize("trio", TRIOS)
@pytest.mark.parametrize("N,W", [(2, 64), (8, 1000), (8, 4096), (8, 4097)])
def test_node_select_exact(native, cuda, request, N, W, trio):
    """``node_select`` over the union of N sorted lists; N * W = 32768 is the last size staged
    in LDS, W = 4097 the first searched in L2."""
    import torch

    rng = np.random.default_rng(N * W)
    lists = _node_lists(rng, N, W)
    S = len(lists[0])
    node = np.full((N, S, W + 1), np.inf, np.float32)
    for i in range(N):
        for s in range(S):
            node[i, s, 0] = len(lists[i][s])
            node[i, s, 1:1 + len(lists[i][s])] = lists[i][s]
    cols = [np.concatenate([lists[i][s] for i in range(N)]) for s in range(S)]
    n = max(1, max(len(c) for c in cols))
    x = np.full((n, S), np.nan, np.float32)
    for s, c in enumerate(cols):
        x[n - len(c):, s] = c
    ex = exact_stats(x, trio)
    assert ex.nv[2] == 0 and ex.nv[8] == N and ex.nv[0] == N * W and ex.nv[4] == N * W
    dev = torch.from_numpy(node).to(cuda)
    out = torch.empty((S, 8), device=cuda)
    native.node_select(dev.data_ptr(), N, S, W, out.data_ptr(), torch.cuda.current_stream().cuda_stream, trio[0], trio[1],
                       trio[2])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    compared = assert_exact(got, ex, trio, sum_group=1, last=False)
    assert compared == expected_comparisons(S, last=False)
    assert np.isnan(got[:, 6]).all()
    _report(request, compared)

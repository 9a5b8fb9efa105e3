"""The window-excursion kernels (csrc/window_excursions.hip) against
``window_excursions_reference``: the one-shot op over a wrapped ring, forced chunk lengths,
a long window, DeviceWindowSet.export_excursions after every refresh, LongWindowSet over a
filling and a wrapped device ring, the argument checks, and GpuAgent and the exporter end to
end on a recording.

Every comparison is EQUALITY of all eight integers; every output buffer is filled with -1
before the call that writes it. The inputs are built from series families that put run
boundaries at every lane, wave, chunk and wrap hand-off whatever the kernel's geometry."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURE = os.path.join(ROOT, "tests", "fixtures", "mi355x_capture.npz")
PCT = (50.0, 90.0, 99.0)
POSITIONS = (0, 1, 63, 64, 65, "n/2", "n-2", "n-1")
RUN_MEANS = (1, 7, 300, 5000)
NUM_FAMILIES = 3 + 2 * len(POSITIONS) + 2 * len(RUN_MEANS) + 4


def _thresholds(S, K):
    """[S, K]: series s has the thresholds 10 s, 10 s + 1, ...: a kernel that took another
    series' row of them would count differently."""
    return (10.0 * np.arange(S)[:, None] + np.arange(K)[None, :]).astype(np.float32)


def _runs(rng, n, mean):
    """bool [n]: alternating runs with geometric lengths of the given mean."""
    lens = rng.geometric(1.0 / mean, size=n // mean + 8)
    while lens.sum() < n:
        lens = np.concatenate([lens, rng.geometric(1.0 / mean, size=n // mean + 8)])
    up = (np.arange(len(lens)) + rng.integers(2)) % 2 == 1
    return np.repeat(up, lens)[:n]


def _patterns(rng, n):
    """[(above-mask [n], NaN-mask [n] or None, kind)] of the families, in a fixed order."""
    pos = [{"n/2": n // 2, "n-2": n - 2, "n-1": n - 1}.get(p, p) % n for p in POSITIONS]
    out = [(np.ones(n, bool), None, ""), (np.zeros(n, bool), None, ""), (np.arange(n) % 2 == 1, None, "")]
    for single in (False, True):  # one not-above sample in an all-above series; then one above sample
        for p in pos:
            m = np.full(n, not single)
            m[p] = single
            out.append((m, None, ""))
    out += [(_runs(rng, n, mean), None, "") for mean in RUN_MEANS]
    out += [(_runs(rng, n, mean), rng.random(n) < 0.1, "") for mean in RUN_MEANS]  # NaN inside runs too
    out.append((np.zeros(n, bool), np.ones(n, bool), ""))  # all NaN
    out.append((_runs(rng, n, 3), None, "equal"))
    out += [(_runs(rng, n, 5), None, "-inf+inf"), (_runs(rng, n, 5), None, "+inf-inf")]
    assert len(out) == NUM_FAMILIES
    return out


_CASES = {}


def _case(n, K):
    """(x [F, n], thresholds [F, K], reference [F, K, 8]) of the families, built once per
    (n, K) and shared read-only. A family's pattern is what the LAST threshold sees: an above
    sample is above every threshold, a not-above sample lies at a random level below the
    last one, so the lower thresholds see other, random runs."""
    from rocmdash.ops.window_excursions import window_excursions_reference

    if (n, K) not in _CASES:
        rng = np.random.default_rng(1000 * K + n)
        thr = _thresholds(NUM_FAMILIES, K)
        x = np.empty((NUM_FAMILIES, n), np.float32)
        for s, (up, nan, kind) in enumerate(_patterns(rng, n)):
            low = thr[s, rng.integers(0, K, n)] - 0.5
            if kind == "equal":  # exactly on a threshold: not above it
                low = thr[s, rng.integers(0, K, n)]
            v = np.where(up, thr[s, -1] + 0.5, low).astype(np.float32)
            if nan is not None:
                v[nan] = np.nan
            if kind == "-inf+inf":
                v[0], v[-1] = -np.inf, np.inf  # n = 1: the one sample is +inf
            if kind == "+inf-inf":
                v[0], v[-1] = np.inf, -np.inf
            x[s] = v
        ref = window_excursions_reference(x.T, thr)
        for a in (x, thr, ref):
            a.setflags(write=False)
        _CASES[(n, K)] = (x, thr, ref)
    return _CASES[(n, K)]


# the families a ring of each stride takes: consecutive, together all of them
_FIRST = {1: 0, 5: 1, 11: 6, 16: 17, 23: 2}


def _take(n, K, stride):
    x, thr, ref = _case(n, K)
    idx = (np.arange(stride) + _FIRST[stride]) % NUM_FAMILIES
    return np.array(x[idx]), np.array(thr[idx]), ref[idx]


def test_families_cover_every_stride():
    seen = set()
    for stride, first in _FIRST.items():
        seen |= set(((np.arange(stride) + first) % NUM_FAMILIES).tolist())
    assert seen == set(range(NUM_FAMILIES))


SHAPES = [(1, 64), (63, 64), (64, 64), (65, 128), (4096, 4096), (4097, 8192)]


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("stride", [1, 5, 11, 16, 23])
@pytest.mark.parametrize("head_kind", ["n", "n+1", "wrapped"])
@pytest.mark.parametrize("n,window", SHAPES)
def test_window_excursions_one_shot(native, cuda, n, window, head_kind, stride, K):
    import torch

    from rocmdash.ops.window_excursions import window_excursions

    head = {"n": n, "n+1": n + 1, "wrapped": 3 * window - 1}[head_kind]
    x, thr, ref = _take(n, K, stride)
    got = window_excursions(torch.from_numpy(x).to(cuda), thr, head=head, window=window)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


@pytest.mark.parametrize("wrapped", [False, True])
def test_forced_chunks_agree_bit_for_bit(native, cuda, wrapped):
    """n = 4096 cut every 4 (5 when wrapped: the smallest the cap of 1024 chunks allows), 7,
    64, 65 and 4096 rows, and planned: all equal the reference, so each other; one row per
    chunk less raises and writes nothing."""
    import torch

    from rocmdash.ops.window_excursions import MAX_CHUNKS, excursion_chunk_rows_min, window_excursions

    n = W = 4096
    head = 3 * W - 1 if wrapped else n + 77
    x, thr, ref = _take(n, 4, 11)
    xd = torch.from_numpy(x).to(cuda)
    smallest = excursion_chunk_rows_min(head, n, 2 * W)
    assert smallest == (5 if wrapped else 4)
    assert native.excursion_chunk_count(2 * W, head, n, smallest) <= MAX_CHUNKS < native.excursion_chunk_count(
        2 * W, head, n, smallest - 1)
    results = []
    for chunk_rows in (smallest, 7, 64, 65, 4096, 0):
        got = window_excursions(xd, thr, head=head, window=W, chunk_rows=chunk_rows)
        torch.cuda.synchronize()
        results.append(got.cpu().numpy())
        np.testing.assert_array_equal(results[-1], ref, err_msg=f"chunk_rows {chunk_rows}")
    for r in results[1:]:
        assert r.tobytes() == results[0].tobytes()
    with pytest.raises(RuntimeError):
        window_excursions(xd, thr, head=head, window=W, chunk_rows=smallest - 1)


def test_long_window_many_chunks_and_one_workgroup(native, cuda):
    """window 2^17 x 3 series at head = window + 12345: planned (512 chunks of 256 rows), and
    forced into one chunk - one workgroup streaming 2^17 rows, far more than its threads."""
    import torch

    from rocmdash.ops.window_excursions import window_excursions, window_excursions_reference

    W = 1 << 17
    rng = np.random.default_rng(17)
    thr = _thresholds(3, 3)
    up = [_runs(rng, W, 5000), _runs(rng, W, 7), np.ones(W, bool)]
    x = np.stack([np.where(u, thr[s, -1] + 0.5, thr[s, rng.integers(0, 3, W)] - 0.5) for s, u in enumerate(up)]).astype(np.float32)
    x[1, rng.random(W) < 0.1] = np.nan
    ref = window_excursions_reference(x.T, thr)
    assert ref[2, 2, 3] == W and ref[0, 2, 2] > 4
    xd = torch.from_numpy(x).to(cuda)
    assert native.excursion_plan_chunk_rows(W) == 256
    for chunk_rows in (0, W):
        got = window_excursions(xd, thr, head=W + 12345, window=W, chunk_rows=chunk_rows)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=f"chunk_rows {chunk_rows}")


def _stream(rng, rows, S, K):
    """[rows, S] of a long stream: series s in runs of mean 1, 7, 300, 5000 (by s), every
    third series with 10 % NaN, levels as in ``_case``."""
    thr = _thresholds(S, K)
    x = np.empty((rows, S), np.float32)
    for s in range(S):
        up = _runs(rng, rows, RUN_MEANS[s % len(RUN_MEANS)])
        x[:, s] = np.where(up, thr[s, -1] + 0.5, thr[s, rng.integers(0, K, rows)] - 0.5)
        if s % 3 == 2:
            x[rng.random(rows) < 0.1, s] = np.nan
    return x, thr


class _Rings:
    """Rings of the given widths in one DeviceWindowSet, fed from one long stream."""

    def __init__(self, nat, W, widths, stream):
        self.W, self.widths, self.stream = W, widths, stream
        self.rings = [nat.SeriesRing(w, 8 * W) for w in widths]
        self.dws = nat.DeviceWindowSet(W, 0)
        for r in self.rings:
            self.dws.add_ring(r)
        self.t = 0

    def push(self, k):
        x = self.stream[self.t:self.t + k]
        assert len(x) == k
        ts = np.arange(self.t + 1, self.t + 1 + k, dtype=np.uint64)
        c0 = 0
        for r, w in zip(self.rings, self.widths):
            r.push_many(np.ascontiguousarray(x[:, c0:c0 + w]), ts)
            c0 += w
        self.t += k

    def window(self):
        return self.stream[max(0, self.t - self.W):self.t]


@pytest.mark.parametrize("W", [256, 4096])
def test_export_excursions_after_every_refresh(native, cuda, W):
    """Two rings (5 + 11 series) in one DeviceWindowSet, pull mode: the records are exact
    after EVERY refresh of a filling, then sliding window - 1, 3 and 100 entering rows -
    each ring's series at its offset; all zeroes without state."""
    import torch

    from rocmdash.ops.window_excursions import window_excursions_reference

    nat = native
    nat.set_pinned_host_rings(True)
    nat.set_pull_mode(True)
    K, steps = 3, [W // 2, 1, 3, 100, W // 2 + 9, 1, 3, 100, 1, W - 1, 100]
    stream, thr = _stream(np.random.default_rng(W), sum(steps), 16, K)
    rs = _Rings(nat, W, (5, 11), stream)
    out = torch.empty((16, 8), device=cuda)
    td = torch.from_numpy(thr).to(cuda)
    dst = torch.empty((16, K, 8), dtype=torch.int32, device=cuda)
    nbytes = nat.excursion_workspace_bytes(16, K)
    work = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    hs = torch.cuda.current_stream().cuda_stream

    def export():
        dst.fill_(-1)
        rs.dws.export_excursions(td.data_ptr(), K, dst.data_ptr(), work.data_ptr(), nbytes, hs)
        torch.cuda.synchronize()
        return dst.cpu().numpy()

    assert (export() == 0).all()  # no refresh yet
    for add in steps:
        rs.push(add)
        rs.dws.refresh(out.data_ptr(), hs, *PCT)
        got = export()
        win = rs.window()
        np.testing.assert_array_equal(got, window_excursions_reference(win, thr), err_msg=f"after +{add} rows (t = {rs.t})")
        np.testing.assert_array_equal(got[:, 0, 1], out.cpu().numpy()[:, 7])  # valid = the statistics' count
    assert rs.t > 2 * W
    rs.dws.invalidate()
    assert (export() == 0).all()


@pytest.mark.parametrize("W", [1024, 65536])
def test_long_window_export_excursions(native, cuda, W):
    """One ring of 12 series in a LongWindowSet: before any refresh, a window that is not full
    yet, then full, after +100 rows, and after enough rows to wrap the device ring.
    hipErrorNotReady (rows staged that no kernel has written) cannot be reached from Python -
    refresh() always flushes - as for export_trend; a non-zero hipError_t raises RuntimeError
    in the binding either way (see the argument checks)."""
    import torch

    from rocmdash.ops.window_excursions import window_excursions_reference

    nat = native
    nat.set_pinned_host_rings(True)
    K = 4
    ring = nat.SeriesRing(12, 2 * W)
    lw = nat.LongWindowSet(W, 0)
    lw.add_ring(ring)
    out = torch.empty((12, 8), device=cuda)
    dst = torch.empty((12, K, 8), dtype=torch.int32, device=cuda)
    nbytes = nat.excursion_workspace_bytes(12, K)
    work = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    hs = torch.cuda.current_stream().cuda_stream
    steps = (W // 2 + 5, W // 2 + 32, 100, W + W // 4 + 7)
    stream, thr = _stream(np.random.default_rng(W + 1), sum(steps), 12, K)
    td = torch.from_numpy(thr).to(cuda)

    def export():
        dst.fill_(-1)
        lw.export_excursions(td.data_ptr(), K, dst.data_ptr(), work.data_ptr(), nbytes, hs)
        torch.cuda.synchronize()
        return dst.cpu().numpy()

    assert (export() == 0).all()
    t = 0
    for add in steps:
        x = np.ascontiguousarray(stream[t:t + add])
        ring.push_many(x, np.arange(t + 1, t + 1 + add, dtype=np.uint64))
        t += add
        lw.refresh(out.data_ptr(), hs, *PCT)
        got = export()
        np.testing.assert_array_equal(got, window_excursions_reference(stream[max(0, t - W):t], thr),
                                      err_msg=f"after +{add} rows (t = {t})")
        np.testing.assert_array_equal(got[:, 0, 1], out.cpu().numpy()[:, 7])
    assert lw.stats()["rows_lost"] == 0


def test_excursion_entries_reject_before_launching(native, cuda):
    """Every rejected case raises with nothing launched or written: the -1 fill is intact."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    hs = torch.cuda.current_stream().cuda_stream
    W = 64
    dst = torch.full((4, 4, 8), -1, dtype=torch.int32, device=cuda)
    ring_mem = torch.zeros((2 * W, 4), device=cuda)
    thr = torch.from_numpy(_thresholds(4, 4)).to(cuda)
    nbytes = nat.excursion_workspace_bytes(4, 4)
    work = torch.full((nbytes + 64,), 255, dtype=torch.uint8, device=cuda)
    assert nbytes == 1024 * 4 * 4 * 32 and nat.excursion_workspace_bytes(4, 0) == 0 == nat.excursion_workspace_bytes(4, 5)

    def one_shot(base=None, stride=4, cols=4, depth=2 * W, head=W, n=W, t=None, K=4, chunk_rows=0, d=None, w=None, wb=nbytes):
        nat.excursion_ring(ring_mem.data_ptr() if base is None else base, stride, cols, depth, head, n,
                           thr.data_ptr() if t is None else t, K, chunk_rows, dst.data_ptr() if d is None else d,
                           work.data_ptr() if w is None else w, wb, hs)

    big = torch.zeros((4096, 1), device=cuda)  # 4096 rows cut every 3: 1366 chunks > 1024
    bad = [dict(base=big.data_ptr(), stride=1, cols=1, depth=4096, head=4096, n=4096, chunk_rows=3),
           dict(wb=nbytes - 1), dict(wb=0), dict(depth=96), dict(depth=0), dict(n=2 * W + 1, head=4 * W), dict(n=W, head=W - 1),
           dict(cols=0), dict(cols=5), dict(stride=0, cols=0), dict(stride=65, cols=65, wb=1 << 30), dict(K=0), dict(K=5),
           dict(base=0), dict(t=0), dict(d=0), dict(w=0), dict(base=ring_mem.data_ptr() + 2), dict(t=thr.data_ptr() + 2),
           dict(d=dst.data_ptr() + 8), dict(w=work.data_ptr() + 8)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            one_shot(**kw)

    rd = nat.SeriesRing(4, 8 * W)
    dws = nat.DeviceWindowSet(W, 0)
    dws.add_ring(rd)
    rl = nat.SeriesRing(4, 1 << 10)
    lw = nat.LongWindowSet(1 << 10, 0)
    lw.add_ring(rl)
    for ws in (dws, lw):
        good = dict(t=thr.data_ptr(), K=4, d=dst.data_ptr(), w=work.data_ptr(), wb=nbytes)
        for kw in (dict(K=0), dict(K=5), dict(t=0), dict(d=0), dict(w=0), dict(wb=nbytes - 1), dict(d=dst.data_ptr() + 4),
                   dict(w=work.data_ptr() + 4)):
            a = dict(good, **kw)
            with pytest.raises(RuntimeError):
                ws.export_excursions(a["t"], a["K"], a["d"], a["w"], a["wb"], hs)
    torch.cuda.synchronize()
    assert bool((dst == -1).all()) and bool((work == 255).all())  # nothing ran
    one_shot(n=0, head=0)  # a valid call: an empty window
    torch.cuda.synchronize()
    assert bool((dst == 0).all())


def _agent_reference(agent, thr):
    from rocmdash.ops.window_excursions import window_excursions_reference

    blocks, s = [], 0
    for i, r in enumerate(agent.rings):
        rows, _ = agent.window_host(i)
        blocks.append(window_excursions_reference(np.asarray(rows, np.float32).reshape(-1, r.width), thr[s:s + r.width]))
        s += r.width
    return np.concatenate(blocks)


def test_agent_window_excursions_on_a_recording(native, cuda):
    """GpuAgent replaying the MI355X capture: window_excursions() in stream order after
    refresh() equals the reference over each ring's host window, with the default
    thresholds and with given ones; output and workspace are reused."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.runtime.agent import GpuAgent

    agent = GpuAgent(0, source="replay", replay=CAPTURE, cfg=SamplerConfig(window=256, ring_capacity=1024))
    try:
        assert type(agent.dws).__name__ == "DeviceWindowSet"
        agent.prefill(300)
        S = len(agent.series)
        given = agent.default_excursion_thresholds((0.05, 0.3, 0.6, 0.9))
        first = None
        for more, thr in ((0, None), (1, None), (7, given)):
            for _ in range(more):
                agent.sample()
            agent.refresh()
            e = agent.window_excursions(thr)
            torch.cuda.synchronize()
            t = agent.default_excursion_thresholds() if thr is None else thr
            assert e.dtype == torch.int32 and tuple(e.shape) == (S, t.shape[1], 8)
            np.testing.assert_array_equal(e.cpu().numpy(), _agent_reference(agent, t))
            if first is None:
                first = e.data_ptr()
            elif thr is None:
                assert e.data_ptr() == first
        assert int(e[:, 0, 2].sum()) > 0  # the recording does cross 5 % of some axis
    finally:
        agent.close()


def test_exporter_serves_the_excursion_families(native, cuda):
    """LocalNodeSource on the recording with --window-excursions 0.5,0.9: the five families
    are in /metrics and equal the reference over the agent's host rows; off (the default)
    none of them is, and a bad option is refused before an agent exists."""
    from rocmdash.config import SamplerConfig
    from rocmdash.prom.exporter import Exporter, LocalNodeSource
    from rocmdash.prom.exposition import EXCURSION_FAMILIES, parse_text

    cfg = SamplerConfig(window=256, ring_capacity=1024)
    with pytest.raises(ValueError):
        LocalNodeSource(devices=[0], source="replay", counters="synthetic", replay=CAPTURE, cfg=cfg, window_excursions="0.9,0.5")
    src = LocalNodeSource(devices=[0], source="replay", counters="synthetic", replay=CAPTURE, cfg=cfg, window_excursions="0.5,0.9")
    exp = Exporter(src, hostname="n1")
    try:
        agent = src.agents[0]
        agent.stop()  # the background samplers: the rows below are pushed from this thread
        agent.prefill(300)
        samples = parse_text(exp.render())
        thr = src.excursion_thresholds
        ref = _agent_reference(agent, thr)
    finally:
        exp.close()
    assert thr.shape == (len(src.series), 2)
    for name, field, _ in EXCURSION_FAMILIES:
        rows = [s for s in samples if s.name == name]
        assert len(rows) == len(src.series) * 2
        for s in rows:
            lab = s.label_dict()
            si = src.series.index(lab["metric"])
            k = [repr(float(v)) for v in thr[si]].index(lab["threshold"])
            assert s.value == ref[si, k, field], (name, lab)

    off = LocalNodeSource(devices=[0], source="replay", counters="synthetic", replay=CAPTURE, cfg=cfg)
    exp = Exporter(off)
    try:
        text = exp.render()
        assert off.excursion_thresholds is None and "excursion" not in text and "rocmdash_window_above_samples" not in text
    finally:
        exp.close()

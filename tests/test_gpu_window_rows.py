"""The stats kernel with a handful of rows entering one ring per refresh - what the
amd-smi ring sees once its thread runs at the free-running cap (4-6 rows a refresh) while
the counter ring still brings one: 1 row (the one-row path), 4 (all by value in the
kernel argument), 5, 8 and 9 (the rows before the newest four pulled from the mapped host
ring, or staged with a copy), across the wrap of the host and the device ring."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMI_W, CTR_W = 11, 5  # the two rings' widths in the dashboard


@pytest.mark.parametrize("pull", [True, False], ids=["pull", "staged"])
@pytest.mark.parametrize("W", [64, 512])
def test_few_entering_rows_match_reference(native, cuda, W, pull):
    import torch

    from rocmdash.ops.window_stats import window_stats_reference

    nat = native
    nat.set_pinned_host_rings(True)
    nat.set_pull_mode(pull)
    try:
        cap = 4 * W  # host ring; the device ring is 2 W deep: both wrap at row 4 W
        ring_a = nat.SeriesRing(SMI_W, cap)
        ring_b = nat.SeriesRing(CTR_W, cap)
        dws = nat.DeviceWindowSet(W, 0)
        dws.add_ring(ring_a)
        dws.add_ring(ring_b)
    finally:
        nat.set_pull_mode(True)
    out = torch.empty((SMI_W + CTR_W, 8), device=cuda)
    rng = np.random.default_rng(W + int(pull))
    t = 0

    def push(ring, width, n):
        nonlocal t
        for _ in range(n):
            t += 1
            row = rng.integers(0, 9, width).astype(np.float32)  # ties, like integer telemetry
            row[rng.random(width) < 0.05] = np.nan  # failed reads
            ring.push(row, t)

    def check(what):
        dws.refresh(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ra, _ = ring_a.window(W)
        rb, _ = ring_b.window(W)
        ref = np.concatenate([window_stats_reference(ra.T), window_stats_reference(rb.T)])
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-4, err_msg=what)

    # up to 30 rows before the wrap: the first refresh sorts, the rest are incremental
    push(ring_a, SMI_W, cap - 30)
    push(ring_b, CTR_W, cap - 8)
    check("first refresh")
    st0 = dws.stats()
    ks = [1, 4, 5, 9, 8, 1, 9, 5, 4, 1, 9, 1, 5, 9, 4, 8]  # 84 rows + 16 rows: across row 4 W on both rings
    for it, k in enumerate(ks):
        push(ring_a, SMI_W, k)
        push(ring_b, CTR_W, 1)
        check(f"refresh {it}: {k} rows + 1 row")
    assert ring_a.head > cap and ring_b.head > cap  # both wrapped
    st = dws.stats()
    assert st["incremental_launches"] - st0["incremental_launches"] == len(ks), st
    inline_cap = nat.WS_INLINE_ROWS  # csrc/window_stats.h kInlineRows
    assert st["inline_rows"] - st0["inline_rows"] == sum(min(k, inline_cap) for k in ks) + len(ks), st
    n9 = sum(k > inline_cap for k in ks)
    if pull:
        assert st["pulled_series"] - st0["pulled_series"] == n9 * SMI_W, st
        assert st["memcpy_calls"] == st0["memcpy_calls"], st
    else:
        assert st["pulled_series"] == 0 and st["memcpy_calls"] - st0["memcpy_calls"] >= n9, st

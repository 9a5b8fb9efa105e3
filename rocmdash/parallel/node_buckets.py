"""Node-wide window distributions: every GPU's cumulative le-buckets and their sum.

Per refresh (after every rank's ``GpuAgent.refresh()``) each rank counts its series'
buckets on its GPU (``GpuAgent.window_buckets``, csrc/window_buckets.hip) and ONE small
all-gather - ``[S, B + 1]`` float32, about 1 KB per rank, on the aggregator's native
communicator like the stats gather - builds ``[N, S, B + 1]``. Buckets add up, so the
node's distribution is the sum over the ranks (exact in float32: N x W < 2^24); nothing
of the windows themselves moves, unlike the node-window statistics' gather of the sorted
windows (``rocmdash.parallel.node_window``). Other ranks take part and get ``None``.

Counts only add up over the same bounds: the ranks compare theirs at construction.
"""

from __future__ import annotations

import numpy as np

from ..ops.window_buckets import check_bounds


class NodeBuckets:
    """Every rank's window buckets on rank 0, and their sum (one collective per refresh)."""

    def __init__(self, agent, aggregator, bounds=None, collective_timeout_s: float = 60.0):
        self.agent = agent
        self.aggregator = aggregator
        self.is_root = aggregator.rank == 0
        self.collective_timeout_s = float(collective_timeout_s)
        self._pub = None  # completion signal behind the native gather (bounded wait)
        if getattr(agent.cfg, "long_window", False):
            raise ValueError("a window of > 32768 samples has no le-buckets (they are counted in the resident sorted "
                             "windows of <= 32768 samples)")
        b = agent.default_bucket_bounds() if bounds is None else bounds
        self.bounds = check_bounds(b, len(agent.series))
        theirs = aggregator.all_gather_object(self.bounds.tobytes())  # collective
        differ = [r for r, t in enumerate(theirs) if t != theirs[0]]
        if differ:
            raise ValueError(f"window bucket bounds differ between ranks (ranks {differ} from rank 0): buckets only "
                             "add up over the same bounds - pass every rank the same ones")

    def refresh(self):
        """Collective: every rank calls it after its ``agent.refresh()``. Returns
        ``(per_gpu [N, S, B + 1], node [S, B + 1])`` float32 host arrays on rank 0 (the
        gather was waited for), ``None`` elsewhere. The wait for the native gather is
        bounded like the node-window gather's: a peer that died makes it raise."""
        local = self.agent.window_buckets(self.bounds)
        node = self.aggregator.all_gather(local)
        self._await(node)
        if not self.is_root:
            return None
        per_gpu = node.detach().to("cpu").numpy().astype(np.float32, copy=True)
        return per_gpu, per_gpu.sum(axis=0, dtype=np.float64).astype(np.float32)

    def _await(self, node) -> None:
        tr = self.aggregator.native
        if tr is None or not node.is_cuda or not hasattr(tr, "publisher"):
            return  # identity / host gathers are synchronous already
        import torch

        from .node import await_publication

        if self._pub is None:
            self._pub = tr.publisher(False)
        seq = self._pub.publish(0, 0, 0, torch.cuda.current_stream(node.device).cuda_stream)
        try:
            await_publication(self._pub, seq, tr, self.collective_timeout_s, what="window-bucket gather",
                              abandon=self.aggregator.abandon)
        except RuntimeError:
            if not tr.healthy():
                self.aggregator.native = None
            raise

"""Every hipGraph of the optimisers and solvers is recorded here (``torch.cuda.CUDAGraph`` is hipGraph on ROCm).
The warm-up runs on a side stream joined back to the caller's, as torch documents for ``torch.cuda.graph``."""

from typing import Any, Callable, Optional, Sequence, Tuple

import torch


def capture_graph(body: Callable[[], Any], warmups: int = 1, restore: Sequence[torch.Tensor] = (),
                  warmup: Optional[Callable[[], Any]] = None, device=None) -> Tuple["torch.cuda.CUDAGraph", Any]:
    """``warmups`` eager runs of ``warmup`` (default: ``body``), then ``body`` recorded into one graph.
    Returns the graph and what the recorded ``body`` returned (its outputs live in the graph's memory)."""
    saved = [t.clone() for t in restore]
    cur = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(warmups):
            (warmup or body)()
    cur.wait_stream(side)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    for t, s in zip(restore, saved):
        t.copy_(s)
    return graph, out

"""The small pieces every captured path in the engine shares: the module
under a DDP wrapper, its recurrent-state holder, the autocast context and
the warm-up / roll-back / capture sequence of a hipGraph."""

from __future__ import annotations

import contextlib

import torch

__all__ = ["unwrap", "state_holder", "amp_autocast", "capture_graph"]


def unwrap(model):
    """The module under a DDP wrapper (the model itself without one)."""
    return model.module if hasattr(model, "module") else model


def state_holder(model):
    """The submodule whose ``.state`` carries the recurrence, or None."""
    return getattr(unwrap(model), "time_propagate", None)


def amp_autocast(amp_dtype, device, cache_enabled: bool = True):
    """Autocast context for `amp_dtype` on a CUDA device, else a no-op.
    Captured bodies pass ``cache_enabled=False``: a cached weight cast made
    during capture would not be re-run by a replay."""
    if amp_dtype is None or torch.device(device).type != "cuda":
        return contextlib.nullcontext()
    return torch.autocast("cuda", dtype=amp_dtype, cache_enabled=cache_enabled)


def capture_graph(body, *, warmup: int, device=None, after_warmup=None,
                  pool=None):
    """Record ``body()`` into a hipGraph; returns ``(graph, out)`` with `out`
    what the recorded call returned (its static output tensors).

    `body` first runs `warmup` times on a side stream (library plans,
    autograd and optimizer-state allocations).  Those runs are real:
    `after_warmup` is where the caller undoes what they changed.  Capture
    itself records and does not execute, so the first replay starts from the
    state `after_warmup` left behind."""
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(warmup):
            body()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    if after_warmup is not None:
        after_warmup()
        torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=pool):
        out = body()
    torch.cuda.synchronize(device)
    return graph, out

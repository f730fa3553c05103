"""Write log and age census helpers (``gs_note_writes`` / ``gs_age_census``, include/gossip_sim.h).

The write log is ``u32 log[n_cols][WL]``: entry ``[jl][v]`` holds the tick at which owner column ``jl``'s own
``max_version`` was first seen equal to ``v`` (``GS_NONE``: never seen; entry 0 unused).  Every effective owner write
raises ``max_version`` by exactly one (``aiocluster/state.py:137-180``), so noting the owners' versions after each
write batch logs every write, and a no-op (a same-value ``set``, a ``delete`` of an absent key) logs nothing.

``note_writes_host`` is the definition of ``gs_note_writes``; the histogram helpers turn the census's power-of-two
buckets (``GS_VC_BUCKETS``' rule, in ticks of 1/64 s) into "p50 / p99 below X s" bounds.
"""

from __future__ import annotations

import math

import numpy as np

from ._lib import GS_AC_BUCKETS, GS_NONE, TICK_US, write_log_words

__all__ = ["write_log_words", "new_log_host", "alloc_log", "note_writes_host", "bucket", "bucket_bound_ticks",
           "quantile_bound_ticks", "quantile_bound_s", "ticks_to_s", "hist_summary"]


def new_log_host(n_cols: int, wl: int) -> np.ndarray:
    """An empty host log: every entry ``GS_NONE``."""
    return np.full((n_cols, wl), GS_NONE, dtype=np.uint32)


def alloc_log(torch, device, n_cols: int, wl: int):
    """The device log's memory (int32 [n_cols, wl], uninitialised: ``gs_write_log_init`` fills it)."""
    return torch.empty((n_cols, wl), dtype=torch.int32, device=device)


def note_writes_host(log: np.ndarray, self_mv, tick: int) -> np.ndarray:
    """``gs_note_writes`` on a host log, in place: for every owner column ``jl`` with ``v = self_mv[jl] > 0`` whose
    entry ``log[jl][v]`` is still ``GS_NONE``, store ``tick``.  Returns ``log``."""
    v = np.asarray(self_mv).astype(np.int64)
    if v.shape != (log.shape[0],):
        raise ValueError(f"self_mv of shape {v.shape} for a log of {log.shape[0]} owner columns")
    jl = np.flatnonzero((v > 0) & (v < log.shape[1]))
    jl = jl[log[jl, v[jl]] == GS_NONE]
    log[jl, v[jl]] = np.uint32(tick)
    return log


def bucket(x: int) -> int:
    """The histogram bucket of ``x`` ticks: 0 for 0, else min(19, bit length)."""
    return 0 if x == 0 else min(GS_AC_BUCKETS - 1, int(x).bit_length())


def bucket_bound_ticks(b: int) -> float:
    """The smallest number of ticks that every value of bucket ``b`` is below or equal to: bucket 0 holds 0 only,
    bucket b >= 1 values below 2^b, the last bucket has no bound."""
    if not 0 <= b < GS_AC_BUCKETS:
        raise ValueError(f"bucket {b}")
    if b == GS_AC_BUCKETS - 1:
        return math.inf
    return 0.0 if b == 0 else float(1 << b)


def quantile_bound_ticks(hist, q: float) -> float | None:
    """An upper bound in ticks of the ``q`` quantile (0 < q <= 1) of a bucketed histogram: the bound of the first
    bucket at which the cumulative count reaches ``ceil(q * total)``.  ``None`` for an empty histogram."""
    if not 0.0 < q <= 1.0:
        raise ValueError(f"quantile {q}")
    h = [int(x) for x in hist]
    total = sum(h)
    if total == 0:
        return None
    need = max(1, math.ceil(q * total))
    acc = 0
    for b, c in enumerate(h):
        acc += c
        if acc >= need:
            return bucket_bound_ticks(b)
    raise AssertionError("unreachable")


def ticks_to_s(ticks: float) -> float:
    return ticks * TICK_US / 1e6


def quantile_bound_s(hist, q: float) -> float | None:
    t = quantile_bound_ticks(hist, q)
    return None if t is None else ticks_to_s(t)


def hist_summary(hist, max_ticks: int | None = None) -> dict:
    """``{"n", "p50_s", "p99_s"[, "max_s"]}`` of a bucketed histogram: the quantiles as upper bounds in seconds."""
    out = {"n": sum(int(x) for x in hist), "p50_s": quantile_bound_s(hist, 0.5), "p99_s": quantile_bound_s(hist, 0.99)}
    if max_ticks is not None:
        out["max_s"] = ticks_to_s(int(max_ticks))
    return out

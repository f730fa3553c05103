"""The age census (gs_age_census, include/gossip_sim.h) from numpy, written from its definition (no GPU).

Inputs are plain arrays -- each view's max_version, which pairs the observer knows, the owners' own max_version, a
write log and the counted rows -- so the same function serves device readback and the oracle's export.  It never
reads a result of the kernel.
"""

import numpy as np

GS_NONE = 0xFFFFFFFF
BUCKETS = 20
TOTALS = ("observers", "pairs", "unknown", "behind", "unlogged", "max_age", "spread_writes", "pending_writes",
          "unlogged_writes", "max_spread_latency", "max_pending_age")
HISTS = ("age_hist", "spread_hist", "pending_age_hist")


def bucket(x: int) -> int:
    return 0 if x == 0 else min(BUCKETS - 1, int(x).bit_length())


def hist_of(values) -> list[int]:
    v = np.asarray(values, dtype=np.int64).ravel()
    assert (v >= 0).all()
    edges = 1 << np.arange(BUCKETS - 1, dtype=np.int64)  # 1, 2, 4 .. 2^18: bucket = the edges at or below the value
    return np.bincount(np.searchsorted(edges, v, side="right"), minlength=BUCKETS).tolist()


def age_census_ref(ver, known, M, log, tick, up=None, done=None) -> dict:
    """``ver`` [N][nc]: each view's max_version; ``known`` [N][nc] bool (a pair the observer does not know is a view
    at version 0); ``M`` [nc]: the owners' own; ``log`` u32 [nc][WL]; ``up`` [N] or None (all rows); ``done`` [nc] or
    None.  Returns the totals, the three histograms, ``owner_floor`` [nc], ``row_max_age`` [N] and ``done`` (the
    updated copy, or None)."""
    ver = np.asarray(ver).astype(np.int64)
    known = np.asarray(known).astype(bool)
    M = np.asarray(M).astype(np.int64)
    log = np.asarray(log).astype(np.int64)
    n, nc = ver.shape
    rows = np.ones(n, bool) if up is None else np.asarray(up).astype(bool)
    v = np.where(known, ver, 0)
    assert (v <= M[None, :]).all()
    cnt = np.broadcast_to(rows[:, None], (n, nc))
    behind = cnt & (v < M[None, :])
    out = {"observers": int(rows.sum()), "pairs": int(rows.sum()) * nc, "unknown": int((cnt & ~known).sum()),
           "behind": int(behind.sum())}
    # the oldest write a view lacks: version v + 1 (only read where the view is behind, so v + 1 <= M)
    entry = log[np.arange(nc)[None, :], np.minimum(v + 1, log.shape[1] - 1)]
    logged = behind & (entry != GS_NONE)
    age = np.where(logged, tick - entry, 0)
    out["unlogged"] = int((behind & ~logged).sum())
    out["max_age"] = int(age.max()) if logged.any() else 0
    out["age_hist"] = hist_of(age[logged])
    out["row_max_age"] = age.max(1) if nc else np.zeros(n, np.int64)
    floor = np.where(cnt, v, M[None, :]).min(0) if n else M.copy()
    out["owner_floor"] = floor
    spread, pending, unlogged_w = [], [], 0
    new_done = None if done is None else np.asarray(done).astype(np.int64).copy()
    if out["observers"]:
        for j in range(nc):
            f = int(floor[j])
            d = f if done is None else int(new_done[j])
            if done is not None:
                for w in range(d + 1, f + 1):
                    if log[j, w] == GS_NONE:
                        unlogged_w += 1
                    else:
                        spread.append(tick - int(log[j, w]))
                new_done[j] = max(d, f)
            for w in range(max(d, f) + 1, int(M[j]) + 1):
                if log[j, w] == GS_NONE:
                    unlogged_w += 1
                else:
                    pending.append(tick - int(log[j, w]))
    out["spread_writes"], out["pending_writes"], out["unlogged_writes"] = len(spread), len(pending), unlogged_w
    out["max_spread_latency"] = max(spread, default=0)
    out["max_pending_age"] = max(pending, default=0)
    out["spread_hist"], out["pending_age_hist"] = hist_of(spread), hist_of(pending)
    out["done"] = new_done
    return out


def assert_age_census(got: dict, want: dict, what=""):
    """Totals and histograms exactly; ``owner_floor`` / ``row_max_age`` whole where ``got`` has them (tensors or
    arrays)."""
    for k in TOTALS + HISTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("owner_floor", "row_max_age"):
        if k in got:
            g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
            g = g.astype(np.int64)
            assert g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k, np.flatnonzero(g != want[k])[:8])
    assert sum(got["age_hist"]) == got["behind"] - got["unlogged"], what
    assert sum(got["spread_hist"]) == got["spread_writes"] and sum(got["pending_age_hist"]) == got["pending_writes"]

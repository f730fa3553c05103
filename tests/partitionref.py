"""Network partitions: a numpy reference of the zoned detection census, and a scenario builder.

TEST INFRASTRUCTURE.  ``pairwise_reference`` is the detection census with the truth given PER PAIR -- ``truth[o, j]``
(is target ``j`` up for observer ``o``) and ``since[o, j]`` (since when it is not) -- so it states the zoned census
(include/gossip_sim.h: a target is reachable for an observer iff it is up and their zones are in one component)
without the per-component composition ``GossipSim.detect_census_zoned`` is built from.  ``detect_reference_for`` is
the same reference for ``gs_detect_census_for`` (rows = ``observers``, truth = ``up`` for every row).  Both take an
``export()`` dict and reuse ``detectref``'s decoding of it; every field is an integer, compared exactly.

``partition_scenario`` turns an ordinary scenario into one under a ``Topology`` with link events: per round the
pairs whose connect would fail are removed and the legs of the others drawn with the mirror
(``cuts.draw_cuts_zoned``), as ``driver.prepare`` does for a workload.
"""

import numpy as np
from detectref import BUCKETS, OLD_AGE, STATE_ONLY_ZERO, arrays_of_export, hist_of

from aiocluster_amd.cuts import draw_cuts_zoned
from aiocluster_amd.topology import LinkClock


def pairwise_reference(a: dict, obs, truth, since, tick: int, thresholds=(), col_lo: int = 0) -> dict:
    """``a``: detectref's arrays (st, tod, win, phi, age: [n, nc]); ``obs`` bool [n]; ``truth`` bool [n, nc];
    ``since`` int [n, nc] or None."""
    st, tod, win, phi = a["st"], a["tod"], a["win"], a["phi"]
    n, nc = st.shape
    obs = np.asarray(obs).astype(bool)
    cols = col_lo + np.arange(nc)
    pair = obs[:, None] & (cols[None, :] != np.arange(n)[:, None])
    upp, dnp = pair & truth, pair & ~truth
    live, dead = st == 1, st == 2
    out = {"observers": int(obs.sum())}
    for name, m in (("up", upp), ("down", dnp)):
        out[f"{name}_pairs"] = int(m.sum())
        out[f"{name}_live"] = int((m & live).sum())
        out[f"{name}_dead"] = int((m & dead).sum())
        out[f"{name}_unknown"] = int((m & (st == 0)).sum())
    thresholds = [float(x) for x in thresholds]
    hasphi = win & ~np.isnan(phi)
    if thresholds:
        out["up_windows"], out["down_windows"] = int((upp & win).sum()), int((dnp & win).sum())
        out["up_phi"], out["down_phi"] = int((upp & hasphi).sum()), int((dnp & hasphi).sum())
        out["old_windows"] = int((pair & hasphi & (a["age"] >= OLD_AGE)).sum())
    else:
        for k in STATE_ONLY_ZERO:
            out[k] = 0
    with np.errstate(invalid="ignore"):
        out["up_over"] = [int((upp & hasphi & (phi > t)).sum()) for t in thresholds]
        out["down_over"] = [int((dnp & hasphi & (phi > t)).sum()) for t in thresholds]
    fa = (tick - tod)[upp & dead]
    out["false_age_hist"] = hist_of(fa)
    out["max_false_age"] = int(fa.max()) if fa.size else 0
    out["early_deaths"] = 0
    out["detect_latency_hist"], out["undetected_age_hist"] = [0] * BUCKETS, [0] * BUCKETS
    out["max_detect_latency"] = out["max_undetected_age"] = 0
    if since is not None:
        ds = np.asarray(since).astype(np.int64)
        lat = tod - ds
        dd = dnp & dead
        ok = dd & (lat >= 0)
        out["early_deaths"] = int((dd & (lat < 0)).sum())
        out["detect_latency_hist"] = hist_of(lat[ok])
        out["max_detect_latency"] = int(lat[ok].max()) if ok.any() else 0
        und = np.maximum(tick - ds, 0)[dnp & live]
        out["undetected_age_hist"] = hist_of(und)
        out["max_undetected_age"] = int(und.max()) if und.size else 0
    out["false_suspicion_rate"] = out["up_dead"] / max(1, out["up_pairs"])
    out["detected_fraction"] = out["down_dead"] / max(1, out["down_pairs"])
    out["undetected"] = out["down_live"]
    pd = pair & dead
    out["target_live_by"] = (pair & live).sum(0).astype(np.int64)
    out["target_dead_by"] = pd.sum(0).astype(np.int64)
    big = np.iinfo(np.int64).max
    out["target_first_tod"] = np.where(pd.any(0), np.where(pd, tod, big).min(0), -1)
    out["target_last_tod"] = np.where(pd.any(0), np.where(pd, tod, -1).max(0), -1)
    out["row_false_suspicions"] = (upp & dead).sum(1).astype(np.int64)
    out["row_undetected"] = (dnp & live).sum(1).astype(np.int64)
    return out


def detect_reference_for(ex: dict, observers, up, down_since, tick: int, thresholds=(), prior5=None, col_lo=0) -> dict:
    """gs_detect_census_for over an export: rows = ``observers``, every row's truth = ``up``."""
    a = arrays_of_export(ex, tick, prior5)
    n, nc = a["st"].shape
    cols = col_lo + np.arange(nc)
    truth = np.broadcast_to(np.asarray(up).astype(bool)[cols][None, :], (n, nc))
    since = None
    if down_since is not None:
        since = np.broadcast_to(np.asarray(down_since).astype(np.int64)[cols][None, :], (n, nc))
    return pairwise_reference(a, observers, truth, since, tick, thresholds, col_lo)


def zoned_reference(ex: dict, up, topo, down_since, link_clock: LinkClock, tick: int, thresholds=(), prior5=None) -> dict:
    """The zoned census over an export of the whole matrix: observers = the up nodes, truth[o, j] = up[j] and the
    zones of o and j in one component, since[o, j] = the unreachable_since of o's component."""
    a = arrays_of_export(ex, tick, prior5)
    up = np.asarray(up).astype(bool)
    comp = topo.node_components()
    truth = up[None, :] & (comp[:, None] == comp[None, :])
    since = link_clock.unreachable_since(topo, up, down_since).astype(np.int64)[comp]  # [n, n]: row o = its component's
    return pairwise_reference(a, up, truth, since, tick, thresholds)


def cross_dead(ex: dict, up, topo_zone, comp_of_zone=None) -> int:
    """Pairs (o up, j up, o and j in different zones -- or different components of ``comp_of_zone``) with o holding
    j dead, over an export."""
    up = np.asarray(up).astype(bool)
    z = np.asarray(topo_zone).astype(np.int64)
    if comp_of_zone is not None:
        z = np.asarray(comp_of_zone)[z]
    dead = np.asarray(ex["tod"]) >= 0
    return int((dead & up[:, None] & up[None, :] & (z[:, None] != z[None, :])).sum())


def views_behind_reference(ex: dict, up, zone, n_zones: int) -> np.ndarray:
    """int64 [Z, Z]: [x, y] = the views of zone y's owners, held by the up observers of zone x, whose max_version is
    below the owner's own (the diagonal of ``mv``); a pair the observer does not know (``pos`` -1: never met, or
    removed by the failure detector's garbage collection) is unknown, not behind, as gs_view_census counts it."""
    mv = np.asarray(ex["mv"]).astype(np.int64)
    behind = (np.asarray(ex["pos"]) >= 0) & (mv < np.diag(mv)[None, :])
    up = np.asarray(up).astype(bool)
    zone = np.asarray(zone).astype(np.int64)
    out = np.zeros((n_zones, n_zones), dtype=np.int64)
    for x in range(n_zones):
        rows = behind[up & (zone == x)].sum(0)
        out[x] = np.bincount(zone, weights=rows, minlength=n_zones).astype(np.int64)
    return out


def partition_scenario(scen: dict, topo, link_events, seed: int) -> dict:
    """``scen`` (in place; returned) under ``topo`` with ``link_events`` [(round, action, args)]: per round
    ``"phases"`` keeps the pairs whose connect succeeds, ``"legs"`` their zoned draw, ``"all_phases"`` the pairs
    before the filter, ``"no_connect"`` the number removed and ``"topo"`` the round's snapshot of the links."""
    topo = topo.copy()
    for r, rd in enumerate(scen["rounds"]):
        for rr, action, args in link_events:
            if rr == r:
                topo.apply(action, args)
        snap = topo.copy()
        rd["topo"], rd["all_phases"], rd["legs"], rd["no_connect"] = snap, rd["phases"], [], 0
        kept = []
        for p, ph in enumerate(rd["all_phases"]):
            arr = np.asarray(ph, dtype=np.int64).reshape(-1, 2)
            legs = draw_cuts_zoned(arr[:, 0], arr[:, 1], seed, r, p, snap.zone, snap.link)
            ok = snap.connect_ok(arr[:, 0], arr[:, 1])
            assert np.array_equal(ok, legs != 255)
            rd["no_connect"] += int((~ok).sum())
            kept.append([[int(x), int(y)] for x, y in arr[ok]])
            rd["legs"].append([int(x) for x in legs[ok]])
        rd["phases"] = kept
    return scen

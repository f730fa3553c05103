"""A numpy reference of gs_detect_census (include/gossip_sim.h), shared by the host and the GPU tests.

``detect_reference`` takes either the canonical per-observer states of a golden fixture (``expect.states[r]``: the
real reference's ``live``, ``dead`` ``[j, tod]`` and ``windows`` ``[j, last, len, sum, phi]``, whose own phi values
it compares with the thresholds) or an ``export()`` dict (``live``, ``tod``, ``fd_last``, ``fd_len``, ``fd_sum``,
from which it computes phi with the binary64 expression of ``SamplingWindow.phi``, failure_detector.py:43-53).
"""

import numpy as np

BUCKETS = 20
OLD_AGE = 1 << 15
TOTALS = ("observers", "up_pairs", "up_live", "up_dead", "up_unknown", "down_pairs", "down_live", "down_dead",
          "down_unknown", "up_windows", "down_windows", "up_phi", "down_phi", "old_windows", "early_deaths",
          "max_detect_latency", "max_undetected_age", "max_false_age")
STATE_ONLY_ZERO = ("up_windows", "down_windows", "up_phi", "down_phi", "old_windows")
HISTS = ("detect_latency_hist", "undetected_age_hist", "false_age_hist")
TARGETS = ("target_live_by", "target_dead_by", "target_first_tod", "target_last_tod")
ROWS = ("row_false_suspicions", "row_undetected")


def bucket(x: int) -> int:
    return 0 if x == 0 else min(BUCKETS - 1, int(x).bit_length())


def hist_of(values) -> list[int]:
    v = np.asarray(values, dtype=np.int64).ravel()
    bounds = 1 << np.arange(BUCKETS - 1, dtype=np.int64)  # 1, 2, 4, ..., 2^18: values below bounds[b] are in buckets <= b
    return np.bincount(np.searchsorted(bounds, v, side="right"), minlength=BUCKETS).tolist()


def arrays_of_states(states, n: int) -> dict:
    """state (0 / 1 / 2), tod, window flag and phi (NaN = None) as [n, n] arrays from a fixture's states."""
    st = np.zeros((n, n), np.int64)
    tod = np.full((n, n), -1, np.int64)
    win = np.zeros((n, n), bool)
    phi = np.full((n, n), np.nan)
    age = np.zeros((n, n), np.int64)
    for o, s in enumerate(states):
        for j in s["live"]:
            st[o, j] = 1
        for j, t in s["dead"]:
            st[o, j] = 2
            tod[o, j] = t
        for j, last, ln, sm, p in s["windows"]:
            win[o, j] = True
            if p is not None:
                phi[o, j] = p
    return {"st": st, "tod": tod, "win": win, "phi": phi, "age": age}


def arrays_of_export(ex: dict, tick: int, prior5: float) -> dict:
    live, tod = np.asarray(ex["live"]), np.asarray(ex["tod"]).astype(np.int64)
    st = np.where(tod >= 0, 2, np.where(live == 1, 1, 0)).astype(np.int64)
    last = np.asarray(ex["fd_last"]).astype(np.int64)
    win = last >= 0
    ln = np.asarray(ex["fd_len"]).astype(np.float64)
    age = np.where(win, tick - last, 0)
    age = np.where(age >= OLD_AGE, OLD_AGE, age)  # an old window decodes as tick - 2^15
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (np.asarray(ex["fd_sum"], dtype=np.float64) + prior5) / (ln + 5.0)
        phi = (age.astype(np.float64) * (1.0 / 64.0)) / mean
    phi = np.where(win & (ln > 0), phi, np.nan)
    return {"st": st, "tod": tod, "win": win, "phi": phi, "age": age}


def detect_reference(states_or_export, up, down_since, tick, thresholds=(), prior5=None, col_lo=0) -> dict:
    """The census of the given state: every total, histogram, ``up_over`` / ``down_over``, the per-target planes and
    the per-row counts, as ``GossipSim.detect_census`` returns them (tensors as int64 arrays, GS_NONE as -1).
    ``down_since`` may be None.  ``prior5`` (5 x initial_interval_s) is needed for an export."""
    up = np.asarray(up).astype(bool)
    n = len(up)
    if isinstance(states_or_export, dict):
        a = arrays_of_export(states_or_export, tick, prior5)
    else:
        a = arrays_of_states(states_or_export, n)
    st, tod, win, phi = a["st"], a["tod"], a["win"], a["phi"]
    nc = st.shape[1]
    cols = col_lo + np.arange(nc)
    tup = up[cols]
    pair = up[:, None] & (cols[None, :] != np.arange(n)[:, None])
    upp, dnp = pair & tup[None, :], pair & ~tup[None, :]
    live, dead = st == 1, st == 2
    out = {"observers": int(up.sum())}
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
    if down_since is not None:
        ds = np.asarray(down_since).astype(np.int64)[cols]
        lat = (tod - ds[None, :])
        dd = dnp & dead
        ok = dd & (lat >= 0)
        out["early_deaths"] = int((dd & (lat < 0)).sum())
        out["detect_latency_hist"] = hist_of(lat[ok])
        out["max_detect_latency"] = int(lat[ok].max()) if ok.any() else 0
        und = np.broadcast_to(np.maximum(tick - ds, 0)[None, :], st.shape)[dnp & live]
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


def assert_census(got: dict, want: dict, what=""):
    """Every field exact; device tensors against the reference's arrays."""
    for k in TOTALS + HISTS + ("up_over", "down_over", "false_suspicion_rate", "detected_fraction", "undetected"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in TARGETS + ROWS:
        if k in got:
            g = got[k].cpu().numpy().astype(np.int64)
            assert g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k, np.flatnonzero(g != want[k])[:8])
    assert got["up_pairs"] == got["up_live"] + got["up_dead"] + got["up_unknown"]
    assert got["down_pairs"] == got["down_live"] + got["down_dead"] + got["down_unknown"]
    assert sum(got["false_age_hist"]) == got["up_dead"]

"""How stale the views are, and how long a write takes to reach every node, round by round (GPU).

Runs a ``WorkloadSpec`` with the write log on (``GossipSim(write_log=True)``) and calls ``gs_age_census`` after every
round, against the round's up mask.  One JSON line per round:

* ``view_age``: of the views that are behind their owner, the age of the oldest write each lacks -- p50 / p99 as upper
  bounds (the census's buckets are powers of two of ticks of 1/64 s) and the exact maximum, in seconds;
* ``spread``: the writes found at every up node for the first time by this round's census, with the same bounds on their
  latency (write tick to this census's tick: quantised to the census, one per round here);
* ``pending``: the writes not yet everywhere, and the age of the oldest.

``--loss P`` loses each message with probability P.  ``--split R --heal S`` puts the nodes in two zones of equal size
and cuts the links between them in rounds [R, S): writes made on one side stay pending, and the ages grow, until the
heal.  The summary line gives the bounds over the whole run.

``--time`` measures, at the start of round ``--time-at`` (default: the last), after the round's writes and before its
first phase -- every fresh write then leaves n - 1 views behind, so ``--write-frac 0.2`` puts about 20 % of the views
behind -- the wall time of ``age_census`` (host clock around the blocking call) against ``view_census`` without
heartbeats on the same state, 2 warm-ups and the median of ``--reps`` >= 5 alternating repeats; and, over the rounds, the
HIP-event time of each round's ``gs_owner_writes`` batch and of the ``gs_note_writes`` after it.

    python tools/staleness.py [--nodes 4096] [--keys 16] [--rounds 12] [--write-frac 0.05] [--loss 0.0]
                              [--split R --heal S] [--quiet-from R] [--time] [--time-at R] [--reps 9]
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--fanout", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--write-frac", type=float, default=0.05, help="fraction of the nodes that write a key each round")
    ap.add_argument("--down-frac", type=float, default=0.0, help="steady-state fraction of nodes down (churn)")
    ap.add_argument("--loss", type=float, default=0.0, help="probability that a message is lost")
    ap.add_argument("--split", type=int, default=None, help="the round at whose start the two halves lose their links")
    ap.add_argument("--heal", type=int, default=None, help="the round at whose start they come back")
    ap.add_argument("--quiet-from", type=int, default=None, help="rounds >= this: no writes, every node up")
    ap.add_argument("--hist-cap", type=int, default=64)
    ap.add_argument("--time", action="store_true", help="time the age census against the view census")
    ap.add_argument("--time-at", type=int, default=None, help="the round at whose start to time (default: the last)")
    ap.add_argument("--reps", type=int, default=9, help="timed repeats (at least 5), after 2 warm-ups")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: a median of at least 5")
    if (args.split is None) != (args.heal is None):
        ap.error("--split and --heal come together")
    if args.split is not None and not 0 <= args.split < args.heal <= args.rounds:
        ap.error("0 <= --split < --heal <= --rounds")
    time_at = args.rounds - 1 if args.time_at is None else args.time_at
    if args.time and not 0 <= time_at < args.rounds:
        ap.error("--time-at: a round of the run")

    import torch

    from aiocluster_amd import driver
    from aiocluster_amd.scenario import DEFAULT_CFG
    from aiocluster_amd.sim import GossipSim
    from aiocluster_amd.staleness import hist_summary
    from aiocluster_amd.topology import Topology
    from aiocluster_amd.workload import WorkloadSpec, key_names, synthetic_node_ids

    n, K = args.nodes, args.keys
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    kw = {}
    if args.split is not None:  # two zones; a uniform loss is then every link's loss
        topo = Topology.blocks([0, n // 2, n])
        if args.loss:
            for x in range(2):
                for y in range(x, 2):
                    topo.set_link(x, y, loss=args.loss)
        kw = dict(topology=topo, link_events=[(args.split, "split", [[1]]), (args.heal, "heal_all", ())])
    else:
        kw = dict(loss=args.loss)
    spec = WorkloadSpec(n=n, k=K, fanout=args.fanout, seed=args.seed, init="warm", write_frac=args.write_frac,
                        down_frac=args.down_frac, cut_seed=args.seed, quiet_from=args.quiet_from, **kw)
    sim = GossipSim(synthetic_node_ids(n), key_names(K), dict(DEFAULT_CFG), init="warm", device=str(dev), fd_ring=False,
                    hist_cap=args.hist_cap, initial_ops=driver.boot_ops(n, K), tombstones=False, hb8=True, mv8=True,
                    write_log=True)
    plans = driver.prepare(spec, args.rounds, torch, dev)
    total = {k: [0] * 20 for k in ("age_hist", "spread_hist")}
    maxima = {"max_age": 0, "max_spread_latency": 0, "max_pending_age": 0}
    spread_total = 0
    timing, write_ms, note_ms = None, [], []
    for rd in plans:
        if args.time:  # driver.begin, with the write batch and its note between HIP events
            if rd["nops"]:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record(sim.stream)
                sim._chk(sim.L.gs_owner_writes(sim.h, C.c_void_p(rd["ops"].data_ptr()), rd["nops"], rd["t"]),
                         "gs_owner_writes")
                ev[1].record(sim.stream)
                sim.note_writes(rd["t"])
                ev[2].record(sim.stream)
                ev[2].synchronize()
                write_ms.append(ev[0].elapsed_time(ev[1]))
                note_ms.append(ev[1].elapsed_time(ev[2]))
            sim._chk(sim.L.gs_begin_round(sim.h, C.c_void_p(rd["up"].data_ptr()), rd["t"]), "gs_begin_round")
            if rd["r"] == time_at:
                timing = time_census(sim, rd, args)
        else:
            driver.begin([sim], rd)
        driver.run_phases([sim], rd)
        driver.end([sim], rd)
        c = sim.age_census(up=rd["up"], tick=rd["t_live"])
        for k in total:
            total[k] = [a + b for a, b in zip(total[k], c[k])]
        for k in maxima:
            maxima[k] = max(maxima[k], c[k])
        spread_total += c["spread_writes"]
        print(json.dumps({
            "round": rd["r"], "tick": rd["t_live"], "observers": c["observers"], "behind": c["behind"],
            "behind_frac": c["behind"] / max(1, c["pairs"]), "unlogged": c["unlogged"],
            "view_age": hist_summary(c["age_hist"], c["max_age"]),
            "spread": hist_summary(c["spread_hist"], c["max_spread_latency"]),
            "pending": {"n": c["pending_writes"], "oldest_s": c["max_pending_age"] / 64.0},
        }), flush=True)
    out = {
        "tool": "staleness",
        "workload": f"N={n} K={K} F={args.fanout} warm, hb8mv8, write_frac {args.write_frac:g}, loss {args.loss:g}"
                    + (f", halves split in rounds [{args.split}, {args.heal})" if args.split is not None else "")
                    + f", {args.rounds} rounds",
        "view_age_over_the_run": hist_summary(total["age_hist"], maxima["max_age"]),
        "spread_latency_over_the_run": hist_summary(total["spread_hist"], maxima["max_spread_latency"]),
        "writes_spread": spread_total, "writes_pending_at_the_end": c["pending_writes"],
        "oldest_pending_s": maxima["max_pending_age"] / 64.0,
    }
    if timing:
        timing["owner_writes_ms_median"] = statistics.median(write_ms) if write_ms else None
        timing["note_writes_ms_median"] = statistics.median(note_ms) if note_ms else None
        timing["write_batches"] = len(write_ms)
        out["timing"] = timing
    sim.check()
    print(json.dumps(out))
    sim.close()


def time_census(sim, rd, args) -> dict:
    """Wall time of the two blocking censuses on the state as it stands (mid-round), alternating, after 2 warm-ups."""
    def wall(fn):
        sim.sync()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    age = lambda: sim.age_census(up=rd["up"], spread=False)  # noqa: E731  (done untouched: the run's own census credits)
    view = lambda: sim.view_census(up=rd["up"])  # noqa: E731
    for _ in range(2):
        a, v = age(), view()
    ta, tv = [], []
    for _ in range(args.reps):
        ta.append(wall(age))
        tv.append(wall(view))
    ma, mv = statistics.median(ta), statistics.median(tv)
    return {
        "state": f"start of round {rd['r']}: writes in, no phase yet", "nodes": sim.n,
        "behind_frac": a["behind"] / max(1, a["pairs"]), "view_census_behind": v["behind"],
        "age_census_ms": {"median": ma, "min": min(ta), "max": max(ta), "reps": args.reps},
        "view_census_ms": {"median": mv, "min": min(tv), "max": max(tv), "reps": args.reps},
        "age_over_view": ma / mv,
    }


if __name__ == "__main__":
    main()

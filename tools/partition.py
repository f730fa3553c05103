"""A split-and-heal curve: what a partition does to detection and to the data, round by round (GPU).

The nodes lie in ``--zones`` zones of equal size.  At round ``--split-at`` the last zone loses its links to the rest
(it stays up and keeps gossiping inside itself); at round ``--heal-at`` the links come back.  ``--cross-loss`` is the
loss of every link between two different zones while it is up.  After every round one JSON line with, per component
of the network:

* the zoned detection census (``GossipSim.detect_census_zoned``: one gs_detect_census_for call per component, truth =
  reachability): the unreachable targets still held live and those held dead, the detection latency of the split (median
  and highest bucket, in ticks of 1/64 s: 0, then 2^(b-1) <= x < 2^b) and the false suspicions inside the component;
* ``views_behind``: the zone x zone matrix of views that are behind their owner (``topology.views_behind``: one
  gs_view_census per observer zone, ``owner_behind`` summed by owner zone) -- how far each side's data has spread into
  the other.

``cross_side_held_dead`` counts the pairs (observer up, target up) on different sides of the cut -- the split-off zone
and the rest -- with the observer holding the target dead: two gs_detect_census_for calls (one side's rows against the
other side's up nodes), during the split and after it.  From ``--quiet-from`` on (default: the heal) nothing is written
and every node is up, so the data can converge.  The summary line gives, after the heal, the round at which the matrix
is back to zero off the diagonal, the round at which nobody holds a node of the other side dead any more, and the round
at which no reachable target at all is held dead (false suspicions inside a side included; with a low phi threshold
that may never happen).

``--time`` adds, on the last split round's state, the HIP-event time (2 warm-ups, the median of ``--reps`` >= 5) of the
two zoned kernels (gs_draw_cuts_zoned over a phase's exchanges, gs_filter_targets_zoned over the selected targets) and
of a zoned census against one gs_detect_census call at the same size.

    python tools/partition.py [--nodes 4096] [--zones 4] [--split-at 4] [--heal-at 10] [--rounds 20]
                              [--cross-loss 0.0] [--quiet-from R] [--peer-select] [--time]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--fanout", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--zones", type=int, default=4, help="zones of equal size (at most 16); the last one is split off")
    ap.add_argument("--split-at", type=int, default=4, help="the round at whose start the last zone loses its links")
    ap.add_argument("--heal-at", type=int, default=10, help="the round at whose start they come back")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--cross-loss", type=float, default=0.0, help="loss of a message between two different zones")
    ap.add_argument("--quiet-from", type=int, default=None,
                    help="rounds >= this: no writes, every node up (default: --heal-at)")
    ap.add_argument("--down-frac", type=float, default=0.0, help="steady-state fraction of nodes down (churn)")
    ap.add_argument("--peer-select", action="store_true",
                    help="the reference's own peer selection on the device (gs_select_peers), filtered per link")
    ap.add_argument("--phi-threshold", type=float, default=None, help="the detector's threshold (default 8)")
    ap.add_argument("--initial-interval", type=float, default=None, help="initial_interval_s (default 5)")
    ap.add_argument("--thresholds", default="", help="phi thresholds swept by every census (at most 16)")
    ap.add_argument("--time", action="store_true", help="time the zoned kernels and a zoned census")
    ap.add_argument("--reps", type=int, default=9, help="timed repeats (at least 5), after 2 warm-ups")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: a median of at least 5")
    if not 2 <= args.zones <= 16:
        ap.error("--zones: 2..16")
    if not 0 <= args.split_at < args.heal_at <= args.rounds:
        ap.error("0 <= --split-at < --heal-at <= --rounds")
    thresholds = [float(x) for x in args.thresholds.split(",") if x]

    import numpy as np
    import torch

    from aiocluster_amd import detect, driver
    from aiocluster_amd.peers import PeerSelector
    from aiocluster_amd.scenario import DEFAULT_CFG
    from aiocluster_amd.sim import GossipSim
    from aiocluster_amd.topology import LinkClock, Topology, views_behind
    from aiocluster_amd.workload import WorkloadSpec, key_names, synthetic_node_ids

    n, K, Z = args.nodes, args.keys, args.zones
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = dict(DEFAULT_CFG)
    if args.phi_threshold is not None:
        cfg["phi_threshold"] = args.phi_threshold
    if args.initial_interval is not None:
        cfg["initial_interval_s"] = args.initial_interval
    topo = Topology.blocks([n * z // Z for z in range(Z + 1)])
    if args.cross_loss:
        for x in range(Z):
            for y in range(x + 1, Z):
                topo.set_link(x, y, loss=args.cross_loss)
    events = [(args.split_at, "split", [[Z - 1]]), (args.heal_at, "heal_all", ())]
    spec = WorkloadSpec(n=n, k=K, fanout=args.fanout, seed=args.seed, init="warm", write_frac=0.05,
                        down_frac=args.down_frac, cut_seed=args.seed,
                        quiet_from=args.heal_at if args.quiet_from is None else args.quiet_from, topology=topo,
                        link_events=events)
    sim = GossipSim(synthetic_node_ids(n), key_names(K), cfg, init="warm", device=str(dev), fd_ring=False, hist_cap=64,
                    initial_ops=driver.boot_ops(n, K), tombstones=False, hb8=True, mv8=True)
    sel = PeerSelector(sim, fanout=args.fanout, seed=args.seed) if args.peer_select else None
    plans = driver.prepare(spec, args.rounds, torch, dev)
    down, links = detect.DownClock(n), LinkClock(Z)
    data_back = detect_back = cross_back = None
    far = topo.zone == Z - 1  # the two sides of the cut
    timing = None
    for rd in plans:
        driver.run_round([sim], rd, sel=sel)
        r, t = rd["r"], rd["topo"]
        down.update(rd["up_host"], rd["t"])
        links.update(t, rd["t"])
        c = sim.detect_census_zoned(rd["up_host"], t, down, links, thresholds, rd["t_live"], per_component=True)
        m = views_behind(sim, rd["up_host"], t)
        comps = t.components()
        off = int(m.sum() - np.trace(m))
        up_h = rd["up_host"].astype(bool)
        cross = sum(sim.detect_census((up_h & b).astype(np.uint8), rd["t_live"],
                                      observers=(up_h & a).astype(np.uint8))["up_dead"]
                    for a, b in ((far, ~far), (~far, far)))
        if r >= args.heal_at:
            if data_back is None and off == 0:
                data_back = r
            if detect_back is None and c["up_dead"] == 0:
                detect_back = r
            if cross_back is None and cross == 0:
                cross_back = r
        print(json.dumps({
            "round": r, "exchanges": rd["exchanges"], "no_connect": rd["no_connect"],
            "components": [{
                "zones": zs, "observers": p["observers"],
                "unreachable_held_live": p["down_live"], "unreachable_held_dead": p["down_dead"],
                "detect_latency_median_bucket": detect.hist_quantile_bucket(p["detect_latency_hist"]),
                "detect_latency_max_bucket": detect.max_bucket(p["detect_latency_hist"]),
                "max_detect_latency": p["max_detect_latency"],
                "false_suspicions": p["up_dead"], "false_suspicion_rate": p["false_suspicion_rate"],
                "views_behind_by_owner_zone": m[zs].sum(0).tolist(),
            } for zs, p in zip(comps, c["components"])],
            "reachable_held_dead": c["up_dead"], "cross_side_held_dead": cross, "views_behind": m.tolist(), "views_behind_off_diagonal": off,
        }), flush=True)
        if args.time and r == args.heal_at - 1:
            timing = time_kernels(sim, sel, rd, down, links, thresholds, args, torch, statistics)
    out = {
        "tool": "partition",
        "workload": f"N={n} K={K} F={args.fanout} warm, hb8mv8; {Z} zones, zone {Z - 1} split off in rounds "
                    f"[{args.split_at}, {args.heal_at}) of {args.rounds}, cross-zone loss {args.cross_loss:g}, "
                    + ("device peer selection" if sel else "explicit schedule"),
        "phi_threshold": cfg["phi_threshold"],
        "views_behind_zero_off_diagonal_at_round": data_back,
        "no_node_of_the_other_side_held_dead_at_round": cross_back,
        "no_reachable_target_held_dead_at_round": detect_back,
    }
    if timing:
        out["timing"] = timing
    sim.check()
    print(json.dumps(out))
    sim.close()


def time_kernels(sim, sel, rd, down, links, thresholds, args, torch, statistics) -> dict:
    """HIP-event times on the sim's stream: the two zoned kernels, and a zoned census against one gs_detect_census."""
    import numpy as np

    from aiocluster_amd.peers import PeerSelector

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(sim.stream)
            fn()
            e1.record(sim.stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "reps": args.reps}

    n, t = sim.n, rd["topo"]
    rng = np.random.default_rng(1)
    m = n // 2  # a phase of a perfect matching
    perm = rng.permutation(n).astype(np.int32)
    ini, res = sim._pairs_dev(perm[:m], perm[m:2 * m])
    legs = torch.empty(m, dtype=torch.uint8, device=sim.device)
    t_draw = timed(lambda: sim.draw_cuts_zoned(ini, res, 1, rd["r"], 0, rd["zone"], rd["link"], out=legs))
    psel = sel or PeerSelector(sim, fanout=args.fanout, seed=args.seed)
    psel.select(rd["up"], rd["r"])
    scratch = torch.empty_like(psel.targets)
    t_filter = timed(lambda: sim.filter_targets(psel.targets, rd["zone"], rd["link"], out=scratch))
    ds = sim._dev(down.down_since.view("int32"), torch.int32)
    tick = rd["t_live"]
    t_one = timed(lambda: sim.detect_census(rd["up"], tick, ds))
    t_zoned = timed(lambda: sim.detect_census_zoned(rd["up_host"], t, down, links, (), tick))
    out = {
        "state": f"after round {rd['r']} (the last split round), {len(t.components())} components",
        "draw_cuts_zoned": {**t_draw, "exchanges": m}, "filter_targets_zoned": {**t_filter, "targets": int(scratch.numel())},
        "detect_census": t_one, "detect_census_zoned": t_zoned,
        "zoned_over_single": t_zoned["median_ms"] / t_one["median_ms"],
    }
    if thresholds:
        t_one_phi = timed(lambda: sim.detect_census(rd["up"], tick, ds, thresholds))
        t_zoned_phi = timed(lambda: sim.detect_census_zoned(rd["up_host"], t, down, links, thresholds, tick))
        out.update(detect_census_phi=t_one_phi, detect_census_zoned_phi=t_zoned_phi,
                   zoned_over_single_phi=t_zoned_phi["median_ms"] / t_one_phi["median_ms"])
    return out


if __name__ == "__main__":
    main()

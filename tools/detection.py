"""What the failure detector makes of a cluster with churn, loss or a partition (GPU).

A seeded workload runs with nodes going down for a few rounds at a time; after every round one gs_detect_census
call compares the detector's live / dead sets (FailureDetector.live_nodes / dead_nodes,
aiocluster/failure_detector.py:60-67) with the truth: one JSON line per round with the false-suspicion rate, the
share of the failures detected, the median and the highest bucket of the detection latency (buckets in ticks of
1/64 s: 0, then 2^(b-1) <= x < 2^b) and the longest-standing false suspicion.  The summary line sweeps
phi_threshold over the last round's windows (detect.roc: the share of up targets a detector with that threshold
would suspect against the share of down targets it would).

``--time`` adds the census's own cost on the last round's state, from HIP events on the sim's stream (2 warm-ups,
the median of ``--reps`` >= 5): the state-only pass (1 B per pair) and the pass with thresholds (7 B per pair),
beside the k_liveness time of the same run (gs_kernel_times), which reads the same 7 B and writes 6.

    python tools/detection.py [--nodes 4096] [--rounds 12] [--down-frac 0.05] [--down-rounds 3] [--loss 0.1]
                              [--partition A B] [--thresholds 2,4,8,12] [--layout hb8mv8] [--time]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LAYOUTS = {
    "hb8mv8": dict(tombstones=False, hb8=True, mv8=True),  # the layout bench.py measures
    "hb8": dict(tombstones=False, hb8=True),
    "u16": dict(tombstones=False),
    "tombstones": dict(tombstones=True),
    "no_held": dict(tombstones=False, held=False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--fanout", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--down-frac", type=float, default=0.05, help="steady-state fraction of nodes down")
    ap.add_argument("--down-rounds", type=int, default=3, help="rounds a node stays down")
    ap.add_argument("--loss", type=float, default=0.0, help="probability that a Syn / SynAck / Ack is lost")
    ap.add_argument("--partition", type=int, nargs=2, metavar=("A", "B"), default=None,
                    help="rounds [A, B) with the cluster split in halves")
    ap.add_argument("--thresholds", default="2,4,8,12", help="phi thresholds swept over the last round (at most 16)")
    ap.add_argument("--layout", choices=list(LAYOUTS), default="hb8mv8")
    ap.add_argument("--phi-threshold", type=float, default=None, help="the detector's own threshold (default 8)")
    ap.add_argument("--initial-interval", type=float, default=None, help="initial_interval_s (default 5)")
    ap.add_argument("--time", action="store_true", help="time the census and k_liveness on the last round's state")
    ap.add_argument("--reps", type=int, default=9, help="timed repeats (at least 5), after 2 warm-ups")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: a median of at least 5")
    thresholds = [float(x) for x in args.thresholds.split(",") if x]

    import torch

    from aiocluster_amd import detect, driver
    from aiocluster_amd.scenario import DEFAULT_CFG
    from aiocluster_amd.sim import GossipSim
    from aiocluster_amd.workload import WorkloadSpec, key_names, synthetic_node_ids

    n, K = args.nodes, args.keys
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = dict(DEFAULT_CFG)
    if args.phi_threshold is not None:
        cfg["phi_threshold"] = args.phi_threshold
    if args.initial_interval is not None:
        cfg["initial_interval_s"] = args.initial_interval
    if args.layout == "no_held":
        cfg["mtu"] = 1 << 30  # version-only views: no NodeDelta may be cut
    spec = WorkloadSpec(n=n, k=K, fanout=args.fanout, seed=args.seed, init="warm", write_frac=0.05,
                        down_frac=args.down_frac, down_rounds=args.down_rounds,
                        partition=tuple(args.partition) if args.partition else None, loss=args.loss, cut_seed=args.seed)
    sim = GossipSim(synthetic_node_ids(n), key_names(K), cfg, init="warm", device=str(dev), fd_ring=False, hist_cap=64,
                    initial_ops=driver.boot_ops(n, K), **LAYOUTS[args.layout])
    plans = driver.prepare(spec, args.rounds, torch, dev)
    clock = detect.DownClock(n)
    if args.time:
        sim.set_timing(True)
    c = None
    for rd in plans:
        driver.run_round([sim], rd)
        ds = clock.update(rd["up_host"], rd["t"])
        last = rd is plans[-1]
        c = sim.detect_census(rd["up"], rd["t_live"], ds, thresholds if last else ())
        print(json.dumps({
            "round": rd["r"], "down": int(n - c["observers"]), "false_suspicion_rate": c["false_suspicion_rate"],
            "detected_fraction": c["detected_fraction"], "undetected": c["undetected"],
            "detect_latency_median_bucket": detect.hist_quantile_bucket(c["detect_latency_hist"]),
            "detect_latency_max_bucket": detect.max_bucket(c["detect_latency_hist"]),
            "max_detect_latency": c["max_detect_latency"], "max_false_age": c["max_false_age"],
            "early_deaths": c["early_deaths"]}), flush=True)
    rd = plans[-1]
    out = {
        "tool": "detection",
        "workload": f"N={n} K={K} F={args.fanout} warm, layout {args.layout}; {args.rounds} rounds, {args.down_frac:g} down "
                    f"for {args.down_rounds} rounds, loss {args.loss:g}"
                    + (f", partition in rounds [{args.partition[0]}, {args.partition[1]})" if args.partition else ""),
        "phi_threshold": cfg["phi_threshold"],
        "last_round": {k: c[k] for k in ("up_pairs", "up_dead", "down_pairs", "down_dead", "down_live", "up_windows",
                                          "down_windows", "up_phi", "down_phi", "old_windows")},
        "roc": [{"threshold": t, "false_suspicion_share": fs, "detected_share": dt}
                for t, fs, dt in detect.roc(c, thresholds)],
    }
    if args.time:
        kt = sim.kernel_times()["liveness"]

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

        ds_dev = sim._dev(ds.view("int32"), torch.int32)
        pairs = n * sim.ncol
        t_state = timed(lambda: sim.detect_census(rd["up"], rd["t_live"], ds_dev))
        t_phi = timed(lambda: sim.detect_census(rd["up"], rd["t_live"], ds_dev, thresholds))
        t_all = timed(lambda: sim.detect_census(rd["up"], rd["t_live"], ds_dev, thresholds, per_target=True, per_row=True))
        up_rows = c["observers"]  # rows of down observers are not read

        def tbs(nbytes, tm):
            return nbytes / (tm["median_ms"] * 1e-3) / 1e12

        out["timing"] = {
            "pairs": pairs, "rows_read": up_rows,
            "census_state_only": {**t_state, "bytes": up_rows * sim.np_, "TBps": tbs(up_rows * sim.np_, t_state)},
            "census_phi": {**t_phi, "bytes": up_rows * sim.np_ * 7, "TBps": tbs(up_rows * sim.np_ * 7, t_phi)},
            "census_phi_per_target_per_row": t_all,
            "k_liveness": {"mean_ms": kt[0] / max(1, kt[1]), "launches": kt[1]},
        }
    sim.check()
    print(json.dumps(out))
    sim.close()


if __name__ == "__main__":
    main()

"""What the gossip protocol costs on the wire, and what the reference's frame limit does to it (GPU).

A seeded workload runs; before every phase one gs_traffic_census call sizes the phase's Syn, SynAck and Ack frames
(aiocluster/server.py:327-370, 516-521) on the state as it stands, and the phase then runs with what the peers would
accept.  One JSON line per round: messages and bytes by kind, the digest share of all body bytes, the messages refused
as oversize by kind (``--frame-limit``: aiocluster/server.py:502-514), the ten busiest nodes by bytes sent, and beside
them gs_view_census's ``behind``, so the cost of a refused exchange shows as slower spread.

``--time`` adds the census's own cost on the last round's first phase, from HIP events on the sim's stream (2 warm-ups,
the median of ``--reps`` >= 5): the pass with ``legs_out`` alone and with every output, beside the pass-1 and packer
time per phase of the same run (gs_kernel_times).  Each census wave streams both rows of its exchange whole.

    python tools/traffic.py [--nodes 4096] [--rounds 6] [--loss 0.1] [--frame-limit] [--mtu 65507]
                            [--peer-select] [--time]
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
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--loss", type=float, default=0.0, help="probability that a Syn / SynAck / Ack is lost")
    ap.add_argument("--frame-limit", action="store_true", help="refuse frames larger than the mtu (_read_message)")
    ap.add_argument("--mtu", type=int, default=65507, help="Config.max_payload_size")
    ap.add_argument("--peer-select", action="store_true",
                    help="the reference's own peer selection (seeds 0-7 answer every phase) instead of the schedule")
    ap.add_argument("--wide-views", action="store_true", help="16-bit views instead of GS_HB8 + GS_MV8")
    ap.add_argument("--time", action="store_true", help="time the census on the last round's first phase")
    ap.add_argument("--reps", type=int, default=9, help="timed repeats (at least 5), after 2 warm-ups")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: a median of at least 5")

    import torch

    from aiocluster_amd import driver
    from aiocluster_amd.peers import PeerSelector
    from aiocluster_amd.scenario import DEFAULT_CFG
    from aiocluster_amd.sim import GossipSim
    from aiocluster_amd.workload import WorkloadSpec, key_names, synthetic_node_ids

    n, K = args.nodes, args.keys
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = dict(DEFAULT_CFG, mtu=args.mtu)
    spec = WorkloadSpec(n=n, k=K, fanout=args.fanout, seed=args.seed, init="warm", write_frac=0.05, down_frac=0.05,
                        down_rounds=3, loss=args.loss, cut_seed=args.seed, frame_limit=args.frame_limit)
    sim = GossipSim(synthetic_node_ids(n), key_names(K), cfg, init="warm", device=str(dev), tombstones=False,
                    fd_ring=False, hist_cap=64, initial_ops=driver.boot_ops(n, K), hb8=not args.wide_views,
                    mv8=not args.wide_views)
    sel = PeerSelector(sim, fanout=args.fanout, seeds=range(8), seed=args.seed) if args.peer_select else None
    plans = driver.prepare(spec, args.rounds, torch, dev)
    if args.time:
        sim.set_timing(True)
    nodes = torch.zeros((2, n), dtype=torch.int64, device=dev)
    kinds = ("syn", "synack", "ack")
    for rd in plans:
        nodes.zero_()
        rd["traffic_nodes"], rd["traffic_totals"] = nodes, True  # the census runs before every phase either way
        driver.run_round([sim], rd, sel=sel)
        t = rd["traffic"] or {}
        top = torch.topk(nodes[0], min(10, n))
        vc = sim.view_census(up=rd["up"])
        print(json.dumps({
            "round": rd["r"], "exchanges": t.get("exchanges", 0),
            "sent": dict(zip(kinds, t.get("sent", [0] * 3))), "delivered": dict(zip(kinds, t.get("delivered", [0] * 3))),
            "lost": dict(zip(kinds, t.get("lost", [0] * 3))), "rejected": dict(zip(kinds, t.get("rejected", [0] * 3))),
            "bytes_sent": dict(zip(kinds, t.get("bytes_sent", [0] * 3))),
            "bytes_delivered": dict(zip(kinds, t.get("bytes_delivered", [0] * 3))),
            "max_frame": dict(zip(kinds, t.get("max_frame", [0] * 3))), "digest_share": t.get("digest_share", 0.0),
            "busiest": [[int(i), int(b)] for i, b in zip(top.indices.cpu().tolist(), top.values.cpu().tolist())],
            "behind": vc["behind"], "max_version_lag": vc["max_version_lag"]}), flush=True)
    out = {"tool": "traffic",
           "workload": f"N={n} K={K} F={args.fanout} warm, {'16-bit' if args.wide_views else 'hb8+mv8'} views, mtu {args.mtu}; "
                       f"{args.rounds} rounds of 5% writes + 5% down churn, loss {args.loss:g}, frame limit "
                       f"{'on' if args.frame_limit else 'off'}, {'peer selection' if sel else 'explicit schedule'}",
           "cut_exchanges": sim.counters()["cut_exchanges"]}
    if args.time:
        kt = sim.kernel_times()
        rd = plans[-1]
        a, b, m, _ = next(p for p in rd["phases"] if p[2])
        tick = sim.latest_tick()

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

        lean = timed(lambda: sim.traffic_census(tick, (a, b), frame_limit=args.frame_limit, totals=False))
        full = timed(lambda: sim.traffic_census(tick, (a, b), frame_limit=args.frame_limit, per_exchange=True,
                                                nodes=nodes, totals=True))
        # per exchange: wave 0 streams both rows' max_version views and the initiator's heartbeats, wave 1 all four
        nbytes = m * 7 * sim.np_ * (2 if args.wide_views else 1)
        phases = max(1, kt["pass1"][1])
        out["timing"] = {
            "exchanges": m, "bytes_streamed": nbytes,
            "census_legs_out_only": {**lean, "TBps": nbytes / (lean["median_ms"] * 1e-3) / 1e12},
            "census_every_output": {**full, "TBps": nbytes / (full["median_ms"] * 1e-3) / 1e12},
            "pass1_ms_per_phase": kt["pass1"][0] / phases, "pack_ms_per_phase": kt["pack"][0] / max(1, kt["pack"][1]),
            "lite_ms_per_phase": kt["lite"][0] / max(1, kt["lite"][1]), "phases": phases,
        }
    sim.check()
    print(json.dumps(out))
    sim.close()


if __name__ == "__main__":
    main()

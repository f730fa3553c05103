"""Dissemination curve of fresh writes on the headline layout, and what the census costs (GPU).

A warm cluster (default 65,536 nodes, K = 16, fanout 3, 8-bit heartbeat and max_version views: the layout
bench.py measures) settles for a few rounds of the headline workload; then a handful of owners write one key
each, writes and churn stop, and after every round one gs_view_census call probes each fresh write
(owner, its new max_version): the rounds until 50 %, 99 % and 100 % of the nodes hold it (the anti-entropy of
aiocluster/state.py:340-415 at work).

It also times the census on that state with HIP events on the sim's stream -- without and with
GS_VC_HEARTBEATS, with the probes -- against the bytes it streams (1 B per view for GS_R_MV, 2 B with GS_R_HB),
the gs_stream_read ceiling and gs_check_heartbeat_lag (the k_hb_lag sweep over the same rows) measured in the
same run, and the earlier way to ask "did the version matrix converge": the chunked torch comparison of decoded
max_version words against the owners' own (16,384 rows at a time).  One JSON line.

    python tools/dissemination.py [--nodes 65536] [--settle 4] [--probes 6] [--rounds 12] [--reps 10]
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def chunked_torch_check(sim) -> tuple[int, int]:
    """The comparison the census replaces: (views above their owner's max_version, views below it)."""
    torch = sim.torch
    nc = sim.ncol
    own = sim.region("SELF_MV", torch.int32, (sim.np_,))[:nc]
    above = below = 0
    for r0 in range(0, sim.n, 16384):
        blk = sim.mv_words(slice(r0, r0 + 16384))[:, :nc] & 0x7FFF
        above += int((blk > own[None, :]).sum().item())
        below += int((blk < own[None, :]).sum().item())
    return above, below


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=65536)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--fanout", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--settle", type=int, default=4, help="rounds of the headline workload before the probes")
    ap.add_argument("--probes", type=int, default=6, help="fresh writes to follow (at most 64)")
    ap.add_argument("--rounds", type=int, default=12, help="quiet rounds after the writes")
    ap.add_argument("--reps", type=int, default=10, help="timed repeats of each measurement (after 2 warm-ups)")
    ap.add_argument("--wide-views", action="store_true", help="16-bit views instead of GS_HB8 + GS_MV8")
    ap.add_argument("--loss", type=float, default=0.0,
                    help="probability that a Syn / SynAck / Ack is lost (gs_run_phase_cut): the curve under loss")
    ap.add_argument("--frame-limit", action="store_true",
                    help="refuse frames larger than the mtu, as the reference's _read_message does (gs_traffic_census "
                         "before every phase): the curve of a real deployment")
    args = ap.parse_args()

    import numpy as np
    import torch

    from aiocluster_amd import driver
    from aiocluster_amd.scenario import DEFAULT_CFG
    from aiocluster_amd.sim import GossipSim
    from aiocluster_amd.workload import WorkloadSpec, key_names, round_tick, synthetic_node_ids

    n, K = args.nodes, args.keys
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = dict(DEFAULT_CFG)
    spec = WorkloadSpec(n=n, k=K, fanout=args.fanout, seed=args.seed, init="warm", write_frac=0.05, down_frac=0.05,
                        down_rounds=3, quiet_from=args.settle, loss=args.loss, cut_seed=args.seed,
                        frame_limit=args.frame_limit)
    sim = GossipSim(synthetic_node_ids(n), key_names(K), cfg, init="warm", device=str(dev), tombstones=False,
                    fd_ring=False, hist_cap=64, initial_ops=driver.boot_ops(n, K), hb8=not args.wide_views,
                    mv8=not args.wide_views)
    total = args.settle + args.rounds
    plans = driver.prepare(spec, total, torch, dev)
    for r in range(args.settle):
        driver.run_round([sim], plans[r])

    def timed(fn, reps=args.reps):
        """Median / min GPU milliseconds of fn over reps, from events on the sim's stream (2 warm-ups first)."""
        for _ in range(2):
            fn()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(sim.stream)
            fn()
            e1.record(sim.stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "reps": reps}

    settled = sim.view_census(heartbeats=True)
    # the census on the busy state (views behind after rounds with writes and churn: the per-view paths at work)
    t_busy = timed(lambda: sim.view_census())
    t_busy_hb = timed(lambda: sim.view_census(heartbeats=True))

    # the fresh writes: one key of a handful of owners spread over the index range, at the first quiet round's tick
    owners = [int(x) for x in np.linspace(0, n - 1, num=min(args.probes, 64, n), dtype=np.int64)]
    owners = sorted(set(owners))
    t = round_tick(args.settle)
    # (value ids above every id the boot writes and the workload use: a set of a key's current value is a no-op)
    ops = np.asarray([[j, i % K, 0, (1 << 28) + i, len(f"probe{i}")] for i, j in enumerate(owners)], dtype=np.uint32)
    sim.owner_writes(ops, t)
    M = sim.region("SELF_MV", torch.int32, (sim.np_,)).cpu().numpy()
    probes = [(j, int(M[j])) for j in owners]
    curve = [sim.view_census(probes=probes)["reach"]]
    per_round = []

    timing = None
    for r in range(args.settle, total):
        driver.run_round([sim], plans[r])
        c = sim.view_census(probes=probes)
        curve.append(c["reach"])
        per_round.append({"round": r - args.settle + 1, "behind": c["behind"], "max_version_lag": c["max_version_lag"],
                          "reach": c["reach"]})
        if r == args.settle:  # measured one round after the writes: the state still has views behind
            views = n * sim.ncol
            width = 1 if sim.mv8 else 2
            hwidth = 1 if sim.hb8 else 2
            t_mv = timed(lambda: sim.view_census(probes=probes))
            t_hb = timed(lambda: sim.view_census(heartbeats=True, probes=probes))
            t_all = timed(lambda: sim.view_census(heartbeats=True, probes=probes, per_owner=True, per_row=True))
            # the read ceiling: gs_stream_read over GS_R_MV's bytes, 16 B per lane
            mvr = sim.regions["MV"]
            sink = torch.zeros(1, dtype=torch.int64, device=dev)
            nb = mvr.numel() // 16 * 16
            t_rd = timed(lambda: sim._chk(sim.L.gs_stream_read(C.c_void_p(mvr.data_ptr()), nb, 16,
                                                               C.c_void_p(sink.data_ptr()),
                                                               C.c_void_p(sim.stream.cuda_stream)), "gs_stream_read"))
            ceiling = nb / (t_rd["median_ms"] * 1e-3) / 1e12
            # k_hb_lag over the same rows (reads both regions); timed last of the device passes, then the counters
            # it may have touched are checked
            t_lag = timed(sim.check_heartbeat_lag)
            lag_bytes = views * (hwidth + (1 if sim.mv8 else 0))
            t_old = timed(lambda: chunked_torch_check(sim), reps=max(2, args.reps // 3))
            above, below = chunked_torch_check(sim)
            now = sim.view_census()
            assert above == 0 and below == now["behind"], (above, below, now["behind"])

            def tbs(nbytes, tm):
                return nbytes / (tm["median_ms"] * 1e-3) / 1e12

            timing = {
                "views": views,
                "census_mv_busy_state": {**t_busy, "behind": settled["behind"]},
                "census_mv_hb_busy_state": t_busy_hb,
                "census_mv": {**t_mv, "bytes": views * width, "TBps": tbs(views * width, t_mv)},
                "census_mv_hb": {**t_hb, "bytes": views * (width + hwidth), "TBps": tbs(views * (width + hwidth), t_hb)},
                "census_mv_hb_per_owner_per_row": {**t_all, "bytes": views * (width + hwidth),
                                                   "TBps": tbs(views * (width + hwidth), t_all)},
                "stream_read_ceiling": {**t_rd, "bytes": nb, "TBps": ceiling},
                "hb_lag_sweep": {**t_lag, "bytes": lag_bytes, "TBps": tbs(lag_bytes, t_lag)},
                "chunked_torch_check": t_old,
                "census_mv_fraction_of_ceiling": tbs(views * width, t_mv) / ceiling,
                "census_mv_hb_fraction_of_ceiling": tbs(views * (width + hwidth), t_hb) / ceiling,
                "hb_lag_fraction_of_ceiling": tbs(lag_bytes, t_lag) / ceiling,
                "speedup_over_chunked_torch": t_old["median_ms"] / t_mv["median_ms"],
            }
    final = sim.view_census(heartbeats=True)
    sim.check()

    def rounds_to(frac, i):
        need = -(-int(frac * n * 1000) // 1000) if frac < 1 else n
        return next((r for r, reach in enumerate(curve) if reach[i] >= need), None)

    out = {
        "tool": "dissemination",
        "workload": f"N={n} K={K} F={args.fanout} warm, {'16-bit' if args.wide_views else 'hb8+mv8'} views; {args.settle} "
                    f"rounds of 5% writes + 5% down churn, then {len(probes)} fresh writes and {args.rounds} quiet rounds"
                    + (f"; message loss {args.loss}" if args.loss else ""),
        "loss": args.loss,
        "frame_limit": args.frame_limit,
        "cut_exchanges": sim.counters()["cut_exchanges"],
        "probes": [{"owner": j, "version": v, "rounds_to_50pct": rounds_to(0.5, i), "rounds_to_99pct": rounds_to(0.99, i),
                    "rounds_to_100pct": rounds_to(1.0, i)} for i, (j, v) in enumerate(probes)],
        "settled": {k: settled[k] for k in ("views", "behind", "inexact", "max_version_lag", "max_heartbeat_lag")},
        "final": {k: final[k] for k in ("views", "behind", "converged", "max_version_lag", "max_heartbeat_lag")},
        "rounds": per_round,
        "timing": timing,
    }
    print(json.dumps(out))
    sim.close()


if __name__ == "__main__":
    main()

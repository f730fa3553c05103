"""Framed exchanges (gs_traffic_census with GS_TC_FRAME_LIMIT): the scenarios of the reference's fixtures.

TEST INFRASTRUCTURE.  A framed scenario is an ordinary scenario with ``"frame_limit": true``; it may carry
``"net_legs"`` per round (what the network delivers, drawn by ``aiocluster_amd.cuts.draw_cuts``).  Its fixture
(tools/gen_traffic_fixture.py, from the real reference) adds per round ``"legs"`` -- the messages delivered AND
accepted, so an ordinary ``replay_round`` reproduces it -- and ``"traffic"``: per phase and exchange
``[syn_digest, synack_digest, synack_delta, ack_delta, syn_packet, synack_packet, ack_packet]`` in bytes, null for
a message that was never sent.
"""

import numpy as np

from aiocluster_amd.cuts import draw_cuts
from aiocluster_amd.scenario import make_scenario
from aiocluster_amd.workload import WorkloadSpec

CUT_SEED = 0xF4A3
FIXTURES = ["frame10", "framew12s"]


def pad_values(scen: dict, pad) -> dict:
    """Lengthen every written value: ``pad(owner, key, round)`` more bytes (round -1 = the boot writes)."""
    scen["initial"] = [[j, k, v + "x" * pad(j, k, -1)] for j, k, v in scen["initial"]]
    for r, rd in enumerate(scen["rounds"]):
        rd["writes"] = [[j, k, op, (v + "x" * pad(j, k, r)) if v else v] for j, k, op, v in rd["writes"]]
    return scen


def burst_writes(scen: dict, owner: int, per_round: int) -> dict:
    """``per_round`` more SETs by ``owner`` in every round it is up, to keys that rotate with the round."""
    k = len(scen["keys"])
    for r, rd in enumerate(scen["rounds"]):
        if rd["up"][owner]:
            rd["writes"] += [[owner, (5 * r + 3 * i + 1) % k, 0, f"b{owner}.{r}.{i}"] for i in range(per_round)]
    return scen


def frame10() -> dict:
    """Cold start, 10 nodes, deletes and TTL writes, churn with failure-detector garbage collection, window 5 (the
    rings roll over): digest entries carry last_gc, owners enter digests mid-exchange, scheduled-for-deletion and
    removals shorten them; 60 rounds take heartbeats, and one owner's max_version, past 128.  The frame limit alone cuts exchanges: a 10-entry digest fits the mtu, a SynAck that
    adds a delta to one, or an Ack with a long delta, often does not."""
    spec = WorkloadSpec(n=10, k=6, fanout=2, seed=710, init="cold", write_frac=0.5, delete_frac=0.2, ttl_frac=0.1,
                        down_frac=0.3, down_rounds=10)
    scen = make_scenario("frame10", spec, 60, {"mtu": 760, "tombstone_grace_s": 3, "window": 5, "max_interval_s": 1.0,
                                               "initial_interval_s": 1.0, "phi_threshold": 2.0, "dead_grace_s": 8.0})
    scen["frame_limit"] = True
    burst_writes(scen, owner=2, per_round=3)  # owner 2's max_version passes 128: two-byte varints in digests
    return pad_values(scen, lambda j, k, r: 24 + 7 * ((j + k) % 4))


def framew12s() -> dict:
    """Warm, 12 nodes, 13 keys, no deletes: every layout replays it, the 8-bit ones included.  Values of 60-150
    bytes make deltas fill the mtu, so Acks and SynAcks are refused whose delta body alone would fit; on top of
    that the network loses a quarter of the messages."""
    spec = WorkloadSpec(n=12, k=13, fanout=2, seed=1213, init="warm", write_frac=0.6, down_frac=0.3, down_rounds=4)
    scen = make_scenario("framew12s", spec, 40, {"mtu": 1900, "initial_interval_s": 1.0, "phi_threshold": 3.0})
    scen["frame_limit"] = True
    pad_values(scen, lambda j, k, r: 0 if r < 0 else 60 + 15 * ((j + 2 * k + r) % 7))
    for r, rd in enumerate(scen["rounds"]):
        rd["net_legs"] = []
        for p, ph in enumerate(rd["phases"]):
            arr = np.asarray(ph, dtype=np.int64).reshape(-1, 2)
            rd["net_legs"].append([int(x) for x in draw_cuts(arr[:, 0], arr[:, 1], CUT_SEED, r, p, 0.25)])
    return scen


CASES = {"frame10": frame10, "framew12s": framew12s}

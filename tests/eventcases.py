"""Scenarios of the hook-event tests that tests/manyphases.py does not have: the key-index and view-width edges.

``tests/test_gpu_events_layouts.py`` replays them on the device with events on, in lockstep with the C oracle;
``tests/test_eventcases_host.py`` shows on the oracle alone that each one has what its GPU case relies on.
"""

from aiocluster_amd.scenario import make_scenario
from aiocluster_amd.workload import WorkloadSpec

ROUNDS = 6


def cold_k64() -> dict:
    """32 nodes, 64 keys, cold (general layout), deletes and TTL writes, a binding mtu: records carry key indices
    past 31 (the key word is key | kind << 8, the kernels keep 64 keys' ordinals in 16 words)."""
    spec = WorkloadSpec(n=32, k=64, fanout=3, seed=64, init="cold", write_frac=0.6, delete_frac=0.15, ttl_frac=0.2,
                        down_frac=0.1, down_rounds=2)
    cfg = {"mtu": 1500, "tombstone_grace_s": 2, "phi_threshold": 3.0, "initial_interval_s": 1.0}
    return make_scenario("ev_cold_k64", spec, ROUNDS, cfg)


COLD_K64_KW = dict(fd_ring=True)


def warm_k16_esc() -> dict:
    """128 nodes, 16 keys (the widest the 8-bit layouts take), warm, a binding mtu, churn; run as hb8 + mv8 with
    four escape slots."""
    spec = WorkloadSpec(n=128, k=16, fanout=3, seed=16, init="warm", write_frac=0.3, down_frac=0.08, down_rounds=3)
    cfg = {"mtu": 400, "phi_threshold": 3.0, "initial_interval_s": 1.0}  # cuts ~70 deltas (nodes back from 3 rounds)
    return make_scenario("ev_warm_k16_esc", spec, ROUNDS, cfg)


WARM_K16_ESC_KW = dict(tombstones=False, fd_ring=False, hb8=True, mv8=True, esc_cols=4)


def warm_k37() -> dict:
    """96 nodes, 37 keys (10 of the kernels' 16 key words, the last one with a single key), warm, a binding mtu,
    churn; run with canonical prefix views."""
    spec = WorkloadSpec(n=96, k=37, fanout=3, seed=37, init="warm", write_frac=0.6, down_frac=0.08, down_rounds=3)
    cfg = {"mtu": 700, "phi_threshold": 3.0, "initial_interval_s": 1.0}
    return make_scenario("ev_warm_k37", spec, ROUNDS, cfg)


WARM_K37_KW = dict(tombstones=False, fd_ring=False)

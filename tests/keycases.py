"""Seeded scenarios for every key count: odd K (the key regions are strided by KP = round_up(K, 4) > K) and 17-63
keys (the 16-word key arrays of the KWB instantiations only partly used), each with an mtu that cuts NodeDeltas.

``tests/test_gpu_keycounts.py`` replays them on the device in every layout, in lockstep with the C oracle;
``tests/test_keycases_host.py`` shows on the oracle alone that each one has what its GPU case relies on.
"""

from aiocluster_amd.scenario import make_scenario
from aiocluster_amd.workload import WorkloadSpec

KEYS_SMALL = (1, 3, 5, 7, 13, 15)  # KW = 4: one to four key words, K % 4 != 0
KEYS_WIDE = (17, 20, 33, 47, 63, 64)  # KWB = 16: 5 to 16 key words
KEYS_ALL = KEYS_SMALL + KEYS_WIDE

FD = {"initial_interval_s": 1.0, "phi_threshold": 3.0}


def cold(K: int) -> dict:
    """96 nodes, cold (general layout): deletes, TTL writes, tombstone GC after 2 s, churn, ring windows of 6."""
    spec = WorkloadSpec(n=96, k=K, fanout=3, seed=100 + K, init="cold", write_frac=0.4, delete_frac=0.15,
                        ttl_frac=0.1, down_frac=0.1, down_rounds=3)
    cfg = {"mtu": 200 + 40 * K, "tombstone_grace_s": 2, "window": 6, "max_interval_s": 2.0, **FD}
    return make_scenario(f"keys_cold{K}", spec, 8, cfg)


def _warm(name: str, K: int, seed: int, tomb: bool) -> dict:
    spec = WorkloadSpec(n=160, k=K, fanout=3, seed=seed, init="warm", write_frac=0.3,
                        delete_frac=0.1 if tomb else 0.0, ttl_frac=0.05 if tomb else 0.0, down_frac=0.08,
                        down_rounds=3)
    return make_scenario(f"keys_{name}{K}", spec, 8, {"mtu": 300 + 10 * K, "tombstone_grace_s": 2, **FD})


def warm_tomb(K: int) -> dict:
    """160 nodes, warm (canonical layout), deletes, TTL writes and tombstone GC, churn."""
    return _warm("warm_tomb", K, 200 + K, True)


def warm_prefix(K: int, mtu: int | None = None) -> dict:
    """The same without deletes or TTL writes: the prefix-view layouts replay it.  ``mtu`` replaces 300 + 10 K (the
    version-only layout needs one that never binds)."""
    scen = _warm("warm_prefix", K, 300 + K, False)
    if mtu is not None:
        scen["config"]["mtu"] = mtu
    return scen


def _part(name: str, K: int, seed: int, tomb: bool) -> dict:
    spec = WorkloadSpec(n=128, k=K, fanout=2, seed=seed, init="warm", write_frac=1.0,
                        delete_frac=0.15 if tomb else 0.0, ttl_frac=0.1 if tomb else 0.0, partition=(1, 6),
                        down_frac=0.05, down_rounds=3)
    cfg = {"mtu": 500 + 6 * K, **FD}
    if tomb:
        cfg["tombstone_grace_s"] = 2
    return make_scenario(f"keys_{name}{K}", spec, 9, cfg)


def part_prefix(K: int) -> dict:
    """128 nodes, warm, every node writes a key a round, split in halves for rounds 1-5: after the heal every
    NodeDelta across the halves carries several keys, so the mtu cuts in the middle of a key list."""
    return _part("part_prefix", K, 400 + K, False)


def part_tomb(K: int) -> dict:
    """The same with deletes, TTL writes and tombstone GC."""
    return _part("part_tomb", K, 500 + K, True)


SCENARIOS = {"cold": cold, "warm_tomb": warm_tomb, "warm_prefix": warm_prefix, "part_prefix": part_prefix,
             "part_tomb": part_tomb}
TOMBSTONE_VARIANTS = ("cold", "warm_tomb", "part_tomb")

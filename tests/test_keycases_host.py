"""The scenarios of tests/keycases.py on the C oracle alone (CPU): each has the properties its GPU cases in
tests/test_gpu_keycounts.py rely on, so that no case passes because its input was tame."""

import functools

import numpy as np
import pytest
from helpers import make_backend
from keycases import KEYS_ALL, SCENARIOS, TOMBSTONE_VARIANTS
from oracle import OracleSim

from aiocluster_amd.scenario import replay


@functools.lru_cache(maxsize=None)
def run(kind, K):
    """(the scenario's shape, the oracle's counters, its final export)."""
    scen = SCENARIOS[kind](K)
    orc = make_backend(OracleSim, scen)
    replay(orc, scen)
    s, ex = orc.stats(), orc.export()
    orc.close()
    return (scen["n"], scen["k"], scen["init"], len(scen["rounds"])), s, ex


@pytest.mark.parametrize("K", KEYS_ALL)
@pytest.mark.parametrize("kind", list(SCENARIOS))
def test_scenario_has_what_its_gpu_cases_rely_on(kind, K):
    (n, k, init, rounds), s, ex = run(kind, K)
    assert k == K and init == ("cold" if kind == "cold" else "warm")
    assert (n, rounds) == {"cold": (96, 8), "warm_tomb": (160, 8), "warm_prefix": (160, 8), "part_prefix": (128, 9),
                           "part_tomb": (128, 9)}[kind]
    if K != 1:  # with one key a NodeDelta is sent whole or not at all
        assert s["truncated"] > 0
    if K == 1:  # and carries exactly one kv
        assert s["kvs_sent"] == s["node_deltas"] > 0
    elif kind.startswith("part_"):  # NodeDeltas of several keys: the mtu cuts in the middle of a key list
        assert s["kvs_sent"] >= 1.25 * s["node_deltas"], (s["kvs_sent"], s["node_deltas"])
    if kind in TOMBSTONE_VARIANTS:
        assert (ex["gc"] > 0).any() and (ex["kv_status"] != 0).any()
    else:
        assert not (ex["gc"] > 0).any() and not (ex["kv_status"] != 0).any()
    off = ~np.eye(n, dtype=bool)
    assert (ex["kv_version"][:, :, K - 1] > 0)[off].any()  # the last key is held in some view of another node

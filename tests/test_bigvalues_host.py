"""The large-value scenarios themselves (tests/bigvalues.py), on the C oracle and pbsize alone (CPU).

tests/test_gpu_bigvalues.py compares the device with the oracle on these scenarios; what makes that comparison
bite -- NodeDeltas of 65,536 bytes and more in the slots of the returning nodes, one of exactly 65,536, deltas cut
by the mtu -- is a property of the inputs, pinned here, so the GPU tests cannot pass for want of large sizes.
"""

import pytest
from bigvalues import EDGES, MAX_VALUE_LEN, big_values, sleeper_scenario
from helpers import make_backend
from oracle import OracleSim

from aiocluster_amd.scenario import make_scenario, replay_round
from aiocluster_amd.workload import WorkloadSpec

N, MTU, SLEEPERS, AWAY, AFTER = 128, 3_000_000, 4, 5, 3


@pytest.fixture(scope="module")
def sleeper():
    scen, sizes = sleeper_scenario(N, MTU, SLEEPERS, AWAY, AFTER)
    orc = make_backend(OracleSim, scen)
    per_round, prev = [], orc.stats()
    for r in range(len(scen["rounds"])):
        replay_round(orc, scen, r)
        s = orc.stats()
        per_round.append({k: s[k] - prev[k] for k in s})
        prev = s
    return scen, sizes, per_round


def test_sleeper_scenario_has_nodedeltas_past_64k(sleeper):
    scen, sizes, _ = sleeper
    writers = [j for j in range(N) if sizes[j]]
    assert writers == list(range(SLEEPERS, N)) and sizes[:SLEEPERS] == [0] * SLEEPERS
    big = [j for j in writers if sizes[j] >= 1 << 16]
    assert 2 * len(big) >= len(writers), (len(big), len(writers))
    assert sizes[5] == 1 << 16  # the designated owner: exactly 65,536 DeltaPb bytes
    assert any(0 < sizes[j] < 1 << 14 for j in writers)  # small NodeDeltas for first-fit continuation
    assert max(sizes) < 1 << 17


def test_sleeper_scenario_shape(sleeper):
    scen, _, _ = sleeper
    assert scen["init"] == "warm" and scen["k"] == 16 and scen["config"]["mtu"] == MTU
    for r, rd in enumerate(scen["rounds"]):
        away = r < AWAY
        assert rd["up"] == [0 if (away and o < SLEEPERS) else 1 for o in range(N)]
        assert all(min(a, b) >= SLEEPERS for ph in rd["phases"] for a, b in ph) or not away
        assert [(w[0], w[1], w[2]) for w in rd["writes"]] == ([(j, r, 0) for j in range(SLEEPERS, N)] if away else [])
        assert all(1 <= len(w[3]) <= MAX_VALUE_LEN for w in rd["writes"])
    # the sleepers are in some exchange of the return round
    back = {x for ph in scen["rounds"][AWAY]["phases"] for p in ph for x in p}
    assert set(range(SLEEPERS)) <= back


def test_oracle_cuts_deltas_of_large_nodedeltas_on_the_return(sleeper):
    _, _, per_round = sleeper
    assert all(d["truncated"] == 0 for d in per_round[:AWAY])
    d = per_round[AWAY]
    assert d["truncated"] > 0
    assert d["delta_bytes"] > (1 << 16) * d["exchanges"]


def test_sleeper_scenario_is_deterministic():
    a = sleeper_scenario(12, 300_000, 2, 5, 3)
    assert a == sleeper_scenario(12, 300_000, 2, 5, 3)
    assert a[1][5] == 1 << 16


def test_big_values_lengths_and_distinctness():
    spec = WorkloadSpec(n=24, k=16, fanout=2, seed=7, init="warm", write_frac=0.5, delete_frac=0.15, ttl_frac=0.1)
    base = make_scenario("bv", spec, 10, {})
    scen = big_values(make_scenario("bv", spec, 10, {}))
    assert scen == big_values(make_scenario("bv", spec, 10, {}))
    seen = set()
    for (j, k, v0), (_, _, v) in zip(base["initial"], scen["initial"]):
        assert len(v) in EDGES and (v.startswith(v0) or len(v) < len(v0))
        seen.add(len(v))
    last = {(j, k): v for j, k, v in scen["initial"]}
    for rd0, rd in zip(base["rounds"], scen["rounds"]):
        assert [w[:3] for w in rd0["writes"]] == [w[:3] for w in rd["writes"]]
        for (j, k, op, v0), (_, _, _, v) in zip(rd0["writes"], rd["writes"]):
            if op in (1, 3):
                assert v == v0 == ""
                continue
            assert len(v) in EDGES and (v.startswith(v0) or len(v) < len(v0))
            assert v != last[(j, k)]  # never a no-op of NodeState.set that the original was not
            last[(j, k)] = v
            seen.add(len(v))
    assert seen == set(EDGES)  # every edge length is written somewhere

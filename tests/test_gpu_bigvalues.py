"""The packers with values up to the 16,383-byte limit and NodeDeltas past 64 KiB, against the C oracle.  GPU only.

Every other test writes values of about ten bytes, so the size arithmetic of the device -- length varints of 2 and
3 bytes, 16-bit packed size fields, 32-bit running totals, slice totals, chain states -- never sees a value length
field of 128 or more, or a NodeDelta of 16,384 bytes or more.  The scenarios of tests/bigvalues.py do (their
properties are pinned on the CPU by tests/test_bigvalues_host.py); here each one runs in lockstep with the oracle
(64-bit sizes, itself checked against the reference at these sizes: scen_bigval6, scen_bigsleep12), compared after
every round, through

* k_pack_heavy (hand-off threshold lowered by GS_HEAVY_T, read once per process: a child process), both view widths;
* k_pack_slice alone (GS_HEAVY=0) and the default threshold (lite path + k_pack_slice);
* an mtu that puts the NodeDelta of exactly 65,536 bytes inside a heavy slot's whole-fit prefix;
* the sliced path (count, gather, overflow list, chain) over 2 and 4 slices, driven by shard.py and by the library;
* the tombstone layout (eval_cand, the key ranking of a cut NodeDelta, apply with holes);
* the value limit: 16,383 bytes are stored and gossiped, 16,384 are refused loudly.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

N, MTU, SLEEPERS, AWAY, AFTER = 128, 3_000_000, 4, 5, 3
DESIGNATED = 5
STATS = ("node_deltas", "kvs_sent", "truncated", "delta_bytes")


def prefix_mtu(sizes):
    """An mtu at which a returning node's first delta holds, whole, every owner up to the designated one (65,536
    bytes exactly) and stops inside the next: the sizes before it in column order, its own, and half the next."""
    assert sizes[DESIGNATED] == 1 << 16
    nxt = next(s for s in sizes[DESIGNATED + 1:] if s)
    return sum(sizes[:DESIGNATED]) + (1 << 16) + nxt // 2


def lockstep(scen, gpu, check_round=None):
    """Run ``scen`` on ``gpu`` (a GossipSim or ShardGroup) and the oracle, compare after every round and the send
    counters at the end; returns (the device's counters, the oracle)."""
    from helpers import compare_exports, make_backend
    from oracle import OracleSim

    from aiocluster_amd.scenario import replay_round

    orc = make_backend(OracleSim, scen)
    for r in range(len(scen["rounds"])):
        replay_round(gpu, scen, r)
        replay_round(orc, scen, r)
        ex = orc.export()
        d = compare_exports(gpu.export(), ex)
        assert d is None, f"round {r}: {d}"
        if check_round:
            check_round(r, ex)
    c, s = gpu.check(), orc.stats()
    for k in STATS:
        assert c[k] == s[k], (k, c[k], s[k])
    return c, orc


def run_sleeper(mtu=None, designated_whole=False, **kw):
    """The sleeper scenario on one handle in the prefix-view layout; ``mtu`` = "prefix": prefix_mtu of its sizes,
    and with ``designated_whole`` the oracle must have sent the designated owner's NodeDelta whole to some
    returning node in the return round (that node's max_version of the owner equals the owner's own)."""
    from bigvalues import sleeper_scenario
    from helpers import make_backend

    from aiocluster_amd.sim import GossipSim

    scen, sizes = sleeper_scenario(N, MTU, SLEEPERS, AWAY, AFTER)
    if mtu == "prefix":
        scen["config"]["mtu"] = prefix_mtu(sizes)
    whole = []

    def check_round(r, ex):
        if r == AWAY:
            mv = ex["mv"]
            assert mv[DESIGNATED, DESIGNATED] == 16 + AWAY
            whole.extend(s for s in range(SLEEPERS) if mv[s, DESIGNATED] == mv[DESIGNATED, DESIGNATED])

    gpu = make_backend(GossipSim, scen, tombstones=False, fd_ring=False, **kw)
    c, _ = lockstep(scen, gpu, check_round)
    if designated_whole:
        assert whole, "no returning node got the 65,536-byte NodeDelta in the return round"
    gpu.close()
    return c


CHILD = r"""
import sys
sys.path[:0] = [%(here)r, %(repo)r, %(oracle)r]
from test_gpu_bigvalues import run_sleeper
c = run_sleeper(**%(kw)r)
print("ok heavy_slots %%d truncated %%d" %% (c["heavy_slots"], c["truncated"]))
"""


def child(env_extra, **kw):
    code = CHILD % dict(here=HERE, repo=REPO, oracle=os.path.join(REPO, "oracle"), kw=kw)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env_extra), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("ok"), line
    return dict(zip(line.split()[1::2], (int(x) for x in line.split()[2::2])))


@pytest.mark.parametrize("v8", [True, False], ids=["hb8mv8", "hb16"])
def test_heavy_slots_with_nodedeltas_past_64k(v8):
    """GS_HEAVY_T=48: the returning nodes' slots (124 stale owners, most NodeDeltas of 65,536 bytes or more, the
    delta cut at 3,000,000) go through k_pack_heavy's whole-fit prefix and first-fit continuation."""
    st = child({"GS_HEAVY_T": "48"}, hb8=v8, mv8=v8)
    assert st["heavy_slots"] > 0 and st["truncated"] > 0, st


@pytest.mark.parametrize("v8", [True, False], ids=["hb8mv8", "hb16"])
def test_heavy_prefix_holds_the_nodedelta_of_exactly_64k(v8):
    """The same at an mtu that ends the whole-fit prefix of a returning node's slot right after the NodeDelta of
    exactly 65,536 bytes: it must be sent whole, as the oracle does."""
    st = child({"GS_HEAVY_T": "48"}, mtu="prefix", designated_whole=True, hb8=v8, mv8=v8)
    assert st["heavy_slots"] > 0 and st["truncated"] > 0, st


def test_pack_slice_alone_with_nodedeltas_past_64k():
    """GS_HEAVY=0: no hand-off, k_pack_slice walks the same slots."""
    st = child({"GS_HEAVY": "0"}, hb8=True, mv8=True)
    assert st["heavy_slots"] == 0 and st["truncated"] > 0, st


@pytest.mark.parametrize("v8", [True, False], ids=["hb8mv8", "hb16"])
def test_default_threshold_with_nodedeltas_past_64k(v8):
    """In-process, at the default hand-off threshold (no slot of 128 nodes reaches it): lite path + k_pack_slice."""
    c = run_sleeper(hb8=v8, mv8=v8)
    assert c["truncated"] > 0 and c["lite_slots"] > 0, c


@pytest.mark.parametrize("n,G,native", [(N, 2, False), (N, 2, True), (2 * N, 4, False), (2 * N, 4, True)],
                         ids=["G2-shard_py", "G2-library", "G4-shard_py", "G4-library"])
def test_slices_carry_sizes_past_64k_across_boundaries(n, G, native):
    """Owner-column slices: slice totals, the overflow list and the chain state carry the running size past 64 KiB
    from slice to slice; the NodeDelta of exactly 65,536 bytes is followed by a chain step.  (A slice is a multiple
    of 64 columns and none may be empty, so four slices need more than 192 nodes: 256 here.)"""
    from bigvalues import sleeper_scenario

    from aiocluster_amd import _lib
    from aiocluster_amd.scenario import initial_by_owner, scenario_node_ids
    from aiocluster_amd.shard import ShardGroup

    scen, sizes = sleeper_scenario(n, MTU, SLEEPERS, AWAY, AFTER)
    lo, ncol = _lib.slice_columns(n, G, 0)
    assert sizes[DESIGNATED] == 1 << 16 and sum(s >= 1 << 16 for s in sizes) * 2 >= n - SLEEPERS
    assert lo <= DESIGNATED < lo + ncol - 1 and G > 1  # not the last column of its slice, and slices follow it
    grp = ShardGroup.in_process(scenario_node_ids(scen), scen["keys"], scen["config"], G, native=native,
                                init=scen["init"], initial_values=initial_by_owner(scen), tombstones=False,
                                fd_ring=False)
    c, _ = lockstep(scen, grp)
    assert c["truncated"] > 0, c
    if not native:  # (the library's driver keeps no count of its chained phases)
        assert grp.chain_phases > 0
    for s in grp.slices:
        s.close()


def test_tombstone_layout_with_values_at_the_length_edges():
    """big_values over a workload with deletes and TTL writes: value lengths 1 .. 16,383 through eval_cand, the key
    ranking of a cut NodeDelta in pack_group, and apply with holes."""
    from bigvalues import big_values
    from helpers import make_backend

    from aiocluster_amd.scenario import make_scenario
    from aiocluster_amd.sim import GossipSim
    from aiocluster_amd.workload import WorkloadSpec

    spec = WorkloadSpec(n=96, k=16, fanout=3, seed=96, init="warm", write_frac=0.5, delete_frac=0.1, ttl_frac=0.05,
                        down_frac=0.1, down_rounds=3)
    scen = big_values(make_scenario("bigtomb96", spec, 8, {"mtu": 120_000}))
    gpu = make_backend(GossipSim, scen, tombstones=True)
    c, _ = lockstep(scen, gpu)
    assert c["truncated"] > 0, c
    gpu.close()


def test_value_limit_16383_is_stored_and_16384_is_refused():
    """gs_owner_writes takes value lengths below 2^14: a SET of 16,383 bytes is stored and gossiped; one of 16,384
    is refused and counted (err_hist_full, which check() raises on), and the state stays that of an oracle that
    never saw it."""
    from helpers import compare_exports, make_backend
    from oracle import OracleSim

    from aiocluster_amd._lib import GsError
    from aiocluster_amd.scenario import make_scenario, replay_round
    from aiocluster_amd.sim import GossipSim
    from aiocluster_amd.workload import WorkloadSpec, round_tick

    n = 8
    spec = WorkloadSpec(n=n, k=4, fanout=3, seed=8, init="warm", write_frac=0.0)
    scen = make_scenario("limit8", spec, 3, {})
    gpu = make_backend(GossipSim, scen)
    orc = make_backend(OracleSim, scen)
    ok, over = "a" * ((1 << 14) - 1), "b" * (1 << 14)
    for b in (gpu, orc):
        b.write(round_tick(0), 2, 1, 0, ok)
    for r in range(3):
        if r == 1:
            gpu.write(round_tick(1), 3, 1, 0, over)  # the oracle never sees it
        replay_round(gpu, scen, r)
        replay_round(orc, scen, r)
        d = compare_exports(gpu.export(), orc.export())
        assert d is None, f"round {r}: {d}"
        if r == 0:
            c = gpu.check()
            assert c["err_hist_full"] == 0
        else:
            with pytest.raises(GsError, match="err_hist_full"):
                gpu.check()
    ex = orc.export()
    assert np.all(ex["mv"][:, 2] == 5) and np.all(ex["mv"][:, 3] == 4)  # gossiped to all / never written
    for o in (0, 7):
        assert gpu.node_state(o, 2).key_values[scen["keys"][1]].value == ok
        assert gpu.node_state(o, 3).key_values[scen["keys"][1]].value == "v3.1.i"
    c = gpu.counters()
    assert c["err_hist_full"] == 1 and c["delta_bytes"] == orc.stats()["delta_bytes"] > (1 << 14)
    gpu.close()

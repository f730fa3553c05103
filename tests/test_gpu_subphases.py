"""Sub-phases and mid-round report replays in every layout (GPU only).

Several phases of a round may run at one tick (sub-phases), and a round may have more phases than one base of report
planes holds (GS_PLANES = 32): the host then replays the pending planes into the sampling windows mid-round and
starts a new base (plane_slot, Dev::v_round / vt / t_cap, the telescoped and the per-report replay of k_liveness,
DevDyn in the batched group driver).  The scenarios of tests/manyphases.py cut a workload's
matchings into rounds of ~15 / ~50 / ~120 phases and place them on the ticks by three maps -- sub-phases at the
budget's last tick, three phases at every tick, 41 phases at the round's first tick -- and every layout replays them
in lockstep with the C oracle: the whole export bit for bit after every round (windows, liveness, time of death
included), the counters, and a row of phi.  tests/test_manyphases_host.py shows on the oracle alone that each of
these scenarios has the rounds, truncation, window roll-overs and report spacings the comparison needs.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
from helpers import compare_exports, make_backend
from manyphases import (LAYOUTS, RING_ROWS, SLICED_KW, TICK_MAPS, Tap, device_scenario, rounds_past_a_base,
                        sliced_scenario, ticks_after_subphases)
from oracle import OracleSim
from test_gpu_parity import PHI_RTOL

from aiocluster_amd._lib import GS_CHAIN_CAP, GsError, overflow_list_len
from aiocluster_amd.scenario import initial_by_owner, replay_round, round_ticks, scenario_node_ids
from aiocluster_amd.shard import ShardGroup
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.workload import round_tick

pytestmark = pytest.mark.gpu

STAT_KEYS = ("exchanges", "hb_reports", "node_deltas", "kvs_sent", "truncated", "delta_bytes")
NON_FD = ("pos", "hb", "mv", "gc", "kv_version", "kv_status", "kv_value_id", "kv_ts")


def oracle_phi_row(orc, o, t):
    import ctypes

    out = np.full(orc.n, np.nan)
    phi = ctypes.c_double()
    for j in range(orc.n):
        if orc.L.orc_fd_phi(orc.h, o, j, t * 15625, ctypes.byref(phi)):
            out[j] = phi.value
    return out


def assert_phi_row(dev, orc, o, t):
    got, want = dev.phi_row(o, t), oracle_phi_row(orc, o, t)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"phi row {o}: None at different targets"
    m = ~np.isnan(want)
    assert m.sum() > 0
    np.testing.assert_allclose(got[m], want[m], rtol=PHI_RTOL, atol=0)


def assert_counters(c, orc):
    s = orc.stats()
    for k in STAT_KEYS:
        assert c[k] == s[k], (k, c[k], s[k])
    assert c["truncated"] > 0


def assert_flushes(c, scen, kind):
    """plane_flushes counts the mid-round replays of plane_slot: at least one per round with more phases than a
    base has planes, and with three phases per tick one at every tick that follows sub-phases."""
    assert c["plane_flushes"] > 0
    assert c["plane_flushes"] >= rounds_past_a_base(scen), (c["plane_flushes"], rounds_past_a_base(scen))
    if kind == "triples":
        assert c["plane_flushes"] >= ticks_after_subphases(scen), (c["plane_flushes"], ticks_after_subphases(scen))


@pytest.mark.parametrize("kind", list(TICK_MAPS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_one_handle_matches_oracle(layout, kind):
    scen = device_scenario(layout, kind)
    kw = dict(LAYOUTS[layout][2])
    sampled = layout == "sampled"
    if sampled:
        kw["ring_rows"] = RING_ROWS
    gpu = make_backend(GossipSim, scen, **kw)
    orc = make_backend(OracleSim, scen)
    ring = list(RING_ROWS)
    for r in range(len(scen["rounds"])):
        replay_round(gpu, scen, r)
        replay_round(orc, scen, r)
        got, want = gpu.export(), orc.export()
        if sampled:
            # the ring rows are exact, windows included; a compact row's full window is counted in fd_saturated and
            # inexact from then on (the sampled-ring contract), so the other rows are compared on everything else
            diff = compare_exports({k: v[ring] for k, v in got.items()}, {k: v[ring] for k, v in want.items()})
            diff = diff or compare_exports({k: (got[k] if k in NON_FD else v) for k, v in want.items()}, want)
        else:
            diff = compare_exports(got, want)
        assert diff is None, f"round {r}: device vs oracle: {diff}"
    c = gpu.check(accept_saturated=sampled)
    print(f"{layout}/{kind}: phases/round {[len(rd['phases']) for rd in scen['rounds']]}, plane flushes "
          f"{c['plane_flushes']} (rounds past a base {rounds_past_a_base(scen)}, ticks after sub-phases "
          f"{ticks_after_subphases(scen)}), truncated {c['truncated']}, hb_reports {c['hb_reports']}")
    if sampled:
        assert c["fd_saturated"] > 0 and c["err_fd_overflow"] == 0
    assert_counters(c, orc)
    assert_flushes(c, scen, kind)
    assert_phi_row(gpu, orc, RING_ROWS[2], gpu.last_tick)
    gpu.close()
    orc.close()


class Flushing:
    """A backend that passes everything on to ``sim`` and, after the phases with the given indices of each round,
    calls flush_reports at that phase's tick when the next phase comes at a later tick."""

    def __init__(self, sim, after):
        self.sim, self.after, self.flushes = sim, set(after), 0
        self.next_ticks = None  # the round's ticks (scenario.round_ticks), set by the caller before each round

    def write(self, *a):
        self.sim.write(*a)

    def begin_round(self, t, up):
        self.p = 0
        self.sim.begin_round(t, up)

    def run_phase(self, t, pairs):
        self.sim.run_phase(t, pairs)
        if self.p in self.after and self.next_ticks[self.p + 1] > t:
            self.sim.flush_reports(t)
            self.flushes += 1
        self.p += 1

    def liveness(self, t, up, r=-1):
        self.sim.liveness(t, up, r)


@pytest.mark.parametrize("layout", ["general", "hb8mv8"])
def test_flush_reports_between_phases_is_transparent(layout):
    """gs_flush_reports twice in a round on the device only, between phases at different ticks (once inside the
    first plane base, once after a mid-round replay): the oracle has no such step, and the state must be equal."""
    scen = device_scenario(layout, "budget")
    gpu = make_backend(GossipSim, scen, **LAYOUTS[layout][2])
    orc = make_backend(OracleSim, scen)
    fl = Flushing(gpu, after=(3, 40))
    for r in range(len(scen["rounds"])):
        fl.next_ticks = round_ticks(scen, r)
        replay_round(fl, scen, r)
        replay_round(orc, scen, r)
        diff = compare_exports(gpu.export(), orc.export())
        assert diff is None, f"round {r}: device vs oracle: {diff}"
    long_rounds = sum(len(rd["phases"]) > 41 for rd in scen["rounds"])
    assert fl.flushes >= len(scen["rounds"]) + long_rounds and long_rounds > 0
    assert_counters(gpu.check(), orc)
    assert_phi_row(gpu, orc, 5, gpu.last_tick)
    gpu.close()
    orc.close()


def test_ticks_out_of_order_are_refused():
    """Refusals, not faults: each raises GsError with the library's message, and the round goes on to the oracle's
    state."""
    import torch

    scen = device_scenario("hb8mv8", "budget", rounds=1)
    rd, t0 = scen["rounds"][0], round_tick(0)
    kw = LAYOUTS["hb8mv8"][2]
    gpu = make_backend(GossipSim, scen, **kw)
    orc = make_backend(OracleSim, scen)
    for b in (gpu, orc):
        for j, k, op, v in rd["writes"]:
            b.write(t0, j, k, op, v)
        b.begin_round(t0, rd["up"])
        b.run_phase(t0 + 3, rd["phases"][0])
    with pytest.raises(GsError, match="phase tick .* not after the round start / previous phase"):
        gpu.run_phase(t0 + 2, rd["phases"][1])  # a phase at a tick below the previous phase's
    with pytest.raises(GsError, match="gs_liveness at tick .* precedes a phase at tick"):
        gpu.liveness(t0 + 2, rd["up"])
    gpu.flush_reports(t0 + 5)
    with pytest.raises(GsError, match="phase tick .* not after the round start / previous phase"):
        gpu.run_phase(t0 + 5, rd["phases"][1])  # a phase at the tick of a flush_reports
    for b in (gpu, orc):
        b.run_phase(t0 + 6, rd["phases"][1])
        b.run_phase(t0 + 6, rd["phases"][2])  # a sub-phase
        b.liveness(t0 + 7, rd["up"], 0)
    diff = compare_exports(gpu.export(), orc.export())
    assert diff is None, diff
    gpu.check()
    gpu.close()
    # gs_phase_pack at a tick other than its gs_phase_count's (one slice driven through the sliced calls)
    one = make_backend(GossipSim, scen, sliced=True, **kw)
    for j, k, op, v in rd["writes"]:
        one.write(t0, j, k, op, v)
    one.begin_round(t0, rd["up"])
    arr = np.asarray(rd["phases"][0], dtype=np.int32)
    ini, res = one._pairs_dev(arr[:, 0], arr[:, 1])
    tot_all = one.phase_count(t0 + 3, ini, res).unsqueeze(0)
    chain = torch.empty((len(arr), 2), dtype=torch.int64, device=one.device)
    with pytest.raises(GsError, match="is not the tick of the last gs_phase_count"):
        one.phase_pack(t0 + 4, ini, res, 0, tot_all, None, chain)
    one.phase_pack(t0 + 3, ini, res, 0, tot_all, None, chain)  # the phase completes at its own tick
    one.phase_overflow(tot_all, chain, torch.empty(overflow_list_len(len(arr)), dtype=torch.int32, device=one.device),
                       torch.empty(max(2 * len(arr), GS_CHAIN_CAP) + 1, dtype=torch.int64, device=one.device),
                       read=False)  # as run_sliced_phase ends a phase of one slice
    one.liveness(t0 + 4, rd["up"])
    one.check()
    one.close()
    orc.close()


def sliced_run(row, kind, n, G):
    """G in-process slices vs one handle vs the oracle, every round; returns (the group's counters, the phases
    that chained and were sub-phases, all that chained, plane flushes per slice).  A phase in which the oracle cut a
    delta is one whose slot totals pass the mtu: the slices settle it in chain steps (shard.py step 4); where the
    driver is shard.py's own, its recorded pack steps must say the same."""
    scen = sliced_scenario(row, kind, n)
    kw = SLICED_KW[row]
    one = make_backend(GossipSim, scen, **kw)
    grp = ShardGroup.in_process(scenario_node_ids(scen), scen["keys"], scen["config"], G, init=scen["init"],
                                initial_values=initial_by_owner(scen), native=row != "py", **kw)
    orc = make_backend(OracleSim, scen)
    tap = Tap(orc)
    for r in range(len(scen["rounds"])):
        replay_round(one, scen, r)
        replay_round(grp, scen, r)
        replay_round(tap, scen, r)
        got, want = grp.export(), orc.export()
        diff = compare_exports(got, one.export())
        assert diff is None, f"round {r}: slices vs one handle: {diff}"
        diff = compare_exports(got, want)
        assert diff is None, f"round {r}: slices vs oracle: {diff}"
    c1, cg = one.check(), grp.check()
    for k in STAT_KEYS + ("hb_writes",):
        assert cg[k] == c1[k], (k, cg[k], c1[k])
    assert_counters(cg, orc)
    flushes = [s.counters()["plane_flushes"] for s in grp.slices]
    assert len(set(flushes)) == 1 and flushes[0] == c1["plane_flushes"], (flushes, c1["plane_flushes"])
    assert_flushes(c1, scen, kind)
    o = n // 3
    assert np.array_equal(grp.phi_row(o), one.phi_row(o), equal_nan=True)
    assert_phi_row(grp, orc, o, one.last_tick)
    chained = [i for i, cut in enumerate(tap.cut) if cut]
    chained_sub = [i for i in chained if tap.sub[i]]
    if row == "py":
        assert len(grp.phase_steps) == len(tap.cut)
        stepped = [i for i, s in enumerate(grp.phase_steps) if s > 1]
        assert grp.chain_phases == len(stepped) > 0
        assert set(chained) <= set(stepped), "a phase with a cut delta took no chain step"
        chained, chained_sub = stepped, [i for i in stepped if tap.sub[i]]
    one.close()
    for s in grp.slices:
        s.close()
    orc.close()
    return cg, chained_sub, chained, flushes[0]


@pytest.mark.parametrize("n,G", [(128, 2), (256, 4)])
@pytest.mark.parametrize("kind", ["budget", "triples"])
@pytest.mark.parametrize("row", list(SLICED_KW))
def test_slices_match_single_handle_and_oracle(row, kind, n, G):
    """Sub-phases on sliced handles with a binding mtu, so that chain steps run inside sub-phases: shard.py's driver
    (gs_phase_count / gs_phase_pack), gs_run_phase_group per slice (tombstones) and its batched path (8-bit views)."""
    cg, chained_sub, chained, flushes = sliced_run(row, kind, n, G)
    print(f"{row}/{kind}/{n}x{G}: {len(chained)} chained phases, {len(chained_sub)} of them sub-phases "
          f"(first {chained_sub[:5]}), plane flushes {flushes}, truncated {cg['truncated']}")
    assert chained and chained_sub, (chained[:10], chained_sub[:10])


def test_batched_group_driver_with_lite_in_pass1_runs_sub_phases():
    """The batched path with env GS_GRP_P1LITE=1 (read once per process, so a child process runs it)."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "from test_gpu_subphases import sliced_run\n"
            "cg, sub, chained, fl = sliced_run('batched', 'budget', 256, 4)\n"
            "assert chained and sub and fl > 0, (chained, sub, fl)\n"
            "print('ok', len(chained), len(sub), fl)\n") % (here, os.path.dirname(here),
                                                           os.path.join(os.path.dirname(here), "oracle"))
    env = dict(os.environ, GS_GRP_P1LITE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout

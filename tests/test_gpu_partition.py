"""Network partitions on the device (gs_draw_cuts_zoned, gs_filter_targets_zoned, gs_detect_census_for; GPU only).

1. the device draw equals ``cuts.draw_cuts_zoned`` across the wave and workgroup widths, 255s included;
2. the target filter equals its mirror on gs_select_peers' output, aliased or not, and the phases scheduled from the
   filtered targets hold no pair whose connect would fail;
3. lockstep with the oracle composer of tests/lossycases.py through a split and a heal, whole state after every round;
4. a down pair that was not removed is loud: both rows unchanged, err_bad_index counted;
5. gs_detect_census_for with observers == up is gs_detect_census, field for field;
6. observers != up equals the numpy reference of tests/partitionref.py over readback, on one handle and on three slices;
7. a split-and-heal curve at small size: the zoned census after every round against the reference over the ORACLE's
   state of that round, the zone x zone views-behind matrix against numpy over readback;
8. refusals.
"""

import ctypes as C

import numpy as np
import pytest
import torch
from detectref import assert_census
from helpers import compare_exports, make_backend
from lossycases import CUT_SEED, CutOracleSim, warm_lossy
from partitionref import (cross_dead, detect_reference_for, partition_scenario, views_behind_reference,
                          zoned_reference)
from test_gpu_detect_census import FD_CFG, PRIOR5, SWEEP, dev_u8, fd_readback

from aiocluster_amd import _lib, driver
from aiocluster_amd._lib import GsError
from aiocluster_amd.cuts import LINK_DOWN, draw_cuts_zoned, filter_targets_zoned, loss_q32
from aiocluster_amd.detect import DownClock
from aiocluster_amd.peers import PeerSelector
from aiocluster_amd.scenario import DEFAULT_CFG, make_scenario, replay_round, round_tick, round_ticks
from aiocluster_amd.shard import ShardGroup
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.topology import LinkClock, Topology, views_behind
from aiocluster_amd.workload import WorkloadSpec, key_names, synthetic_node_ids

pytestmark = pytest.mark.gpu

PREFIX = dict(tombstones=False, fd_ring=False)
LAYOUTS = {"prefix": dict(PREFIX), "hb8mv8_esc4": dict(PREFIX, hb8=True, mv8=True, esc_cols=4)}
N = 1100
BOUNDS = [0, 500, 1036, 1100]  # zone boundaries off the 64-column and the 16-column grids
SEED = 0xDEADBEEF_0BADF00D


def make_warm(n=N, K=4, cfg=None, **over):
    kw = dict(init="warm", tombstones=False, fd_ring=False, hist_cap=16, initial_ops=driver.boot_ops(n, K), hb8=True,
              mv8=True)
    kw.update(over)
    return GossipSim(synthetic_node_ids(n), key_names(K), dict(DEFAULT_CFG, **(cfg or FD_CFG)), **kw)


@pytest.fixture(scope="module")
def sim1100():
    sim = make_warm()
    yield sim
    sim.close()


# ---------------------------------------------------------------- 1. the device draw
def link_matrix(Z, rng):
    """Down, lossy, zero and asymmetric entries (for Z = 1 the one entry is lossy)."""
    choices = np.array([0, loss_q32(0.3), loss_q32(0.9), LINK_DOWN, 0xFFFFFFFE, 1], dtype=np.uint32)
    link = choices[rng.integers(0, len(choices), (Z, Z))]
    link[0, 0] = loss_q32(0.5)
    if Z > 1:
        link[0, 1], link[1, 0] = loss_q32(0.3), 0  # asymmetric
        link[Z - 1, 0] = LINK_DOWN  # down one way
        assert (link != link.T).any()
    return link


@pytest.mark.parametrize("Z", [1, 3, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 550])
def test_device_draw_equals_the_mirror(sim1100, n, Z):
    sim = sim1100
    rng = np.random.default_rng(1000 * Z + n)
    link = link_matrix(Z, rng)
    zone = rng.integers(0, Z, N).astype(np.uint8)
    ini = rng.integers(0, N, n).astype(np.int32)
    res = rng.integers(0, N, n).astype(np.int32)
    got = sim.draw_cuts_zoned(ini, res, SEED, 7, 3, zone, link).cpu().numpy()
    want = draw_cuts_zoned(ini, res, SEED, 7, 3, zone, link)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (n, Z, np.flatnonzero(got != want)[:8])
    if n >= 255:
        assert set(want.tolist()) >= ({0, 1, 2, 3, 255} if Z > 1 else {0, 1, 2, 3})
    # a zone byte >= Z and an index >= N give 255; their neighbours in the same wave are drawn as usual
    zone[5] = Z
    ini2 = np.array([5, 6, N, 7, -1, 8, 9], dtype=np.int32)
    res2 = np.array([6, 5, 8, N + 70000, 9, 10, 5], dtype=np.int32)
    got2 = sim.draw_cuts_zoned(ini2, res2, SEED, 7, 3, zone, link).cpu().numpy()
    assert np.array_equal(got2, draw_cuts_zoned(ini2, res2, SEED, 7, 3, zone, link))
    assert got2[[0, 1, 2, 3, 4, 6]].tolist() == [255] * 6
    # every entry one threshold: gs_draw_cuts, byte for byte
    q = loss_q32(0.25)
    uni = sim.draw_cuts_zoned(ini, res, SEED, 7, 3, rng.integers(0, Z, N).astype(np.uint8), np.full((Z, Z), q, np.uint32))
    assert torch.equal(uni, sim.draw_cuts(ini, res, SEED, 7, 3, q))


# ---------------------------------------------------------------- 2. the target filter
def test_target_filter_equals_its_mirror_and_schedules_only_attempted_exchanges(sim1100):
    sim = sim1100
    topo = Topology.blocks(BOUNDS)
    topo.cut(0, 2, both=False)  # one link down, one way: both directions between zones 0 and 2 fail
    up_h = np.ones(N, np.uint8)
    up_h[[3, 600, 1050]] = 0
    up = dev_u8(sim, up_h)
    sel = PeerSelector(sim, fanout=3, seed=4)
    sel.select(up, 0)
    before = sel.targets.clone()
    want, cnt = filter_targets_zoned(before.cpu().numpy(), topo.zone, topo.link)
    assert cnt > 0
    dropped = torch.zeros(1, dtype=torch.int32, device=sim.device)
    out = torch.full_like(before, -7)
    sim.filter_targets(sel.targets, topo, out=out, dropped=dropped)
    assert np.array_equal(out.cpu().numpy(), want) and torch.equal(sel.targets, before)
    assert int(dropped.item()) == cnt
    sim.filter_targets(sel.targets, topo.zone, topo.link, dropped=dropped)  # aliased; the count is added to
    assert np.array_equal(sel.targets.cpu().numpy(), want) and int(dropped.item()) == 2 * cnt
    phases, offs, left = sel.schedule(up, 0)
    assert left == 0 and offs[-1] > 0
    valid = (want >= 0) & (up_h[np.where(want >= 0, want, 0)] != 0) & (up_h[:, None] != 0)
    assert offs[-1] == int(valid.sum())  # every attempted exchange is scheduled, and nothing else
    for a, b, _ in phases:
        assert topo.connect_ok(a.cpu().numpy(), b.cpu().numpy()).all()


# ---------------------------------------------------------------- 3. lockstep through a split and a heal
SPLIT_EVENTS = [(2, "split", [[2]]), (2, "set_link", (0, 1, 0.3, False)),
                (5, "heal_all", ()), (5, "set_link", (0, 1, 0.0, False))]


@pytest.fixture(scope="module")
def split1100():
    """lossycases.warm_lossy's scenario (N = 1,100, K = 4, mtu 1,500), 6 rounds: rounds 0-1 whole, rounds 2-4 with
    zone 2 split off hard and link[0][1] at 30 % one way, round 5 healed.  The composer runs the mirror's pairs and
    legs; the preconditions are asserted on its side."""
    scen = partition_scenario(warm_lossy(rounds=6), Topology.blocks(BOUNDS), SPLIT_EVENTS, CUT_SEED)
    counts = [0, 0, 0, 0]
    for rd in scen["rounds"][2:5]:
        assert rd["topo"].components() == [[0, 1], [2]] and rd["topo"].link[0, 1] == loss_q32(0.3)
        assert rd["topo"].link[1, 0] == 0
        for lg in rd["legs"]:
            for x in lg:
                counts[x] += 1
    assert all(c > 0 for c in counts), counts
    assert sum(rd["no_connect"] for rd in scen["rounds"][2:5]) >= 1
    for r in (0, 1, 5):
        rd = scen["rounds"][r]
        assert rd["no_connect"] == 0 and all(x == 3 for lg in rd["legs"] for x in lg) and not rd["topo"].link.any()
    orc = make_backend(CutOracleSim, scen)
    want = []
    for r in range(len(scen["rounds"])):
        replay_round(orc, scen, r)
        want.append(orc.export())
    assert orc.cut_exchanges == sum(counts[:3])
    orc.close()
    return scen, want


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_lockstep_through_a_split_and_a_heal(split1100, layout):
    """The device draws the legs of every pair of the unpartitioned schedule, removes the pairs the draw marks
    (a device compaction of the 255s) and runs the rest."""
    scen, want = split1100
    gpu = make_backend(GossipSim, scen, **LAYOUTS[layout])
    zone = dev_u8(gpu, scen["rounds"][0]["topo"].zone)
    removed = 0
    for r, rd in enumerate(scen["rounds"]):
        t = round_tick(r)
        ticks = round_ticks(scen, r)
        for j, k, op, v in rd["writes"]:
            gpu.write(t, j, k, op, v)
        gpu.begin_round(t, rd["up"])
        for p, ph in enumerate(rd["all_phases"]):
            arr = np.asarray(ph, dtype=np.int32).reshape(-1, 2)
            ini, res = gpu._pairs_dev(arr[:, 0], arr[:, 1])
            legs = gpu.draw_cuts_zoned(ini, res, CUT_SEED, r, p, zone, rd["topo"].link)
            keep = legs != 255
            removed += int((~keep).sum())
            kept_legs = legs[keep]
            assert kept_legs.cpu().numpy().tolist() == rd["legs"][p], (r, p)
            gpu.run_phase_arrays(ticks[p], ini[keep], res[keep], kept_legs)
        gpu.liveness(ticks[-1], rd["up"], r)
        diff = compare_exports(gpu.export(), want[r])
        assert diff is None, f"round {r}: device vs composer: {diff}"
    c = gpu.check()  # err_bad_index == 0 among them
    assert c["err_bad_index"] == 0
    assert removed == sum(rd["no_connect"] for rd in scen["rounds"]) >= 1
    assert c["exchanges"] == sum(len(ph) for rd in scen["rounds"] for ph in rd["phases"])
    assert c["cut_exchanges"] == sum(x < 3 for rd in scen["rounds"] for lg in rd["legs"] for x in lg) > 0
    gpu.close()


# ---------------------------------------------------------------- 4. an unfiltered down pair is loud
def test_unfiltered_down_pair_is_a_bad_index():
    spec = WorkloadSpec(n=64, k=4, fanout=2, seed=3, init="warm", write_frac=0.5)
    scen = make_scenario("down64", spec, 2, {})
    gpu, ctl = make_backend(GossipSim, scen, **PREFIX), make_backend(GossipSim, scen, **PREFIX)
    replay_round(gpu, scen, 0)
    replay_round(ctl, scen, 0)
    rd = scen["rounds"][1]
    t = round_tick(1)
    pairs = rd["phases"][0]
    x, y = pairs[1]
    zone = np.zeros(64, np.uint8)
    zone[y] = 1
    topo = Topology(zone, 2)
    topo.cut(0, 1)
    for g in (gpu, ctl):
        for j, k, op, v in rd["writes"]:
            g.write(t, j, k, op, v)
        g.begin_round(t, rd["up"])
    arr = np.asarray(pairs, dtype=np.int32)
    legs = gpu.draw_cuts_zoned(arr[:, 0], arr[:, 1], CUT_SEED, 1, 0, topo)
    down = legs.cpu().numpy() == 255
    assert down[1] and np.array_equal(down, ~topo.connect_ok(arr[:, 0], arr[:, 1]))
    gpu.run_phase(t + 1, pairs, legs)  # not filtered
    ctl.run_phase(t + 1, [p for p, d in zip(pairs, down) if not d])
    assert gpu.counters()["err_bad_index"] == int(down.sum())
    assert gpu.counters()["exchanges"] == ctl.counters()["exchanges"]
    eg, ec = gpu.export(), ctl.export()
    for name in eg:
        assert np.array_equal(eg[name], ec[name]), name
    for name in ("HB", "MV", "FD", "FD_LAST", "ROW"):  # both rows of the down pair are unchanged
        got = np.frombuffer(gpu.read_rows(name, 0, gpu.n), np.uint8).reshape(gpu.n, -1)
        ref = np.frombuffer(ctl.read_rows(name, 0, ctl.n), np.uint8).reshape(ctl.n, -1)
        assert np.array_equal(got[[x, y]], ref[[x, y]]), name
    with pytest.raises(GsError, match="err_bad_index"):
        gpu.check()
    ctl.check()
    gpu.close()
    ctl.close()


# ---------------------------------------------------------------- 5 / 6. gs_detect_census_for
@pytest.fixture(scope="module")
def churn1100():
    """1,100 nodes (a 256-row band boundary, a partial last 16-column group), churn for 4 rounds, on one handle and
    on three in-process slices; zone 2 is split off at round 2."""
    n, K = N, 4
    cfg = dict(DEFAULT_CFG, **FD_CFG)
    kw = dict(init="warm", tombstones=False, fd_ring=False, hist_cap=16, initial_ops=driver.boot_ops(n, K), hb8=True,
              mv8=True)
    ids, keys = synthetic_node_ids(n), key_names(K)
    one = GossipSim(ids, keys, cfg, **kw)
    grp = ShardGroup.in_process(ids, keys, cfg, shards=3, **kw)
    topo = Topology.blocks(BOUNDS)
    spec = WorkloadSpec(n=n, k=K, fanout=3, seed=21, init="warm", write_frac=0.1, down_frac=0.15, down_rounds=3,
                        topology=topo, link_events=[(2, "split", [[2]])])
    plans = driver.prepare(spec, 4, torch, one.device)
    down, links = DownClock(n), LinkClock(3)
    for rd in plans:
        assert "legs" not in rd  # whole and down links only: plain phases, which slices run too
        driver.run_round([one], rd)
        driver.run_round(grp.slices, rd, group=grp)
        down.update(rd["up_host"], rd["t"])
        links.update(rd["topo"], rd["t"])
    assert sum(rd["no_connect"] for rd in plans) > 0
    yield one, grp, plans[-1], down, links
    one.close()
    for s in grp.slices:
        s.close()


def test_census_for_with_observers_equal_to_up_is_the_census(churn1100):
    one, _, rd, down, _ = churn1100
    tick, up = rd["t_live"], rd["up"]
    for thr in (SWEEP, ()):
        a = one.detect_census(up, tick, down.down_since, thr, per_target=True, per_row=True)
        b = one.detect_census(up, tick, down.down_since, thr, per_target=True, per_row=True, observers=up.clone())
        assert set(a) == set(b)
        for k in a:
            if hasattr(a[k], "cpu"):
                assert torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], (k, a[k], b[k])
    sw = one.detect_census(up, tick, down.down_since, SWEEP, observers=up)
    for k in ("up_dead", "down_dead", "down_live", "max_detect_latency", "up_phi"):
        assert sw[k] > 0, k


def test_census_for_equals_the_reference_over_readback(churn1100):
    one, grp, rd, down, links = churn1100
    topo, up_h, tick = rd["topo"], rd["up_host"].astype(bool), rd["t_live"]
    assert topo.components() == [[0, 1], [2]]
    comp = topo.node_components()
    reach, since = topo.reachable(up_h), links.unreachable_since(topo, up_h, down)
    ex = fd_readback(one)
    seen = dict.fromkeys(("down_dead", "down_live", "up_dead", "max_detect_latency", "early_deaths"), 0)
    for c in range(2):
        obs = up_h & (comp == c)
        assert 0 < obs.sum() < up_h.sum() and (reach[c] != up_h).any()
        for thr in (SWEEP, ()):
            got = one.detect_census(reach[c].astype(np.uint8), tick, since[c], thr, per_target=True, per_row=True,
                                    observers=obs.astype(np.uint8))
            assert_census(got, detect_reference_for(ex, obs, reach[c], since[c], tick, thr, PRIOR5), (c, thr))
            sl = grp.detect_census(dev_u8(one, reach[c]), tick, since[c], thr, per_target=True, per_row=True,
                                   observers=dev_u8(one, obs))
            for k in got:
                if hasattr(got[k], "cpu"):
                    assert torch.equal(got[k], sl[k]), (c, k)
                else:
                    assert got[k] == sl[k], (c, k, got[k], sl[k])
        for k in seen:
            seen[k] += got[k]
        rows = got["row_undetected"].cpu().numpy()
        assert not rows[~obs].any()  # rows that are not counted stay 0
    assert all(seen.values()), seen
    # observers that are themselves down targets (all rows counted): their own pair is in neither count
    every = np.ones(N, np.uint8)
    got = one.detect_census(up_h.astype(np.uint8), tick, down.down_since, SWEEP, per_target=True, per_row=True,
                            observers=every)
    assert_census(got, detect_reference_for(ex, every, up_h, down.down_since, tick, SWEEP, PRIOR5), "all rows")
    assert got["down_pairs"] == int((~up_h).sum()) * (N - 1) > 0
    # the composition, and its reference stated per pair
    z = one.detect_census_zoned(up_h, topo, down, links, SWEEP, tick, per_target=True, per_row=True)
    assert_census(z, zoned_reference(ex, up_h, topo, down, links, tick, SWEEP, PRIOR5), "zoned")
    assert z["observers"] == int(up_h.sum())


# ---------------------------------------------------------------- 7. a split-and-heal curve
# Chosen on the CPU with the oracle (96 nodes in zones of 40 / 41 / 15, FD_CFG, workload seed 5, 5 % of the nodes down
# for 3 rounds each until the quiet rounds from 7 on; zone 2 split off in rounds 3-5): the ORACLE's states hold 207,
# 730 and 1,348 cross-component pairs dead after rounds 3, 4 and 5, and none after round 11.  Asserted below.
CURVE = dict(n=96, bounds=[0, 40, 81, 96], split_at=3, heal_at=6, rounds=12, quiet_from=7)


@pytest.fixture(scope="module")
def curve96():
    cv = CURVE
    spec = WorkloadSpec(n=cv["n"], k=4, fanout=3, seed=5, init="warm", write_frac=0.2, down_frac=0.05, down_rounds=3,
                        quiet_from=cv["quiet_from"])
    topo = Topology.blocks(cv["bounds"])
    events = [(cv["split_at"], "split", [[2]]), (cv["heal_at"], "heal_all", ())]
    scen = partition_scenario(make_scenario("curve96", spec, cv["rounds"], FD_CFG), topo, events, CUT_SEED)
    orc = make_backend(CutOracleSim, scen)
    exports = []
    for r in range(cv["rounds"]):
        replay_round(orc, scen, r)
        exports.append(orc.export())
    orc.close()
    dead = [cross_dead(ex, rd["up"], topo.zone, [0, 0, 1]) for ex, rd in zip(exports, scen["rounds"])]
    assert min(dead[cv["split_at"]:cv["heal_at"]]) >= 1 and dead[-1] == 0, dead
    return scen, exports, dead


def test_split_and_heal_curve(curve96):
    scen, exports, dead = curve96
    n = scen["n"]
    # the general layout: FD_CFG's dead_grace_s lets the detector forget nodes dead for 8 rounds (garbage_collect)
    gpu = make_backend(GossipSim, scen, canonical=False)
    down, links = DownClock(n), LinkClock(3)
    nonzero = dict.fromkeys(("down_dead", "down_live", "up_dead", "max_detect_latency"), 0)
    behind_seen = False
    for r, rd in enumerate(scen["rounds"]):
        replay_round(gpu, scen, r)
        topo, up = rd["topo"], np.asarray(rd["up"]).astype(bool)
        down.update(up, round_tick(r))
        links.update(topo, round_tick(r))
        tick = round_ticks(scen, r)[-1]
        ex = gpu.export()
        diff = compare_exports(ex, exports[r])
        assert diff is None, f"round {r}: device vs oracle: {diff}"
        for thr in ((), (1.0, 2.0, 4.0)):
            got = gpu.detect_census_zoned(up, topo, down, links, thr, tick, per_target=True, per_row=True)
            want = zoned_reference(exports[r], up, topo, down, links, tick, thr, PRIOR5)
            assert_census(got, want, (r, thr))
        for k in nonzero:
            nonzero[k] += got[k]
        split = CURVE["split_at"] <= r < CURVE["heal_at"]
        if split:  # every cross-component pair is a down pair of the zoned truth
            assert got["down_dead"] >= dead[r] >= 1
        m = views_behind(gpu, up, topo)
        assert np.array_equal(m, views_behind_reference(ex, up, topo.zone, 3)), r
        behind_seen |= bool(split and (m[2, :2].sum() > 0 or m[:2, 2].sum() > 0))
    assert all(nonzero.values()), nonzero
    assert behind_seen
    # healed, every node up: no target is unreachable, and nobody holds a node of the other side dead (dead[-1] == 0)
    assert got["down_pairs"] == 0 and got["observers"] == n
    assert cross_dead(ex, up, topo.zone, [0, 0, 1]) == 0
    gpu.check()
    gpu.close()


# ---------------------------------------------------------------- 8. refusals
def test_refusals(sim1100):
    sim = sim1100
    L, h = sim.L, sim.h
    zone = dev_u8(sim, np.zeros(N, np.uint8))
    ini = torch.zeros(4, dtype=torch.int32, device=sim.device)
    legs = torch.full((4,), 9, dtype=torch.uint8, device=sim.device)
    tg = torch.zeros((N, 5), dtype=torch.int32, device=sim.device)
    link = (C.c_uint32 * 289)()
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def refused(rc, fn):
        assert rc == _lib.GS_E_INVALID, (fn, rc)
        assert fn + ":" in L.gs_last_error(h).decode(), L.gs_last_error(h)

    for Z in (0, 17):
        refused(L.gs_draw_cuts_zoned(h, P(ini), P(ini), 4, 1, 0, 0, P(zone), link, Z, P(legs)), "gs_draw_cuts_zoned")
        refused(L.gs_filter_targets_zoned(h, P(tg), P(tg), N * 5, P(zone), link, Z, None), "gs_filter_targets_zoned")
        with pytest.raises(GsError, match="GS_E_INVALID.*gs_draw_cuts_zoned"):
            sim.draw_cuts_zoned(ini, ini, 1, 0, 0, zone, np.zeros((Z, Z), np.uint32))
    for miss in range(5):
        a = [P(ini), P(ini), P(zone), link, P(legs)]
        a[miss] = None
        refused(L.gs_draw_cuts_zoned(h, a[0], a[1], 4, 1, 0, 0, a[2], a[3], 3, a[4]), "gs_draw_cuts_zoned")
    for miss in range(4):
        a = [P(tg), P(tg), P(zone), link]
        a[miss] = None
        refused(L.gs_filter_targets_zoned(h, a[0], a[1], N * 5, a[2], a[3], 3, None), "gs_filter_targets_zoned")
    refused(L.gs_filter_targets_zoned(h, P(tg), P(tg), N * 5 - 1, P(zone), link, 3, None), "gs_filter_targets_zoned")
    sim.sync()
    assert (legs == 9).all() and not tg.any()  # refused before any device work
    tot = _lib.GsDetectTotals()
    up = dev_u8(sim, np.ones(N, np.uint8))
    for obs, u, out in ((None, P(up), C.byref(tot)), (P(up), None, C.byref(tot)), (P(up), P(up), None)):
        refused(L.gs_detect_census_for(h, obs, u, None, sim.last_tick, None, 0, None, None, out), "gs_detect_census_for")
    assert L.gs_draw_cuts_zoned(None, P(ini), P(ini), 4, 1, 0, 0, P(zone), link, 3, P(legs)) == _lib.GS_E_INVALID
    assert L.gs_api_version() == 23


def test_sliced_handle_refuses_zoned_draw_and_filter():
    spec = WorkloadSpec(n=128, k=4, fanout=2, seed=3, init="warm", write_frac=0.2)
    scen = make_scenario("sl128", spec, 1, {})
    gpu = make_backend(GossipSim, scen, sliced=True, **PREFIX)
    topo = Topology.blocks([0, 64, 128])
    ini = torch.zeros(4, dtype=torch.int32, device=gpu.device)
    with pytest.raises(GsError, match="GS_E_UNSUPPORTED.*gs_draw_cuts_zoned"):
        gpu.draw_cuts_zoned(ini, ini, 1, 0, 0, topo)
    with pytest.raises(GsError, match="GS_E_UNSUPPORTED.*gs_filter_targets_zoned"):
        gpu.filter_targets(torch.zeros((128, 4), dtype=torch.int32, device=gpu.device), topo)
    gpu.close()

"""Network partitions on the host: the zoned draw's definition, the connect rule, components, the link clock and
``driver.prepare`` under link events (CPU; no device call is made)."""

import numpy as np
import pytest
from partitionref import detect_reference_for, pairwise_reference, partition_scenario, zoned_reference

from aiocluster_amd.cuts import (LEGS_NO_CONNECT, LINK_DOWN, connect_ok, draw_cuts_q32, draw_cuts_zoned,
                                 filter_targets_zoned, loss_q32)
from aiocluster_amd.detect import DownClock
from aiocluster_amd.topology import LOSS_MAX_Q32, LinkClock, Topology
from aiocluster_amd.workload import Workload, WorkloadSpec

SEED = 0xDEADBEEF_0BADF00D


def random_pairs(n_nodes, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_nodes, n), rng.integers(0, n_nodes, n)


# ---------------------------------------------------------------- the draw
@pytest.mark.parametrize("q", [0, loss_q32(0.2), 0xFFFFFFFE])
def test_uniform_matrix_is_the_uniform_draw(q):
    n = 1100
    ini, res = random_pairs(n, 5000, 1)
    zone = np.random.default_rng(2).integers(0, 3, n)
    link = np.full((3, 3), q, dtype=np.uint32)
    got = draw_cuts_zoned(ini, res, SEED, 7, 3, zone, link)
    assert got.dtype == np.uint8 and np.array_equal(got, draw_cuts_q32(ini, res, SEED, 7, 3, q))
    if q == 0:
        assert (got == 3).all()
    elif q == 0xFFFFFFFE:
        assert (got == 0).sum() >= 4999  # a word of 2^32 - 2 or more: 2 in 2^32


def test_asymmetric_link_cuts_only_the_messages_of_its_direction():
    """link[0][1] lossy, link[1][0] = 0.  A 0 -> 1 exchange sends its Syn and its Ack over the lossy link (words 0
    and 2) and its SynAck over the clean one: legs is never 1.  A 1 -> 0 exchange sends only its SynAck over the
    lossy link (word 1): legs is 1 or 3."""
    n = 400
    zone = (np.arange(n) >= 200).astype(np.uint8)
    link = np.zeros((2, 2), dtype=np.uint32)
    link[0, 1] = loss_q32(0.4)
    ini, res = random_pairs(n, 5000, 3)
    legs = draw_cuts_zoned(ini, res, SEED, 1, 0, zone, link)
    z_i, z_r = zone[ini], zone[res]
    fwd, bwd, same = legs[(z_i == 0) & (z_r == 1)], legs[(z_i == 1) & (z_r == 0)], legs[z_i == z_r]
    assert set(fwd.tolist()) == {0, 2, 3}
    assert set(bwd.tolist()) == {1, 3}
    assert (same == 3).all()
    # and word by word: the same Philox words as the uniform draw, with the threshold of the direction
    q = int(link[0, 1])
    uni = draw_cuts_q32(ini, res, SEED, 1, 0, q)
    m = (z_i == 0) & (z_r == 1)
    assert np.array_equal(legs[m] == 0, uni[m] == 0)  # word 0 alone decides legs 0 in both


def test_link_down_one_way_removes_both_directions():
    n = 300
    zone = (np.arange(n) // 100).astype(np.uint8)
    topo = Topology(zone, 3)
    topo.set_link(0, 1, loss=0.3, both=False)
    topo.cut(0, 2, both=False)  # 0 -> 2 down, 2 -> 0 still up
    assert topo.link[0, 2] == LINK_DOWN and topo.link[2, 0] == 0
    ini, res = random_pairs(n, 5000, 4)
    ok = topo.connect_ok(ini, res)
    z_i, z_r = zone[ini], zone[res]
    between = ((z_i == 0) & (z_r == 2)) | ((z_i == 2) & (z_r == 0))
    assert np.array_equal(ok, ~between) and between.any()
    assert ((z_i == 2) & (z_r == 0) & ~ok).any()  # the direction whose own link is up
    legs = draw_cuts_zoned(ini, res, SEED, 0, 0, zone, topo.link)
    assert np.array_equal(legs == LEGS_NO_CONNECT, ~ok)
    assert legs[ok].max() <= 3
    # out of range: an index or a zone byte
    assert draw_cuts_zoned([0, n, -1, 5], [1, 2, 3, n + 7], SEED, 0, 0, zone, topo.link).tolist()[1:] == [255] * 3
    bad = zone.copy()
    bad[7] = 3
    assert draw_cuts_zoned([7, 8], [8, 7], SEED, 0, 0, bad, topo.link).tolist() == [255, 255]
    assert not connect_ok([7], [8], bad, topo.link)[0]


def test_loss_one_still_connects():
    topo = Topology(np.zeros(4, np.uint8), 1)
    topo.set_link(0, 0, loss=1.0)
    assert topo.link[0, 0] == LOSS_MAX_Q32 != LINK_DOWN
    assert topo.connect_ok([0], [1])[0]


def test_filter_targets_mirror():
    n = 60
    zone = (np.arange(n) // 20).astype(np.uint8)
    topo = Topology(zone, 3)
    topo.cut(1, 2)
    rng = np.random.default_rng(5)
    t = rng.integers(-1, n, (n, 5)).astype(np.int32)
    out, dropped = filter_targets_zoned(t, zone, topo.link)
    want = t.copy()
    cnt = 0
    for o in range(n):
        for s in range(5):
            j = t[o, s]
            if j >= 0 and {int(zone[o]), int(zone[j])} == {1, 2}:
                want[o, s] = -1
                cnt += 1
    assert np.array_equal(out, want) and dropped == cnt > 0


# ---------------------------------------------------------------- components and the clocks
def test_components_follow_chains():
    topo = Topology(np.arange(3, dtype=np.uint8), 3)
    topo.cut(0, 2)
    assert topo.components() == [[0, 1, 2]]  # 0 - 1 - 2: gossip relays through zone 1
    assert topo.reachable([1, 1, 0]).tolist() == [[True, True, False]]
    topo.cut(1, 2, both=False)
    assert topo.components() == [[0, 1], [2]]
    assert topo.zone_components().tolist() == [0, 0, 1]
    assert topo.reachable([1, 0, 1]).tolist() == [[True, False, False], [False, False, True]]
    topo.heal(2, 1)
    assert topo.components() == [[0, 1, 2]]
    topo.split([[1]])
    assert topo.components() == [[0], [1], [2]]  # 0 - 2 is still cut, and the only chain between them ran through 1
    topo.heal(0, 2)
    assert topo.components() == [[0, 2], [1]] and topo.link[0, 1] == LINK_DOWN
    topo.heal_all()
    assert topo.components() == [[0, 1, 2]] and not topo.link.any()


def test_heal_restores_the_links_loss():
    topo = Topology(np.array([0, 1], np.uint8), 2)
    topo.set_link(0, 1, loss=0.25, both=False)
    topo.cut(0, 1)
    topo.heal(0, 1)
    assert topo.link.tolist() == [[0, loss_q32(0.25)], [0, 0]]


def test_unreachable_since_takes_the_earliest_cause_in_force():
    zone = np.array([0, 0, 1, 1, 2], np.uint8)
    topo = Topology(zone, 3)
    down, links = DownClock(5), LinkClock(3)
    up = np.ones(5, bool)
    down.update(up, 0)
    links.update(topo, 0)
    up[2] = False  # node 2 (zone 1) goes down at tick 64, before the split
    down.update(up, 64)
    topo.split([[0], [1, 2]])
    links.update(topo, 128)
    up[3] = False  # node 3 (zone 1) goes down at tick 192, after it
    down.update(up, 192)
    us = links.unreachable_since(topo, up, down)
    assert topo.components() == [[0], [1, 2]]
    # for zone 0's observers: node 2 keeps its own tick (64 < 128), node 3 and node 4 were lost with the link
    assert us[0].tolist() == [0, 0, 64, 128, 128]
    # for the other side: zone 0 since the split, its own down nodes since they went down
    assert us[1].tolist() == [128, 128, 64, 192, 0]
    # healed: the separation is no cause any more; the down nodes keep theirs
    topo.heal_all()
    links.update(topo, 256)
    assert links.unreachable_since(topo, up, down).tolist() == [[0, 0, 64, 192, 0]]
    # split again: a new tick
    topo.split([[0], [1, 2]])
    links.update(topo, 320)
    assert links.unreachable_since(topo, up, down.down_since)[0].tolist() == [0, 0, 64, 192, 320]
    stale = LinkClock(3)
    with pytest.raises(ValueError):
        stale.unreachable_since(topo, up, down)


# ---------------------------------------------------------------- the references agree with each other
def test_zoned_reference_is_the_sum_of_its_components():
    """The pairwise reference of the zoned census equals the per-component references merged as the header says."""
    from detectref import HISTS, TOTALS

    n = 40
    rng = np.random.default_rng(9)
    tod = np.where(rng.random((n, n)) < 0.3, rng.integers(0, 500, (n, n)), -1)
    live = ((tod < 0) & (rng.random((n, n)) < 0.8)).astype(np.int32)
    last = np.where(rng.random((n, n)) < 0.7, rng.integers(300, 600, (n, n)), -1)
    ex = {"live": live, "tod": tod, "fd_last": last, "fd_len": rng.integers(0, 6, (n, n)),
          "fd_sum": rng.integers(0, 640, (n, n)) / 64.0}
    zone = (np.arange(n) // 14).astype(np.uint8)
    topo = Topology(zone, 3)
    down, links = DownClock(n), LinkClock(3)
    up = rng.random(n) < 0.8
    down.update(np.ones(n, bool), 0)
    down.update(up, 100)
    links.update(topo, 0)
    topo.split([[2]])
    links.update(topo, 200)
    thr = (0.5, 2.0)
    whole = zoned_reference(ex, up, topo, down, links, 640, thr, 5.0)
    comp = topo.node_components()
    reach, since = topo.reachable(up), links.unreachable_since(topo, up, down)
    parts = [detect_reference_for(ex, up & (comp == c), reach[c], since[c], 640, thr, 5.0) for c in range(2)]
    for k in TOTALS:
        f = max if k.startswith("max_") else sum
        assert whole[k] == f(p[k] for p in parts), k
    for k in HISTS + ("up_over", "down_over"):
        assert whole[k] == [sum(x) for x in zip(*(p[k] for p in parts))], k
    assert whole["down_dead"] > 0 and whole["up_dead"] > 0 and sum(whole["detect_latency_hist"]) > 0
    # observers == up is detectref's reference
    from detectref import detect_reference

    a = detect_reference_for(ex, up, up, down.down_since, 640, thr, 5.0)
    b = detect_reference(ex, up, down.down_since, 640, thr, 5.0)
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    # an observer that is itself a down target: its own pair is in neither count
    obs = np.ones(n, bool)
    c = detect_reference_for(ex, obs, up, None, 640, (), 5.0)
    assert c["up_pairs"] == int(up.sum()) * (n - 1) and c["down_pairs"] == int((~up).sum()) * (n - 1)
    assert pairwise_reference is not None


# ---------------------------------------------------------------- the driver
def test_prepare_applies_link_events_per_round():
    import torch

    from aiocluster_amd import driver

    n = 240
    topo = Topology.blocks([0, 100, 200, 240])
    topo.set_link(0, 1, loss=0.3, both=False)
    events = [(2, "split", [[2]]), (4, "heal_all", ())]
    spec = WorkloadSpec(n=n, k=4, fanout=3, seed=12, init="warm", write_frac=0.2, cut_seed=0xC07, topology=topo,
                        link_events=events)
    plans = driver.prepare(spec, 6, torch, "cpu")
    wl = Workload(WorkloadSpec(n=n, k=4, fanout=3, seed=12, init="warm", write_frac=0.2))
    zone = topo.zone
    removed = 0
    for rd in plans:
        plan = wl.next_round()
        r = rd["r"]
        split = 2 <= r < 4
        assert rd["topo"].components() == ([[0, 1], [2]] if split else [[0, 1, 2]])
        assert rd["exchanges"] + rd["no_connect"] == plan.n_exchanges
        assert len(rd["phases"]) == len(plan.phases) == len(rd["legs"])
        for i, ((a, b, m, _), (pa, pb)) in enumerate(zip(rd["phases"], plan.phases)):
            a, b = a.numpy(), b.numpy()
            cross = (zone[a] == 2) != (zone[b] == 2)
            assert not (split and cross.any())
            ok = rd["topo"].connect_ok(pa, pb)
            assert np.array_equal(a, pa[ok]) and np.array_equal(b, pb[ok]) and m == int(ok.sum())
            legs = rd["legs"][i].numpy()
            assert np.array_equal(legs, draw_cuts_zoned(a, b, 0xC07, r, i, zone, rd["link"])) and (legs <= 3).all()
        if split:
            assert rd["no_connect"] > 0
            removed += rd["no_connect"]
        else:
            assert rd["no_connect"] == 0
    assert removed > 0
    assert not (topo.link == LINK_DOWN).any()  # the spec's own topology is untouched
    # no lossy link: plain phases (no legs); a loss together with a topology is refused
    whole = Topology.blocks([0, 100, 200, 240])
    rd = driver.prepare(WorkloadSpec(n=n, k=4, seed=12, topology=whole, link_events=[(0, "split", [[2]])]), 1, torch, "cpu")[0]
    assert "legs" not in rd and rd["no_connect"] > 0 and not rd["zoned_loss"]
    with pytest.raises(ValueError):
        driver.prepare(WorkloadSpec(n=n, k=4, loss=0.1, topology=whole), 1, torch, "cpu")
    with pytest.raises(ValueError):
        driver.prepare(WorkloadSpec(n=n, k=4, link_events=events), 1, torch, "cpu")
    assert "topo" not in driver.prepare(WorkloadSpec(n=n, k=4, seed=12), 1, torch, "cpu")[0]


def test_partition_scenario_matches_prepare():
    import torch

    from aiocluster_amd import driver
    from aiocluster_amd.scenario import make_scenario

    n = 120
    topo = Topology.blocks([0, 50, 100, 120])
    topo.set_link(0, 1, loss=0.3, both=False)
    events = [(1, "split", [[2]]), (2, "heal_all", ())]
    base = WorkloadSpec(n=n, k=2, fanout=2, seed=3, init="warm", write_frac=0.1)
    scen = partition_scenario(make_scenario("p120", base, 3, {}), topo, events, 0xC07)
    spec = WorkloadSpec(n=n, k=2, fanout=2, seed=3, init="warm", write_frac=0.1, cut_seed=0xC07, topology=topo,
                        link_events=events)
    for rd, sr in zip(driver.prepare(spec, 3, torch, "cpu"), scen["rounds"]):
        assert rd["no_connect"] == sr["no_connect"]
        for (a, b, m, _), ph, lg, dl in zip(rd["phases"], sr["phases"], sr["legs"], rd["legs"]):
            assert np.array_equal(np.stack([a.numpy(), b.numpy()], 1).reshape(-1, 2), np.asarray(ph).reshape(-1, 2))
            assert dl.numpy().tolist() == lg
    assert scen["rounds"][1]["no_connect"] > 0

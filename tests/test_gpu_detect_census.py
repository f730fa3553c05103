"""gs_detect_census, the device-side detection census (GPU only).

Every expected value is ``detect_reference`` (tests/detectref.py, checked on the host against hand-computed values):
over the real reference's own states for the golden fixtures, over readback (``export()``, or the four FD regions
decoded as ``export()`` decodes them) everywhere else.  Every comparison is exact.

What the census answers in the reference's terms: ``FailureDetector.live_nodes`` / ``dead_nodes`` / ``phi``
(``aiocluster/failure_detector.py:60-87``) of every up observer, against the caller's ground truth.
"""

import functools

import numpy as np
import pytest
from detectref import HISTS, TOTALS, arrays_of_export, assert_census, detect_reference
from helpers import load_scenario, make_backend
from lossycases import add_legs

from aiocluster_amd import driver
from aiocluster_amd.detect import DownClock
from aiocluster_amd.scenario import DEFAULT_CFG, make_scenario, replay_round, round_ticks
from aiocluster_amd.shard import ShardGroup
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.workload import (WorkloadSpec, key_names, liveness_tick, permutation_phases, phase_tick,
                                     round_tick, synthetic_node_ids)

pytestmark = pytest.mark.gpu

SWEEP = (0.55, 1.05, 2.05, 4.1)  # tests/test_detect_census_host.py: clear of every fixture phi, counts inside (0, all)
# deaths within a few rounds (fdgc12's detector): a round is one second
FD_CFG = {"phi_threshold": 2.0, "max_interval_s": 10.0, "dead_grace_s": 8.0, "initial_interval_s": 1.0, "mtu": 1 << 30}
PRIOR5 = 5.0 * FD_CFG["initial_interval_s"]


def dev_u8(sim, a):
    return sim.torch.from_numpy(np.asarray(a, dtype=np.uint8)).to(sim.device)


def fd_readback(sim) -> dict:
    """The census's inputs decoded as ``export()`` decodes them, from the four FD regions alone (no key-value
    arrays: usable at thousands of nodes)."""
    torch = sim.torch
    sim.sync()
    n, NP, nc = sim.n, sim.np_, sim.ncol
    st8 = sim.region("FD_STATE", torch.uint8, (n, NP)).cpu().numpy()
    tod = sim.region("FD_TOD", torch.int32, (n, NP)).cpu().numpy().view(np.uint32)
    last, sm, cnt = sim.unpack_fd(st8, sim.region("FD_LAST", torch.int16, (n, NP)).cpu().numpy(),
                                  sim.region("FD", torch.int32, (n, NP)).cpu().numpy(), sim.latest_tick())
    none = last == 0xFFFFFFFF
    W = int(sim.cfg["window"])
    mem = (st8 & 3)[:, :nc]
    return {"live": (mem == 1).astype(np.int32), "tod": np.where(mem == 2, tod[:, :nc].astype(np.int64), -1),
            "fd_last": np.where(none, -1, last.astype(np.int64))[:, :nc],
            "fd_len": np.where(none, 0, np.minimum(cnt, W))[:, :nc],
            "fd_sum": np.where(none, 0.0, sm / 64.0)[:, :nc]}


def check(sim, ex, up_host, ds, tick, what, thresholds=SWEEP):
    """The device's census of ``sim`` against the reference over ``ex``, with and without thresholds."""
    prior5 = 5.0 * float(sim.cfg["initial_interval_s"])
    up = dev_u8(sim, up_host)
    got = sim.detect_census(up, tick, ds, thresholds, per_target=True, per_row=True)
    want = detect_reference(ex, up_host, ds, tick, thresholds, prior5, sim.col_lo)
    assert_census(got, want, what)
    bare = sim.detect_census(up, tick, ds, (), per_target=True, per_row=True)
    assert_census(bare, detect_reference(ex, up_host, ds, tick, (), prior5, sim.col_lo), (what, "state only"))
    return got


def assert_nonzero(c, what):
    for k in ("up_dead", "down_dead", "down_live", "early_deaths", "max_detect_latency", "max_undetected_age",
              "max_false_age", "up_phi", "down_phi"):
        assert c[k] > 0, (what, k)
    for k in HISTS:
        assert sum(c[k]) > 0, (what, k)
    assert any(0 < x < c["up_phi"] for x in c["up_over"]), (what, c["up_over"], c["up_phi"])
    assert any(0 < x < c["down_phi"] for x in c["down_over"]), (what, c["down_over"], c["down_phi"])


# ---------------------------------------------------------------- 1. the reference's fixtures
PREFIX = dict(tombstones=False, fd_ring=False)
FIXTURE_CASES = [
    ("fdgc12", {}), ("fdgc12", dict(tombstones=False)), ("fdgc12", dict(tombstones=False, held=False)),
    ("q9x10", {}), ("q9x10", dict(tombstones=False)), ("q9x10", dict(tombstones=False, held=False)),
    ("sched16", {}), ("sched16", dict(tombstones=False)),
    ("cutw12", dict(canonical=False)), ("cutw12", dict(fd_ring=False)), ("cutw12", dict(PREFIX)),
    ("cutgc12", {}),
]


@pytest.mark.parametrize("name,kw", FIXTURE_CASES, ids=[f"{n}-{'-'.join(k) or 'default'}" for n, k in FIXTURE_CASES])
def test_census_equals_the_reference_over_the_fixtures_states(name, kw):
    """After every round the device's census equals the reference computed from the REAL reference's state of that
    round (its live / dead sets, times of death, windows and phi values), not from the device's readback."""
    scen = load_scenario(name)
    n = scen["n"]
    sim = make_backend(GossipSim, scen, **kw)
    clock = DownClock(n)
    seen = dict.fromkeys(("up_dead", "down_dead", "down_live", "up_over", "down_over"), False)
    for r, rd in enumerate(scen["rounds"]):
        replay_round(sim, scen, r)
        ds = clock.update(rd["up"], round_tick(r))
        tick = round_ticks(scen, r)[-1]
        assert tick == sim.last_tick
        got = sim.detect_census(dev_u8(sim, rd["up"]), down_since=ds, thresholds=SWEEP, per_target=True, per_row=True)
        want = detect_reference(scen["expect"]["states"][r], rd["up"], ds, tick, SWEEP)
        assert_census(got, want, (name, r))
        assert got["old_windows"] == 0
        for k in ("up_dead", "down_dead", "down_live"):
            seen[k] |= got[k] > 0
        seen["up_over"] |= any(0 < x < got["up_phi"] for x in got["up_over"])
        seen["down_over"] |= any(0 < x < got["down_phi"] for x in got["down_over"])
    assert all(seen.values()), (name, seen)
    sim.close()


# ---------------------------------------------------------------- 2. every layout against readback
LAYOUTS = {
    "u16_tombstones": ("warm", dict(tombstones=True, fd_ring=False)),
    "hb8": ("warm", dict(tombstones=False, fd_ring=False, hb8=True)),
    "hb8mv8": ("warm", dict(tombstones=False, fd_ring=False, hb8=True, mv8=True)),
    "cold_general": ("cold", dict(tombstones=True, fd_ring=False)),
    "no_held": ("warm", dict(tombstones=False, held=False, fd_ring=False)),
    "fd_ring": ("warm", dict(tombstones=True, fd_ring=True)),
    "ring_rows": ("warm", dict(tombstones=False, fd_ring=False, ring_rows=[3, 150, 299])),
}


@functools.lru_cache(maxsize=None)
def churn_scenario(init: str) -> dict:
    """300 nodes (4 x 64 + 44 columns), 4 keys, 8 rounds, 15 % of the nodes down for 3 rounds each, a fifth of the
    messages lost.  Through the CPU oracle this workload (seed 7) gives deaths, false suspicions, undetected
    failures, early deaths and threshold counts inside their range from the fourth round on, warm and cold."""
    spec = WorkloadSpec(n=300, k=4, fanout=3, seed=7, init=init, write_frac=0.3, down_frac=0.15, down_rounds=3)
    return add_legs(make_scenario(f"detect_{init}", spec, 8, FD_CFG), 0.2)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_census_matches_readback_in_every_layout(layout):
    init, kw = LAYOUTS[layout]
    scen = churn_scenario(init)
    n = scen["n"]
    sim = make_backend(GossipSim, scen, hist_cap=16, **kw)
    clock = DownClock(n)
    for r, rd in enumerate(scen["rounds"]):
        replay_round(sim, scen, r)
        ds = clock.update(rd["up"], round_tick(r))
        if r not in (3, 7):
            continue
        tick = sim.last_tick
        ex = sim.export()
        got = check(sim, ex, rd["up"], ds, tick, (layout, r))
        assert_nonzero(got, (layout, r))
        ones = check(sim, ex, [1] * n, ds, tick, (layout, r, "all up"))
        assert ones["down_pairs"] == 0 and ones["up_pairs"] == n * (n - 1) and ones["observers"] == n
        if layout == "cold_general":
            assert got["up_unknown"] > 0
        # phi itself, of two rows, against gs_phi_row (which the golden fixtures pin to the reference)
        phi = arrays_of_export(ex, tick, PRIOR5)["phi"]
        for o in (3, n - 1):
            dev = sim.phi_row(o, tick)
            assert np.array_equal(np.isnan(dev), np.isnan(phi[o])), (layout, r, o)
            m = ~np.isnan(dev)
            assert m.any() and np.array_equal(dev[m], phi[o][m]), (layout, r, o)
    sim.close()


# ---------------------------------------------------------------- 3. chunk and band boundaries
def make_warm(n, K, cfg=FD_CFG, **over):
    kw = dict(init="warm", tombstones=False, fd_ring=False, hist_cap=16, initial_ops=driver.boot_ops(n, K), hb8=True,
              mv8=True)
    kw.update(over)
    return GossipSim(synthetic_node_ids(n), key_names(K), dict(DEFAULT_CFG, **cfg), **kw)


def test_census_across_chunk_and_band_boundaries():
    """One row band (256) + one column chunk (4,096) + 37: 18 bands, the last of 37 rows; two column chunks, the
    second of 293 columns (4 x 64 + 37: a partial last group); the diagonal of most bands lies in a chunk that is
    not the band's first workgroup."""
    import torch

    n, K = 256 + 4096 + 37, 4
    sim = make_warm(n, K)
    spec = WorkloadSpec(n=n, k=K, fanout=3, seed=42, init="warm", write_frac=0.05, down_frac=0.15, down_rounds=3)
    plans = driver.prepare(spec, 3, torch, sim.device)
    clock = DownClock(n)
    for rd in plans:
        driver.run_round([sim], rd)
        ds = clock.update(rd["up_host"], rd["t"])
    got = check(sim, fd_readback(sim), rd["up_host"], ds, rd["t_live"], "4389")
    for k in ("up_dead", "down_dead", "down_live", "up_phi", "down_phi", "max_detect_latency", "max_false_age"):
        assert got[k] > 0, k
    assert any(0 < x < got["up_phi"] for x in got["up_over"])
    dead_by = got["target_dead_by"].cpu().numpy()
    assert dead_by[:4096].any() and dead_by[4096:].any()
    rows = got["row_false_suspicions"].cpu().numpy()
    assert rows[:256].any() and rows[4352:].any()
    sim.close()


# ---------------------------------------------------------------- 4. old windows
def test_old_windows_count_above_every_threshold():
    """Four nodes are down while the others gossip through ticks that advance 4,000 at a time.  The liveness sweep
    does not run for a down observer, so its windows keep their intervals while their last reports age: after nine
    steps they are 2^15 ticks old or more, and k_fd_age has marked them old.  Counted as observers (the mask is the
    caller's: here all ones, a node back up before its first sweep), every such window is in old_windows and above
    every valid threshold (51.19 is just below DEFAULT_CFG's bound of 2^15 / 640); the census leaves the counters
    alone, err_fd_overflow included.  (A window about a node its observer has declared dead is reset, so the up
    observers' windows about the down nodes hold no phi.)"""
    import torch

    n, K = 64, 2
    sim = make_warm(n, K, cfg={}, hb8=False, mv8=False)
    up = np.ones(n, np.uint8)
    ring = [[(i, i | s) for i in range(n) if not i & s] for s in (1, 2, 4, 8, 16, 32)]  # hypercube matchings
    clock = DownClock(n)
    t = 0
    for r in range(6):  # every window gains intervals
        t = round_tick(r)
        sim.begin_round(t, up)
        for p, pairs in enumerate(ring):
            sim.run_phase(t + 1 + p, pairs)
        sim.liveness(t + 8, up)
        clock.update(up, t)
    up[60:] = 0
    ones = np.ones(n, np.uint8)
    thr = (0.5, 8.0, 51.19)
    seen_old = False
    for step in range(10):
        t += 4000
        ds = clock.update(up, t)
        sim.begin_round(t, up)
        for p, pairs in enumerate(ring):
            sim.run_phase(t + 1 + p, [(a, b) for a, b in pairs if up[a] and up[b]])
        sim.liveness(t + 8, up)
        if step < 7:
            continue
        c0 = sim.counters()
        rb = fd_readback(sim)
        got = check(sim, rb, up, ds, sim.last_tick, ("old", step), thresholds=thr)
        assert got["old_windows"] == 0 and got["down_dead"] == 60 * 4
        every = check(sim, rb, ones, ds, sim.last_tick, ("old, all rows", step), thresholds=thr)
        assert sim.counters() == c0 and c0["err_fd_overflow"] == 0
        if step >= 8:  # 9 x 4,000 ticks after the down observers' last reports
            seen_old = True
            assert every["old_windows"] == 4 * (n - 1)
            assert all(x >= every["old_windows"] for x in every["up_over"]), every["up_over"]
        else:
            assert every["old_windows"] == 0
    assert seen_old
    st = sim.region("FD_STATE", torch.uint8, (n, sim.np_)).cpu().numpy()
    assert (st[60:, :60] & 8).all(), "k_fd_age marked the down observers' windows old"
    sim.close()


# ---------------------------------------------------------------- 5. read-only and repeatable
def test_census_is_read_only_and_repeatable():
    import torch

    scen = churn_scenario("warm")
    sim = make_backend(GossipSim, scen, hist_cap=16, **LAYOUTS["hb8mv8"][1])
    clock = DownClock(scen["n"])
    for r in range(5):
        replay_round(sim, scen, r)
        ds = clock.update(scen["rounds"][r]["up"], round_tick(r))
    up = dev_u8(sim, scen["rounds"][4]["up"])

    def snap():
        sim.sync()
        return {r: sim.regions[r].cpu().numpy().tobytes() for r in ("FD", "FD_LAST", "FD_STATE", "FD_TOD")}

    before, c0 = snap(), sim.counters()
    a = sim.detect_census(up, down_since=ds, thresholds=SWEEP, per_target=True, per_row=True)
    b = sim.detect_census(up, down_since=ds, thresholds=SWEEP, per_target=True, per_row=True)
    after, c1 = snap(), sim.counters()
    assert before == after
    assert c0 == c1
    for k in a:
        if hasattr(a[k], "cpu"):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k
    assert a["up_dead"] > 0 and a["down_dead"] > 0 and a["up_phi"] > 0
    # without thresholds: the same state fields, the window fields zero
    bare = sim.detect_census(up, down_since=ds, per_target=True, per_row=True)
    for k in TOTALS + HISTS:
        if k in ("up_windows", "down_windows", "up_phi", "down_phi", "old_windows"):
            assert bare[k] == 0, k
        else:
            assert bare[k] == a[k], k
    assert bare["up_over"] == [] and bare["down_over"] == []
    for k in a:
        if hasattr(a[k], "cpu"):
            assert torch.equal(a[k], bare[k]), k
    assert snap() == before and sim.counters() == c0
    sim.close()


# ---------------------------------------------------------------- 6. slices
def test_three_slices_give_one_handles_census():
    """1,100 nodes in three slices of 384 / 384 / 332 owner columns against one handle of the same cluster."""
    import torch

    n, K = 1100, 4
    cfg = dict(DEFAULT_CFG, **FD_CFG)
    kw = dict(init="warm", tombstones=False, fd_ring=False, hist_cap=16, initial_ops=driver.boot_ops(n, K), hb8=True,
              mv8=True)
    ids, keys = synthetic_node_ids(n), key_names(K)
    one = GossipSim(ids, keys, cfg, **kw)
    grp = ShardGroup.in_process(ids, keys, cfg, shards=3, **kw)
    assert [s.ncol for s in grp.slices] == [384, 384, 332]
    spec = WorkloadSpec(n=n, k=K, fanout=3, seed=21, init="warm", write_frac=0.1, down_frac=0.15, down_rounds=3)
    plans = driver.prepare(spec, 4, torch, one.device)
    clock = DownClock(n)
    for rd in plans:
        driver.run_round([one], rd)
        driver.run_round(grp.slices, rd, group=grp)
        ds = clock.update(rd["up_host"], rd["t"])
    tick, up = rd["t_live"], rd["up"]
    a = one.detect_census(up, tick, ds, SWEEP, per_target=True, per_row=True)
    b = grp.detect_census(up, tick, ds, SWEEP, per_target=True, per_row=True)
    assert set(a) == set(b)
    for k in a:
        if hasattr(a[k], "cpu"):
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])
    assert_census(a, detect_reference(fd_readback(one), rd["up_host"], ds, tick, SWEEP, PRIOR5), "one handle")
    for k in ("up_dead", "down_dead", "down_live", "max_detect_latency", "max_false_age", "up_phi"):
        assert a[k] > 0, k
    # each slice alone counts its own target columns; the maxima and the times of death combine as the header says
    parts = []
    for s in grp.slices:
        got = s.detect_census(up, tick, ds, SWEEP, per_target=True, per_row=True)
        assert_census(got, detect_reference(fd_readback(s), rd["up_host"], ds, tick, SWEEP, PRIOR5, s.col_lo),
                      f"slice {s.shard}")
        assert got["observers"] == a["observers"]
        parts.append(got)
    for k in ("max_detect_latency", "max_undetected_age", "max_false_age"):
        assert max(p[k] for p in parts) == a[k], k
    first = torch.cat([p["target_first_tod"] for p in parts])
    assert torch.equal(first, a["target_first_tod"])
    assert torch.equal(torch.stack([p["row_undetected"] for p in parts]).sum(0, dtype=torch.int32), a["row_undetected"])
    one.close()
    for s in grp.slices:
        s.close()


# ---------------------------------------------------------------- 7. a detection curve
CURVE = dict(n=2048, K=2, warm=4, down=range(4, 12), back=2, fanout=3, seed=5, first_down=900, n_down=200)


def curve_rounds(spec=CURVE):
    """The schedule of the detection-curve run: (round, up mask, phases as (initiators, responders) arrays)."""
    n = spec["n"]
    rng = np.random.default_rng(spec["seed"])
    for r in range(spec["warm"] + len(spec["down"]) + spec["back"]):
        up = np.ones(n, np.uint8)
        if r in spec["down"]:
            up[spec["first_down"]:spec["first_down"] + spec["n_down"]] = 0
        phases = []
        for _ in range(spec["fanout"]):
            for a, b in permutation_phases(rng.permutation(n).astype(np.int32)):
                keep = (up[a] & up[b]).astype(bool)
                phases.append((a[keep], b[keep]))
        yield r, up, phases


def test_detection_curve_of_200_failures():
    """200 of 2,048 nodes go down at once.  While they are down the pairs holding them dead only grow (nothing
    reports a down node's heartbeat as new once the cluster has heard its last one, which the run's fanout makes
    sure of before the first detection); per target the first detection is at or before the last; and the
    latencies read from the per-target planes agree with the histogram's maximum."""
    import torch

    n = CURVE["n"]
    sim = make_warm(n, CURVE["K"])
    clock = DownClock(n)
    lo, hi = CURVE["first_down"], CURVE["first_down"] + CURVE["n_down"]
    curve = []
    for r, up, phases in curve_rounds():
        t = round_tick(r)
        up_dev = dev_u8(sim, up)
        sim.begin_round(t, up_dev)
        for p, (a, b) in enumerate(phases):
            sim.run_phase_arrays(phase_tick(r, p), torch.from_numpy(a).to(sim.device), torch.from_numpy(b).to(sim.device))
        sim.liveness(liveness_tick(r, len(phases)), up_dev)
        ds = clock.update(up, t)
        if r not in CURVE["down"]:
            continue
        c = sim.detect_census(up_dev, down_since=ds, per_target=True)
        assert c["down_pairs"] == (n - CURVE["n_down"]) * CURVE["n_down"]
        assert c["down_dead"] + c["down_live"] == c["down_pairs"] and c["early_deaths"] == 0
        curve.append(c["down_dead"])
        first = c["target_first_tod"].cpu().numpy().astype(np.int64)[lo:hi]
        last = c["target_last_tod"].cpu().numpy().astype(np.int64)[lo:hi]
        det = c["target_dead_by"].cpu().numpy()[lo:hi] > 0
        assert ((first >= 0) == det).all() and ((last >= 0) == det).all()
        assert (first[det] <= last[det]).all()
        if det.any():
            t_down = round_tick(CURVE["down"][0])
            assert (first[det] >= t_down).all()
            assert int((last[det] - t_down).max()) == c["max_detect_latency"]
            assert sum(c["detect_latency_hist"]) == c["down_dead"]
    assert all(b >= a for a, b in zip(curve, curve[1:])), curve
    assert curve[0] < curve[-1] == (n - CURVE["n_down"]) * CURVE["n_down"], curve
    sim.close()


# ---------------------------------------------------------------- 8. a communicator
@pytest.fixture(scope="module")
def nccl_world1():
    import socket

    import torch
    import torch.distributed as dist

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


def test_world1_distcomm_gives_the_slices_own_census(nccl_world1):
    """ShardGroup.detect_census over a DistComm: the all-reduce of the sums and maxima and the padded gather of the
    per-target planes, on a world-1 process group over a GS_SLICED one-slice cluster."""
    import torch

    from aiocluster_amd.shard import DistComm

    n, K = 300, 4
    cfg = dict(DEFAULT_CFG, **FD_CFG)
    one = make_warm(n, K, sliced=True)
    grp = ShardGroup([one], DistComm(), cfg["mtu"])
    spec = WorkloadSpec(n=n, k=K, fanout=3, seed=2, init="warm", write_frac=0.1, down_frac=0.15, down_rounds=3)
    plans = driver.prepare(spec, 4, torch, one.device)
    clock = DownClock(n)
    for rd in plans:
        driver.run_round([one], rd, group=grp)
        ds = clock.update(rd["up_host"], rd["t"])
    tick, up = rd["t_live"], rd["up"]
    a = one.detect_census(up, tick, ds, SWEEP, per_target=True, per_row=True)
    b = grp.detect_census(up, tick, ds, SWEEP, per_target=True, per_row=True)
    assert set(a) == set(b)
    for k in a:
        if hasattr(a[k], "cpu"):
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])
    assert_census(a, detect_reference(fd_readback(one), rd["up_host"], ds, tick, SWEEP, PRIOR5), "world-1")
    for k in ("up_dead", "down_dead", "down_live", "up_phi", "max_detect_latency"):
        assert a[k] > 0, k
    one.close()

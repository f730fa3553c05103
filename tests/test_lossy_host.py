"""Cut exchanges on the host (no GPU): the oracle composer against the reference's fixtures, the ABI, the draw,
the scenario replay, and the oracle-only preconditions of tests/test_gpu_lossy.py."""

import ctypes as C
import os
import re

import numpy as np
import pytest
from helpers import load_scenario, make_backend, replay_and_compare
from lossycases import (CUT_SEED, LOSS, CutOracleSim, cold_lossy, cut8, cutgc12, cutw12, cutw12s, legs_counts,
                        warm_lossy, windows_below_capacity)
from peer_select import philox4x32

from aiocluster_amd import _lib
from aiocluster_amd.cuts import draw_cuts, draw_cuts_q32, loss_q32
from aiocluster_amd.scenario import replay, replay_round

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the composer against the reference
@pytest.mark.parametrize("name,block", [("cutw12", "expect"), ("cutw12s", "expect"), ("cutgc12", "expect"),
                                        ("cut8", "expect_w1000")])
def test_composer_matches_reference(name, block):
    """The composer replays the reference's fixture to the reference's state in every round (cut8: its rerun with
    window 1000 -- the composer's limit is an Ack-lost cut on a window that has rolled over)."""
    scen = load_scenario(name)
    exp = scen[block]
    if block != "expect":
        scen["config"] = dict(scen["config"], window=1000)
    orc = make_backend(CutOracleSim, scen)
    bad = replay_and_compare(orc, scen, expect_states=exp["states"], expect_hashes=exp["hashes"])
    assert bad is None, f"round {bad[0]}: {bad[1]}"
    assert orc.q9_events == exp["q9"]
    assert orc.cut_exchanges == sum(legs_counts(scen)[:3]) > 0
    orc.close()


@pytest.mark.parametrize("make", [cut8, cutw12, cutw12s, cutgc12])
def test_fixture_inputs_are_the_builders(make):
    """The fixtures' inputs (legs included) are what tests/lossycases.py builds: the generator is reproducible."""
    want = make()
    scen = load_scenario(want["name"])
    for k in want:
        assert scen[k] == want[k], k
    assert min(legs_counts(scen)) >= 20


# ---------------------------------------------------------------- 2. ABI
def test_header_declares_cut_entry_points():
    hdr = open(os.path.join(REPO, "include", "gossip_sim.h")).read()
    assert re.search(r"int gs_run_phase_cut\(gs_handle \*h, const int32_t \*initiators, const int32_t \*responders,"
                     r"\s*const uint8_t \*legs,\s*uint32_t n, uint32_t tick\);", hdr)
    assert re.search(r"int gs_draw_cuts\(gs_handle \*h, const int32_t \*initiators, const int32_t \*responders, "
                     r"uint32_t n,\s*uint64_t seed,\s*uint32_t round, uint32_t phase, uint32_t loss_q32, "
                     r"uint8_t \*legs\);", hdr)
    assert "#define GS_API_VERSION 23" in hdr
    assert "gs_run_phase_cut" in _lib.EXPORTS and "gs_draw_cuts" in _lib.EXPORTS


def test_api_version_and_counters():
    assert _lib.API_VERSION == 23
    lib = _lib.load()
    assert lib.gs_api_version() == 23
    # (COUNTER_FIELDS stays the vector of bench.py's counters.npy; the new field is listed after it)
    assert "cut_exchanges" in _lib.ALL_COUNTER_FIELDS and len(_lib.COUNTER_FIELDS) == 33
    assert hasattr(_lib.GsCounters, "cut_exchanges")
    assert C.sizeof(_lib.GsCounters) == 40 * 8  # taken from `reserved`: the struct size does not change
    assert _lib.GsCounters.cut_exchanges.offset == 8 * _lib.ALL_COUNTER_FIELDS.index("cut_exchanges") == 8 * 33


# ---------------------------------------------------------------- 3. draw_cuts
def test_draw_cuts_is_philox_of_round_initiator_responder_phase():
    seed = 0x1234_5678_9ABC_DEF0
    q = loss_q32(0.4)
    cases = [(0, 0, 1, 0), (3, 17, 4, 2), (41, 1099, 0, 8), (7, 65535, 65534, 63), (2**31, 5, 9, 2**20)]
    for rnd, a, b, ph in cases:
        w = philox4x32([rnd, a, b, ph], seed & 0xFFFFFFFF, seed >> 32)
        want = 0 if w[0] < q else 1 if w[1] < q else 2 if w[2] < q else 3
        assert draw_cuts_q32([a], [b], seed, rnd, ph, q).tolist() == [want], (rnd, a, b, ph)
    got = draw_cuts([c[1] for c in cases[:3]], [c[2] for c in cases[:3]], seed, 3, 2, 0.4)
    assert got.dtype == np.uint8 and got[1] == draw_cuts_q32([17], [4], seed, 3, 2, q)[0]


def test_loss_q32():
    assert loss_q32(0.0) == 0 and loss_q32(1.0) == 2**32 - 1 and loss_q32(0.25) == 2**30
    with pytest.raises(ValueError):
        loss_q32(1.5)


def test_no_loss_delivers_everything():
    ini = np.arange(5000)
    assert (draw_cuts(ini, ini + 1, 99, 4, 1, 0.0) == 3).all()


def test_draw_frequencies():
    """At loss 0.25 over 200,000 exchanges the four frequencies are within 5 binomial standard deviations of
    p, (1-p) p, (1-p)^2 p and (1-p)^3."""
    n = 200_000
    rng = np.random.default_rng(5)
    legs = draw_cuts(rng.integers(0, 65536, n), rng.integers(0, 65536, n), 2024, 11, 3, 0.25)
    for v, p in enumerate((0.25, 0.1875, 0.140625, 0.421875)):
        sd = (p * (1 - p) / n) ** 0.5
        f = float((legs == v).mean())
        assert abs(f - p) <= 5 * sd, (v, f, p, sd)


# ---------------------------------------------------------------- 4. replay_round
class Recorder:
    def __init__(self):
        self.calls = []

    def write(self, *a):
        pass

    def begin_round(self, *a):
        pass

    def liveness(self, *a):
        pass

    def run_phase(self, *a):
        self.calls.append(a)


def test_replay_round_passes_legs_only_when_present():
    scen = {"rounds": [{"writes": [], "up": [1, 1, 1, 1], "phases": [[[0, 1]], [[2, 3], [1, 0]]]},
                       {"writes": [], "up": [1, 1, 1, 1], "phases": [[[0, 1]], [[2, 3], [1, 0]]],
                        "legs": [[2], [3, 0]]}]}
    rec = Recorder()
    replay(rec, scen)
    assert [len(c) for c in rec.calls] == [2, 2, 3, 3]  # without legs: run_phase(t, pairs) exactly as before
    assert rec.calls[2][1:] == ([[0, 1]], [2]) and rec.calls[3][1:] == ([[2, 3], [1, 0]], [3, 0])
    scen["rounds"][1]["legs"] = [[2]]
    with pytest.raises(ValueError):
        replay_round(Recorder(), scen, 1)


def test_shard_group_refuses_legs():
    from aiocluster_amd._lib import GsError
    from aiocluster_amd.shard import ShardGroup

    grp = ShardGroup.__new__(ShardGroup)  # no device: the refusal comes before anything else
    with pytest.raises(GsError, match="one-slice"):
        grp.run_phase(5, [[0, 1]], [2])
    with pytest.raises(GsError, match="one-slice"):
        grp.run_phase_arrays(5, [0], [1], [2])


# ---------------------------------------------------------------- 5. preconditions of the GPU cases
@pytest.mark.parametrize("make,kw,window", [(warm_lossy, {"rounds": 2}, 1000), (cold_lossy, {"k": 5}, 1000),
                                            (cold_lossy, {"k": 20}, 1000)])
def test_gpu_case_preconditions(make, kw, window):
    """Oracle only: every legs value occurs at least 50 times, the mtu cuts NodeDeltas, and no sampling window
    reaches its capacity (the composer's limit)."""
    scen = make(**kw)
    assert scen["config"]["window"] == window
    counts = legs_counts(scen)
    assert min(counts) >= 50, counts
    orc = make_backend(CutOracleSim, scen)
    replay(orc, scen)
    st = orc.stats()
    assert st["truncated"] > 0, st
    assert windows_below_capacity(orc, window)
    print(scen["name"], "phases", sum(len(rd["phases"]) for rd in scen["rounds"]), "legs", counts, "truncated",
          st["truncated"], "loss", LOSS, "seed", CUT_SEED)
    orc.close()


# ---------------------------------------------------------------- 6. the round driver
def test_driver_prepare_adds_legs_only_under_loss():
    import torch

    from aiocluster_amd import driver
    from aiocluster_amd.workload import WorkloadSpec

    base = dict(n=64, k=4, fanout=2, seed=9, init="warm", write_frac=0.1)
    plain = driver.prepare(WorkloadSpec(**base), 2, torch, torch.device("cpu"))
    assert all("legs" not in rd for rd in plain)  # loss == 0: nothing changes
    lossy = driver.prepare(WorkloadSpec(**base, loss=0.25, cut_seed=5), 2, torch, torch.device("cpu"))
    for rd, rp in zip(lossy, plain):
        assert len(rd["legs"]) == len(rd["phases"]) == len(rp["phases"])
        for i, ((a, b, n, t), lg) in enumerate(zip(rd["phases"], rd["legs"])):
            assert torch.equal(a, rp["phases"][i][0]) and torch.equal(b, rp["phases"][i][1])  # the same schedule
            assert lg.dtype == torch.uint8 and lg.numel() == n
            assert np.array_equal(lg.numpy(), draw_cuts(a.numpy(), b.numpy(), 5, rd["r"], i, 0.25))
    assert sum(int((lg < 3).sum()) for rd in lossy for lg in rd["legs"]) > 0

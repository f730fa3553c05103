"""The many-phase scenarios of tests/manyphases.py on the C oracle alone (CPU): each scenario that
tests/test_gpu_subphases.py replays must have the properties that make the device comparison mean something --
rounds below, inside and far past one base of report planes, deltas cut by the mtu, ring windows that roll over (or
compact windows that cannot overflow), and, with max_interval 0.25 s, reports of one pair within one round both more
and less than 16 ticks apart.  A GPU test then never passes because its input was tame.
"""

import numpy as np
import pytest
from helpers import load_scenario, make_backend
from manyphases import (DEVICE_CASES, LAYOUTS, MAX_INTERVAL_TICKS, PLANES, RING_ROWS, SLICED_CASES, SLICED_KW, Tap,
                        chunk_phases, device_scenario, rounds_past_a_base, sliced_scenario, ticks_after_subphases,
                        with_ticks)
from oracle import OracleSim

from aiocluster_amd.scenario import make_scenario, replay_round, round_ticks
from aiocluster_amd.workload import MAX_PHASES_PER_ROUND, WorkloadSpec, liveness_tick, phase_tick, round_tick


def profile(scen, rows=None):
    """Replay ``scen`` on the oracle phase by phase and watch the heartbeat views of the rows each phase touches: a
    view that rises is a report_heartbeat call (failure_detector.py:32-38; checked against the oracle's own
    hb_reports count).  Returns the largest window length seen on ``rows`` (default all), the most reports of one
    (observer, owner) pair, and how many times a pair reported twice within one round more than / at most
    MAX_INTERVAL_TICKS apart."""
    n = scen["n"]
    orc = make_backend(OracleSim, scen)
    hb = orc.export()["hb"].astype(np.int64)
    reports = np.zeros((n, n), np.int64)
    last = np.full((n, n), -1, np.int64)  # tick of the pair's previous report of this round
    far = near = 0
    max_len = 0
    for r, rd in enumerate(scen["rounds"]):
        ticks = round_ticks(scen, r)
        for j, k, op, v in rd["writes"]:
            orc.write(round_tick(r), j, k, op, v)
        orc.begin_round(round_tick(r), rd["up"])
        hb[np.arange(n), np.arange(n)] = np.diag(orc.export()["hb"])  # inc_heartbeat: a node's own, no report
        last[:] = -1
        for p, ph in enumerate(rd["phases"]):
            orc.run_phase(ticks[p], ph)
            touched = sorted({x for pair in ph for x in pair})
            now = orc.export_rows(touched)["hb"].astype(np.int64)
            for i, o in enumerate(touched):
                for j in np.flatnonzero((now[i] > hb[o]) & (hb[o] > 0)):  # from 0: the first heartbeat, no report
                    if j == o:
                        continue
                    reports[o, j] += 1
                    if last[o, j] >= 0:
                        if ticks[p] - last[o, j] > MAX_INTERVAL_TICKS:
                            far += 1
                        else:
                            near += 1
                    last[o, j] = ticks[p]
                hb[o] = now[i]
        orc.liveness(ticks[-1], rd["up"], r)
        ln = orc.export()["fd_len"]
        max_len = max(max_len, int((ln if rows is None else ln[list(rows)]).max()))
    s = orc.stats()
    assert int(reports.sum()) == s["hb_reports"], (int(reports.sum()), s["hb_reports"])
    orc.close()
    return {"max_len": max_len, "max_reports": int(reports.max()), "far": far, "near": near,
            "truncated": s["truncated"]}


def check_shape(scen):
    counts = [len(rd["phases"]) for rd in scen["rounds"]]
    assert all(len(ph) > 0 for rd in scen["rounds"] for ph in rd["phases"])
    assert any(c <= PLANES for c in counts), counts
    assert any(PLANES < c <= MAX_PHASES_PER_ROUND for c in counts), counts
    # 94 = 62 + 32: the sub-phases at the budget's last tick overflow a plane base on their own
    assert any(c > MAX_PHASES_PER_ROUND + PLANES for c in counts), counts
    assert rounds_past_a_base(scen) > 0
    for r in range(len(counts)):
        round_ticks(scen, r)  # valid


@pytest.mark.parametrize("layout,kind", DEVICE_CASES)
def test_device_scenarios_have_the_properties_the_gpu_tests_rely_on(layout, kind):
    scen = device_scenario(layout, kind)
    check_shape(scen)
    _, cfg, _, ring = LAYOUTS[layout]
    W = scen["config"]["window"]
    p = profile(scen, rows=RING_ROWS if layout == "sampled" else None)
    print(layout, kind, [len(rd["phases"]) for rd in scen["rounds"]], p)
    assert p["truncated"] > 0
    if kind == "triples":
        assert ticks_after_subphases(scen) > rounds_past_a_base(scen)
    if ring or layout == "sampled":  # some window reaches W and rolls over
        assert p["max_len"] == W and p["max_reports"] > W, p
    else:  # compact windows: err_fd_overflow cannot fire
        assert p["max_len"] < W, p
    if cfg.get("max_interval_s") == 0.25:  # both the dropped and the kept interval occur
        assert p["far"] > 0 and p["near"] > 0, p


@pytest.mark.parametrize("row,kind,n", SLICED_CASES)
def test_sliced_scenarios_have_the_properties_the_gpu_tests_rely_on(row, kind, n):
    scen = sliced_scenario(row, kind, n)
    check_shape(scen)
    W = scen["config"]["window"]
    p = profile(scen)
    print(row, kind, n, [len(rd["phases"]) for rd in scen["rounds"]], p)
    assert p["truncated"] > 0
    # some sub-phase cuts a delta: its slot totals pass the mtu, so the slices settle it in chain steps
    tap = Tap(make_backend(OracleSim, scen))
    for r in range(len(scen["rounds"])):
        replay_round(tap, scen, r)
    assert any(c and s for c, s in zip(tap.cut, tap.sub)), sum(tap.cut)
    if SLICED_KW[row]["fd_ring"]:
        assert p["max_len"] == W and p["max_reports"] > W, p
    else:
        assert p["max_len"] < W, p


@pytest.mark.parametrize("name", ["subring24", "subfront40"])
def test_golden_fixtures_have_sub_phases_and_long_rounds(name):
    scen = load_scenario(name)
    counts = [len(rd["phases"]) for rd in scen["rounds"]]
    assert all(len(ph) > 0 for rd in scen["rounds"] for ph in rd["phases"])
    assert max(counts) > 9  # more phases than any Workload round (3 x fanout)
    assert any(len(set(rd["ticks"][:-1])) < len(rd["phases"]) for rd in scen["rounds"])  # two phases at one tick
    if name == "subfront40":
        assert max(counts) > MAX_PHASES_PER_ROUND + PLANES and min(counts) <= PLANES, counts
        assert max(rd["ticks"][:-1].count(1) for rd in scen["rounds"]) > PLANES  # > GS_PLANES sub-phases at a tick
    else:
        # its rounds span at most 19 ticks, so a pair's reports within a round are kept (<= 16 ticks apart) and those
        # of successive rounds dropped (max_interval 0.25 s); the windows roll over
        p = profile(scen)
        assert p["max_len"] == scen["config"]["window"] < p["max_reports"] and p["near"] > 0, p


def test_chunk_phases_keeps_every_exchange_in_order():
    spec = WorkloadSpec(n=50, k=2, fanout=2, seed=1, init="warm", down_frac=0.2, down_rounds=2)
    scen = make_scenario("chunk", spec, 6)
    before = [[pair for ph in rd["phases"] for pair in ph] for rd in scen["rounds"]]
    chunk_phases(scen, (1, 4, 32))
    for r, rd in enumerate(scen["rounds"]):
        assert [pair for ph in rd["phases"] for pair in ph] == before[r]
        size = (1, 4, 32)[r % 3]
        assert all(0 < len(ph) <= size for ph in rd["phases"])
        for ph in rd["phases"]:  # still a matching
            nodes = [x for pair in ph for x in pair]
            assert len(nodes) == len(set(nodes))


def test_tick_maps():
    spec = WorkloadSpec(n=128, k=2, fanout=3, seed=1, init="warm")
    scen = chunk_phases(make_scenario("maps", spec, 1), (1,))
    P = len(scen["rounds"][0]["phases"])
    assert P > 150
    with_ticks(scen, "budget")  # today's phase_tick / liveness_tick
    assert round_ticks(scen, 0) == [phase_tick(0, p) for p in range(P)] + [liveness_tick(0, P)]
    t = with_ticks(scen, "triples")["rounds"][0]["ticks"]
    assert t[:7] == [1, 1, 1, 2, 2, 2, 3] and t[-1] == t[-2] + 1
    t = with_ticks(scen, "front")["rounds"][0]["ticks"]
    assert t[:41] == [1] * 41 and t[41:44] == [2, 3, 4] and max(t) == 63 and t[-2] == 62


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append(name)


@pytest.mark.parametrize("bad,what", [
    (lambda t: t[:2] + [t[1] - 1] + t[3:], "non-decreasing"),  # a phase before the previous one
    (lambda t: t[:-1] + [64], "within the round"),  # the sweep in the next round's first tick
    (lambda t: [0] + t[1:], "from 1"),  # a phase at the round start's tick
    (lambda t: t[:-1] + [t[-2] - 1], "non-decreasing"),  # the sweep before the last phase
    (lambda t: t[:-1], "offsets for"),  # one offset short
])
def test_replay_round_refuses_invalid_ticks(bad, what):
    spec = WorkloadSpec(n=16, k=2, fanout=2, seed=1, init="warm")
    scen = make_scenario("bad", spec, 1)
    rd = scen["rounds"][0]
    rd["ticks"] = bad([2 + p for p in range(len(rd["phases"]))] + [40])
    rec = Recorder()
    with pytest.raises(ValueError, match=what):
        replay_round(rec, scen, 0)
    assert rec.calls == []  # refused before the backend saw anything of the round

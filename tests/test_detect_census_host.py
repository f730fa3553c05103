"""gs_detect_census on the host (CPU): struct layout, constants, argument checks, DownClock, roc, and the numpy
reference the GPU tests compare the device with (tests/detectref.py).

The argument checks come before any HIP call, so a handle from gs_create alone (nothing bound, nothing booted) is
enough, as in tests/test_view_census_host.py.  The reference is checked against hand-computed values, and run over
the real reference's fixtures to show that every field the GPU test compares is exercised by them.
"""

import ctypes as C
import re

import numpy as np
import pytest
from detectref import BUCKETS, bucket, detect_reference
from helpers import load_scenario

from aiocluster_amd import _lib
from aiocluster_amd.detect import DownClock, detect_rates, roc
from aiocluster_amd.scenario import round_ticks
from aiocluster_amd.workload import round_tick

FIXTURES = ["fdgc12", "q9x10", "sched16", "cutw12", "cutgc12"]
# the thresholds swept over the fixtures (the GPU test uses the same): none within 1e-6 relative of a fixture phi
SWEEP = (0.55, 1.05, 2.05, 4.1)


@pytest.fixture()
def handle():
    from aiocluster_amd.scenario import DEFAULT_CFG
    from aiocluster_amd.sim import make_config

    lib = _lib.load()
    h = C.c_void_p()
    cfg = make_config(1000, 16, DEFAULT_CFG, _lib.GS_CANONICAL, 32)
    assert lib.gs_create(C.byref(cfg), C.byref(h)) == 0
    yield lib, h
    lib.gs_destroy(h)


def test_totals_struct_is_120_words():
    T = _lib.GsDetectTotals
    assert C.sizeof(T) == 120 * 8
    assert T.observers.offset == 0 and T.max_false_age.offset == 17 * 8
    assert T.detect_latency_hist.offset == 18 * 8
    assert T.undetected_age_hist.offset == (18 + _lib.GS_DC_BUCKETS) * 8
    assert T.false_age_hist.offset == (18 + 2 * _lib.GS_DC_BUCKETS) * 8
    assert T.up_over.offset == (18 + 3 * _lib.GS_DC_BUCKETS) * 8
    assert T.down_over.offset == (18 + 3 * _lib.GS_DC_BUCKETS + _lib.GS_DC_MAX_THRESHOLDS) * 8
    assert len(_lib.DETECT_TOTAL_FIELDS) == 18


def test_header_and_binding_agree_on_the_constants():
    src = open(_lib.HEADER).read()
    for name, want in (("GS_DC_BUCKETS", _lib.GS_DC_BUCKETS), ("GS_DC_MAX_THRESHOLDS", _lib.GS_DC_MAX_THRESHOLDS),
                       ("GS_API_VERSION", _lib.API_VERSION)):
        m = re.search(rf"^#define {name} (\d+)u?\b", src, re.M)
        assert m and int(m.group(1)) == want, name
    assert (_lib.GS_DC_BUCKETS, _lib.GS_DC_MAX_THRESHOLDS, _lib.API_VERSION) == (20, 16, 23)
    assert "gs_detect_census" in _lib.EXPORTS
    # the header's struct fields, in order, are the binding's
    body = re.search(r"typedef struct gs_detect_totals \{(.*?)\} gs_detect_totals;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\w+\])?\s*[,;]", body)
    assert names == [f[0] for f in _lib.GsDetectTotals._fields_]


def test_argument_errors_return_invalid(handle):
    lib, h = handle
    tot = _lib.GsDetectTotals()
    call, inv = lib.gs_detect_census, _lib.GS_E_INVALID
    up = C.c_void_p(0x1000)  # never dereferenced: every call below fails before any device work

    def thr(*xs):
        return (C.c_double * max(1, len(xs)))(*xs)

    def err():
        return lib.gs_last_error(h)

    assert call(None, up, None, 0, None, 0, None, None, C.byref(tot)) == inv
    assert call(h, None, None, 0, None, 0, None, None, C.byref(tot)) == inv and b"up is NULL" in err()
    assert call(h, up, None, 0, None, 0, None, None, None) == inv and b"out is NULL" in err()
    # n_thresholds > GS_DC_MAX_THRESHOLDS
    assert call(h, up, None, 0, thr(*[1.0] * 17), 17, None, None, C.byref(tot)) == inv and b"17 thresholds" in err()
    # n_thresholds > 0 with thresholds == NULL
    assert call(h, up, None, 0, None, 1, None, None, C.byref(tot)) == inv and b"thresholds is NULL" in err()
    # NaN, negative, and gs_create's bound: DEFAULT_CFG has max_interval 640 ticks > prior 320, so 51.2 x 640 = 2^15
    for bad in (float("nan"), -1.0, -0.0 - 1e-300, float("inf"), 51.2, 1e9):
        assert call(h, up, None, 0, thr(8.0, bad), 2, None, None, C.byref(tot)) == inv, bad
        assert b"threshold 1" in err(), bad
    # tick below gs_latest_tick (0 on a fresh handle: only a wrapped tick is below it), or 2^15 or more past it
    for tick in (1 << 15, (1 << 15) + 7, 1 << 20, 0xFFFFFFFF, 0x80000000):
        assert call(h, up, None, tick, None, 0, None, None, C.byref(tot)) == inv, tick
        assert b"tick" in err() and b"latest tick" in err(), tick
    # valid arguments get as far as the handle's state: still before any device work
    assert call(h, up, None, (1 << 15) - 1, thr(0.0, 51.19), 2, None, None, C.byref(tot)) == inv
    assert b"not booted" in err()
    assert b"gs_detect_census" in err()


def test_down_clock():
    c = DownClock(5)
    # the first update: a down node goes down at that tick
    assert c.update([1, 0, 1, 1, 0], 10).tolist() == [0, 10, 0, 0, 10]
    assert c.down_since.dtype == np.uint32
    # still down: unchanged; node 0 goes down now
    assert c.update([0, 0, 1, 1, 0], 74).tolist() == [74, 10, 0, 0, 10]
    # node 1 returns (its entry is ignored by the census, and kept), node 4 stays down
    assert c.update([0, 1, 1, 1, 0], 138).tolist() == [74, 10, 0, 0, 10]
    # node 1 goes down again: a new tick; node 0 returns
    assert c.update(np.array([1, 0, 1, 1, 0], np.uint8), 202).tolist() == [74, 202, 0, 0, 10]
    with pytest.raises(ValueError):
        c.update([1, 1], 3)


def test_roc_and_rates():
    census = {"up_phi": 200, "down_phi": 40, "up_over": [50, 10, 0], "down_over": [40, 30, 4],
              "up_dead": 3, "up_pairs": 12, "down_dead": 0, "down_pairs": 0, "down_live": 0}
    assert roc(census, [2, 4, 8]) == [(2.0, 0.25, 1.0), (4.0, 0.05, 0.75), (8.0, 0.0, 0.1)]
    with pytest.raises(ValueError):
        roc(census, [2, 4])
    assert detect_rates(census) == {"false_suspicion_rate": 0.25, "detected_fraction": 0.0, "undetected": 0}
    empty = {"up_phi": 0, "down_phi": 0, "up_over": [0], "down_over": [0]}
    assert roc(empty, [1.5]) == [(1.5, 0.0, 0.0)]


def test_buckets():
    assert [bucket(x) for x in (0, 1, 2, 3, 4, 7, 8, (1 << 18) - 1, 1 << 18, 1 << 19, 1 << 30)] == \
        [0, 1, 2, 2, 3, 3, 4, 18, 19, 19, 19]


# a 4-node state by hand, tick 1000: nodes 0, 1, 3 up, node 2 down since 900
#   observer 0: 1 live; 2 dead at 940 (latency 40); 3 dead at 996 (a false suspicion, 4 ticks old)
#   observer 1: 0 live; 2 live (undetected for 100); 3 unknown
#   observer 2 (down: not counted): everything live
#   observer 3: 0 dead at 1000 (false, age 0); 1 live; 2 dead at 890 (before it went down: an early death)
HAND = [
    {"live": [1], "dead": [[2, 940], [3, 996]],
     "windows": [[1, 990, 4, 4.0, 0.5], [2, 880, 3, 3.0, 7.0], [3, 960, 0, 0.0, None]]},
    {"live": [0, 2], "dead": [], "windows": [[0, 995, 2, 2.0, 0.25], [2, 890, 2, 2.0, 3.5]]},
    {"live": [0, 1, 3], "dead": [], "windows": [[0, 800, 2, 2.0, 9.0]]},
    {"live": [1], "dead": [[0, 1000], [2, 890]], "windows": [[0, 900, 5, 5.0, 2.5], [1, 999, 1, 1.0, 0.01], [2, 850, 1, 1.0, 6.0]]},
]


def test_reference_on_a_hand_computed_state():
    up = [1, 1, 0, 1]
    ds = [0, 0, 900, 0]
    got = detect_reference(HAND, up, ds, 1000, (1.0, 3.0, 6.5))
    want = dict(observers=3, up_pairs=6, up_live=3, up_dead=2, up_unknown=1, down_pairs=3, down_live=1, down_dead=2,
                down_unknown=0, up_windows=5, down_windows=3, up_phi=4, down_phi=3, old_windows=0, early_deaths=1,
                max_detect_latency=40, max_undetected_age=100, max_false_age=4)
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)
    h = [0] * BUCKETS
    h[6] = 1  # 40: 32 <= x < 64
    assert got["detect_latency_hist"] == h
    h = [0] * BUCKETS
    h[7] = 1  # 100: 64 <= x < 128
    assert got["undetected_age_hist"] == h
    h = [0] * BUCKETS
    h[0], h[3] = 1, 1  # 0 and 4
    assert got["false_age_hist"] == h
    # up pairs with a phi: (0,1) 0.5, (1,0) 0.25, (3,0) 2.5, (3,1) 0.01; down: (0,2) 7.0, (1,2) 3.5, (3,2) 6.0
    assert got["up_over"] == [1, 0, 0] and got["down_over"] == [3, 3, 1]
    assert got["target_live_by"].tolist() == [1, 2, 1, 0]
    assert got["target_dead_by"].tolist() == [1, 0, 2, 1]
    assert got["target_first_tod"].tolist() == [1000, -1, 890, 996]
    assert got["target_last_tod"].tolist() == [1000, -1, 940, 996]
    assert got["row_false_suspicions"].tolist() == [1, 0, 0, 1]
    assert got["row_undetected"].tolist() == [0, 1, 0, 0]
    assert (got["false_suspicion_rate"], got["detected_fraction"], got["undetected"]) == (2 / 6, 2 / 3, 1)
    # without down_since and without thresholds: those fields are zero, the rest unchanged
    bare = detect_reference(HAND, up, None, 1000)
    for k in ("early_deaths", "max_detect_latency", "max_undetected_age", "up_windows", "down_windows", "up_phi",
              "down_phi", "old_windows"):
        assert bare[k] == 0, k
    assert sum(bare["detect_latency_hist"]) == 0 and sum(bare["undetected_age_hist"]) == 0
    assert bare["false_age_hist"] == got["false_age_hist"] and bare["up_dead"] == 2 and bare["up_over"] == []


def test_reference_on_an_export_computes_phi():
    """The same pairs as an export: phi from (last, len, sum) with SamplingWindow.phi's expression; a window silent
    for 2^15 ticks or more is old, and above every valid threshold."""
    n, tick, prior5 = 3, 40000, 5.0
    ex = {"live": np.array([[0, 1, 1], [1, 0, 0], [1, 1, 0]]), "tod": np.array([[-1, -1, -1], [-1, -1, 39000], [-1, -1, -1]]),
          "fd_last": np.array([[-1, 39936, 100], [39990, -1, 38000], [-1, 39999, -1]]),
          "fd_len": np.array([[0, 3, 2], [0, 0, 4], [0, 1, 0]]), "fd_sum": np.array([[0.0, 3.0, 2.0], [0.0, 0.0, 8.0], [0.0, 1.0, 0.0]])}
    got = detect_reference(ex, [1, 1, 1], [0, 0, 0], tick, (0.5, 1.5, 50.0), prior5=prior5)
    # (0,1): age 64 ticks = 1 s, mean (3 + 5) / 8 = 1: phi 1.0;  (0,2): old: 2^15 ticks = 512 s, mean 1: phi 512
    # (1,0): len 0: no phi;  (1,2): 2000 ticks = 31.25 s, mean 13 / 9;  (2,1): 1 tick, mean 1: phi 1 / 64
    assert (got["up_windows"], got["up_phi"], got["old_windows"]) == (5, 4, 1)
    assert got["up_over"] == [3, 2, 1]
    assert (got["up_dead"], got["max_false_age"]) == (1, 1000)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_exercise_every_compared_field(name):
    """Non-vacuity of the GPU test's first case: over the fixture's rounds the reference sees false suspicions,
    detections, undetected failures, all three histograms, and threshold counts strictly inside their range."""
    scen = load_scenario(name)
    n = scen["n"]
    clock = DownClock(n)
    seen = dict.fromkeys(("up_dead", "down_dead", "down_live", "detect_latency_hist", "undetected_age_hist",
                          "false_age_hist", "up_over_inside", "down_over_inside"), False)
    for r, rd in enumerate(scen["rounds"]):
        ds = clock.update(rd["up"], round_tick(r))
        states = scen["expect"]["states"][r]
        for s in states:
            for w in s["windows"]:
                if w[4] is not None:
                    for t in SWEEP:
                        assert abs(w[4] - t) > 1e-6 * t, (name, r, w, t)
        c = detect_reference(states, rd["up"], ds, round_ticks(scen, r)[-1], SWEEP)
        for k in ("up_dead", "down_dead", "down_live"):
            seen[k] |= c[k] > 0
        for k in ("detect_latency_hist", "undetected_age_hist", "false_age_hist"):
            seen[k] |= sum(c[k]) > 0
        seen["up_over_inside"] |= any(0 < x < c["up_phi"] for x in c["up_over"])
        seen["down_over_inside"] |= any(0 < x < c["down_phi"] for x in c["down_over"])
    assert all(seen.values()), (name, seen)

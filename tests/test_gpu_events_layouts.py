"""Hook events (gs_set_events) in every layout, against the C oracle (GPU only).

While events are on, a phase runs neither the speculative pass-1 merge nor k_lite nor the heavy-slot kernel nor the
version-log evaluation, and every prefix view takes apply_cand's per-key path: a combination of kernels that no
other test runs.  The scenarios of tests/manyphases.py (128 nodes, k = 8, 9 rounds: a binding mtu, candidate
records, mid-round plane replays, sub-phases, churn) and of tests/eventcases.py (64 keys; 37 keys in canonical
prefix views; 16 keys with escape slots) are replayed in lockstep with the oracle, whose event order
tests/test_events.py pins to the reference's (sub-phases included): after every round the drained events must equal the oracle's as lists, in exact order, and
the whole export must be equal; at the end the counters.  Further cases turn events on and off between rounds,
suppress the heavy-slot hand-off, and fill the record buffer past its capacity (a documented, bounds-checked drop).
"""

import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from eventcases import COLD_K64_KW, WARM_K16_ESC_KW, WARM_K37_KW, cold_k64, warm_k16_esc, warm_k37
from helpers import compare_exports, make_backend
from manyphases import LAYOUTS, RING_ROWS, device_scenario
from oracle import OracleSim
from test_gpu_subphases import NON_FD, Flushing, assert_counters

from aiocluster_amd._lib import GsError
from aiocluster_amd.scenario import make_scenario, replay_round, round_ticks
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.workload import WorkloadSpec

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

CASES = [(layout, kind) for layout in LAYOUTS for kind in ("budget", "triples")] + [("general", "front"),
                                                                                   ("hb8mv8", "front")]


def layout_kw(layout):
    kw = dict(LAYOUTS[layout][2])
    if layout == "sampled":
        kw["ring_rows"] = RING_ROWS
    return kw


def export_diff(gpu, orc, sampled=False):
    got, want = gpu.export(), orc.export()
    if not sampled:
        return compare_exports(got, want)
    # the sampled-ring contract (test_gpu_subphases.test_one_handle_matches_oracle): the ring rows are exact,
    # windows included; the other rows are compared on everything but the windows
    ring = list(RING_ROWS)
    diff = compare_exports({k: v[ring] for k, v in got.items()}, {k: v[ring] for k, v in want.items()})
    return diff or compare_exports({k: (got[k] if k in NON_FD else v) for k, v in want.items()}, want)


def assert_same_events(got, want, what):
    got, want = got.astype(np.int64).tolist(), want.astype(np.int64).tolist()
    if got != want:
        i = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} device events vs {len(want)}; first difference at {i}: "
                             f"{got[i:i + 3]} vs {want[i:i + 3]}")
    return want


def exact_under_sampled_rings(ev):
    """The events that stay exact once a compact row's window has saturated (the sampled-ring contract, see
    export_diff): every on_key_change, and the joins and leaves that the ring rows observe.  The other rows' live
    sets come from windows that are inexact from then on, as their ``live`` / ``tod`` / ``fd_*`` fields are."""
    return ev[((ev[:, 2] >> 8) == 0) | np.isin(ev[:, 0], RING_ROWS)]


def lockstep(scen, kw, sampled=False, what=""):
    """Both backends with events on from round 0; returns (device counters, the events of every round).  With
    ``sampled`` the whole lists are compared until the first compact window saturates (fd_saturated > 0), from
    then on exact_under_sampled_rings of them, still in exact order."""
    gpu = make_backend(GossipSim, scen, **kw)
    orc = make_backend(OracleSim, scen)
    gpu.enable_events()
    orc.enable_events()
    events, kinds, saturated_rounds = [], set(), 0
    for r in range(len(scen["rounds"])):
        replay_round(gpu, scen, r)
        replay_round(orc, scen, r)
        got, want = gpu.drain_events(), orc.drain_events()
        if sampled and gpu.counters()["fd_saturated"]:
            got, want = exact_under_sampled_rings(got), exact_under_sampled_rings(want)
            saturated_rounds += 1
        ev = assert_same_events(got, want, f"{what} round {r}")
        diff = export_diff(gpu, orc, sampled)
        assert diff is None, f"{what} round {r}: device vs oracle: {diff}"
        events.append(ev)
        kinds |= {e[2] >> 8 for e in ev}
    c = gpu.check(accept_saturated=sampled)
    assert_counters(c, orc)  # STAT_KEYS, truncated > 0
    assert c["lite_slots"] == 0 and c["heavy_slots"] == 0, (c["lite_slots"], c["heavy_slots"])  # the event path ran
    assert kinds == {0, 1, 2}, kinds
    if sampled:  # both regimes occurred: whole lists first, the exact part after the first saturation
        assert 0 < saturated_rounds < len(events), saturated_rounds
    per_round = [len(ev) for ev in events]
    print(f"{what}: events per round {per_round} (total {sum(per_round)}), plane flushes {c['plane_flushes']}, "
          f"truncated {c['truncated']}")
    gpu.close()
    orc.close()
    return c, events


@pytest.mark.parametrize("layout,kind", CASES)
def test_events_match_oracle_in_every_layout(layout, kind):
    scen = device_scenario(layout, kind)
    c, _ = lockstep(scen, layout_kw(layout), sampled=layout == "sampled", what=f"{layout}/{kind}")
    assert c["plane_flushes"] > 0  # mid-round replays happened while events were on


# ---------------------------------------------------------------- events turned on and off between rounds
@pytest.mark.parametrize("flushing", [False, True], ids=["plain", "flush_reports"])
def test_events_toggled_between_rounds(flushing):
    """Events on in the odd rounds only: spec and lite are decided per phase, so a round of the fast paths (records
    written under the speculative merge, k_lite) is followed directly by an event-path round and the other way
    round.  With ``flushing`` the device also replays its reports mid-round (gs_flush_reports), which must emit no
    join or leave by itself."""
    scen = device_scenario("hb8mv8", "budget")
    gpu = make_backend(GossipSim, scen, **layout_kw("hb8mv8"))
    orc = make_backend(OracleSim, scen)
    orc.enable_events()
    drv = Flushing(gpu, after=(3, 40)) if flushing else gpu
    compared = 0
    for r in range(len(scen["rounds"])):
        if r & 1:
            gpu.enable_events()
        if flushing:
            drv.next_ticks = round_ticks(scen, r)
        replay_round(drv, scen, r)
        replay_round(orc, scen, r)
        want = orc.drain_events()
        if r & 1:
            compared += len(assert_same_events(gpu.drain_events(), want, f"round {r}"))
            gpu.disable_events()
        diff = export_diff(gpu, orc)
        assert diff is None, f"round {r}: device vs oracle: {diff}"
    c = gpu.check()
    assert_counters(c, orc)
    assert compared > 0 and c["lite_slots"] > 0, (compared, c["lite_slots"])  # the fast paths came back
    if flushing:
        assert drv.flushes >= len(scen["rounds"])
    print(f"toggled ({'flush_reports' if flushing else 'plain'}): {compared} events compared, lite slots "
          f"{c['lite_slots']}, plane flushes {c['plane_flushes']}, truncated {c['truncated']}")
    gpu.close()
    orc.close()


# ---------------------------------------------------------------- key-index and view-width edges
def test_events_with_64_keys_general_layout():
    """Keys 32..63 in the records' key word (key | kind << 8), deletes and TTL writes, cold start."""
    _, events = lockstep(cold_k64(), COLD_K64_KW, what="cold k64")
    ev = np.asarray([e for per_round in events for e in per_round], dtype=np.int64)
    applied = ev[((ev[:, 2] >> 8) == 0) & (ev[:, 0] != ev[:, 1])]  # apply_delta's records, as the device wrote them
    assert ((applied[:, 2] & 0xFF) >= 32).sum() > 100 and (applied[:, 2] & 0xFF).max() == 63


def test_events_with_37_keys_canonical_prefix():
    """37 keys in canonical prefix views (the KWB kernels with 10 of 16 key words in use): apply_cand's per-key path
    reports keys up to index 36 and none past it."""
    _, events = lockstep(warm_k37(), WARM_K37_KW, what="warm k37")
    ev = np.asarray([e for per_round in events for e in per_round], dtype=np.int64)
    applied = ev[((ev[:, 2] >> 8) == 0) & (ev[:, 0] != ev[:, 1])]
    assert ((applied[:, 2] & 0xFF) >= 32).any() and (applied[:, 2] & 0xFF).max() == 36


def test_events_with_16_keys_hb8mv8_escape_slots():
    lockstep(warm_k16_esc(), WARM_K16_ESC_KW, what="warm k16 esc4")


# ---------------------------------------------------------------- the heavy-slot hand-off is suppressed
def heavy_run():
    """test_gpu_heavy.py's scenario at n = 768 (K = 16, mtu 1200, 16-bit views) for 4 rounds with events on; run in
    a child process with GS_HEAVY_T=48 (read once per process).  A second handle without events runs beside it: it
    hands slots to the heavy kernel, the handle with events must not."""
    n, rounds = 768, 4
    spec = WorkloadSpec(n=n, k=16, fanout=3, seed=n, init="warm", write_frac=0.3, down_frac=0.1, down_rounds=3)
    scen = make_scenario("heavy%d" % n, spec, rounds, {"mtu": 1200})
    orc = make_backend(OracleSim, scen)
    orc.enable_events()
    want, exports = [], []
    for r in range(rounds):
        replay_round(orc, scen, r)
        want.append(orc.drain_events())
        exports.append(orc.export())
    kw = dict(tombstones=False, fd_ring=False, hb8=False, mv8=False)
    gpu = make_backend(GossipSim, scen, **kw)
    ctl = make_backend(GossipSim, scen, **kw)
    gpu.enable_events(capacity=max(len(w) for w in want))
    for r in range(rounds):
        replay_round(gpu, scen, r)
        replay_round(ctl, scen, r)
        assert_same_events(gpu.drain_events(), want[r], f"round {r}")
        for name, sim in (("events", gpu), ("control", ctl)):
            diff = compare_exports(sim.export(), exports[r])
            assert diff is None, f"round {r}: {name} handle vs oracle: {diff}"
    c, cc, s = gpu.check(), ctl.check(), orc.stats()
    for k in ("node_deltas", "truncated", "delta_bytes"):
        assert c[k] == s[k] == cc[k], (k, c[k], s[k], cc[k])
    print("ok heavy_slots %d control_heavy_slots %d truncated %d events %d"
          % (c["heavy_slots"], cc["heavy_slots"], c["truncated"], sum(len(w) for w in want)))


def test_events_suppress_the_heavy_hand_off():
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "from test_gpu_events_layouts import heavy_run\n"
            "heavy_run()\n") % (HERE, REPO, os.path.join(REPO, "oracle"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GS_HEAVY_T="48"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("ok"), line
    print(line)
    st = dict(zip(line.split()[1::2], (int(x) for x in line.split()[2::2])))
    assert st["heavy_slots"] == 0 and st["truncated"] > 0, st
    assert st["control_heavy_slots"] > 0, st  # without events the same rounds do hand slots over


# ---------------------------------------------------------------- records past the capacity are dropped but counted
CANARY = 0x5A5A5A5A


def test_event_buffer_overflow_is_dropped_and_counted():
    import torch

    cap = 64
    scen = device_scenario("hb8mv8", "budget")
    rounds = len(scen["rounds"])
    orc = make_backend(OracleSim, scen)
    orc.enable_events()
    want, exports = [], []
    for r in range(rounds):
        replay_round(orc, scen, r)
        want.append(orc.drain_events().astype(np.int64))
        exports.append(orc.export())
    R = int(np.argmax([len(w) for w in want]))
    m = len(want[R])
    assert m > cap and R + 2 < rounds and len(want[R + 1]) > cap, (R, m)

    gpu = make_backend(GossipSim, scen, **layout_kw("hb8mv8"))
    for r in range(R):
        replay_round(gpu, scen, r)
    # a buffer of m records, of which the library may use the first 64
    buf = torch.full((m, 8), CANARY, dtype=torch.int32, device=gpu.device)
    count = torch.zeros(1, dtype=torch.int32, device=gpu.device)
    gpu._chk(gpu.L.gs_set_events(gpu.h, C.c_void_p(buf.data_ptr()), cap, C.c_void_p(count.data_ptr())),
             "gs_set_events")
    replay_round(gpu, scen, R)
    gpu.sync()
    assert int(count.item()) == m, (int(count.item()), m)
    rec = buf.cpu().numpy().view(np.uint32).astype(np.int64)
    assert (rec[cap:] == CANARY).all(), "a record past the capacity was written"
    have = collections.Counter(map(tuple, want[R].tolist()))
    kept = collections.Counter(map(tuple, rec[:cap, :6].tolist()))
    assert sum(kept.values()) == cap and not kept - have, list((kept - have).items())[:4]
    gpu.disable_events()
    diff = compare_exports(gpu.export(), exports[R])
    assert diff is None, f"round {R}: {diff}"

    gpu.enable_events(capacity=cap)  # the Python wrapper: the overflow is an error, and the next drain starts clean
    replay_round(gpu, scen, R + 1)
    with pytest.raises(GsError, match="event buffer overflow"):
        gpu.drain_events()
    diff = compare_exports(gpu.export(), exports[R + 1])
    assert diff is None, f"round {R + 1}: {diff}"
    gpu.enable_events()
    replay_round(gpu, scen, R + 2)
    assert_same_events(gpu.drain_events(), want[R + 2], f"round {R + 2}")
    diff = compare_exports(gpu.export(), exports[R + 2])
    assert diff is None, f"round {R + 2}: {diff}"
    gpu.check()
    gpu.close()
    orc.close()

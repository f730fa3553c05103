"""gs_traffic_census on the device (GPU only).

1. the real reference's framed fixtures (tools/gen_traffic_fixture.py): every recorded size, every outcome, the
   state after every round, in every layout that can replay them;
2. against tests/trafficref.py over the C oracle's export, mid-round, at the sizes where k_traffic can still go
   wrong: a second and a third streaming step, a partial last group, both key widths, owners unknown to one side,
   mtus that truncate;
3. against the wire emitter's byte counts;
4. read-only: no state region, no counter changes; a second call repeats the first; ``nodes`` is added to;
5. escaped columns and lagging rows with heartbeats past 2^8;
6. refusals and invalid exchanges;
7. WorkloadSpec(frame_limit=True) through driver.run_round.
"""

import ctypes as C

import numpy as np
import pytest
import torch
from helpers import compare_exports, first_diff, load_scenario, make_backend
from oracle import OracleSim
from test_gpu_lossy import LAYOUTS_W, PREFIX, SCRATCH, state_regions
from trafficref import TrafficRef, for_backend

from aiocluster_amd import _lib
from aiocluster_amd._lib import GsError
from aiocluster_amd.pbsize import nodeid_size
from aiocluster_amd.scenario import DEFAULT_CFG, make_scenario, replay_round, round_tick, round_ticks, state_hash
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.wire import WireEmitter, packet_size
from aiocluster_amd.workload import WorkloadSpec, key_names, synthetic_node_ids

pytestmark = pytest.mark.gpu

TOTAL_KEYS = ("exchanges", "bad_index", "sent", "delivered", "lost", "rejected", "bytes_sent", "bytes_delivered",
              "digest_bytes_sent", "delta_bytes_sent", "delta_bytes_delivered", "max_frame", "frame_hist", "digest_share")


def census(gpu, t, pairs, legs=None, frame_limit=False):
    """One blocking census with every output; numpy / dict results."""
    nodes = torch.zeros((2, gpu.n), dtype=torch.int64, device=gpu.device)
    out = gpu.traffic_census(t, pairs, legs=legs, frame_limit=frame_limit, per_exchange=True, nodes=nodes)
    return {"msg": out["msg"].cpu().numpy().tolist(), "legs_out": out["legs_out"].cpu().numpy().tolist(),
            "nodes": nodes.cpu().numpy(), "totals": {k: out[k] for k in TOTAL_KEYS}}


def assert_census(got, want, what):
    assert got["msg"] == want["msg"], f"{what}: msg {first_row_diff(got['msg'], want['msg'])}"
    assert got["legs_out"] == want["legs_out"], f"{what}: legs_out"
    assert np.array_equal(got["nodes"], want["nodes"]), f"{what}: nodes"
    for k in TOTAL_KEYS:
        assert got["totals"][k] == want["totals"][k], f"{what}: totals.{k}: {got['totals'][k]} != {want['totals'][k]}"


def first_row_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"exchange {i}: device {x} != reference {y}"
    return f"lengths {len(a)} != {len(b)}"


# ---------------------------------------------------------------- 1. the reference's framed fixtures
def replay_framed(name, **kw):
    """Before each phase the census (frame limit on, the fixture's network legs): ``legs_out`` and every recorded
    size and packet are the reference's; the phase then runs with the device's own ``legs_out``; the state after
    every round is the reference's."""
    scen = load_scenario(name)
    exp = scen["expect"]
    gpu = make_backend(GossipSim, scen, **kw)
    delivered, outcomes = 0, [0, 0, 0, 0]
    for r, rd in enumerate(scen["rounds"]):
        t, ticks = round_tick(r), round_ticks(scen, r)
        for j, k, op, v in rd["writes"]:
            gpu.write(t, j, k, op, v)
        gpu.begin_round(t, rd["up"])
        for p, ph in enumerate(rd["phases"]):
            if not ph:
                continue
            net = rd["net_legs"][p] if "net_legs" in rd else None
            out = gpu.traffic_census(ticks[p], ph, legs=net, frame_limit=True, per_exchange=True)
            lo, msg = out["legs_out"].cpu().numpy().tolist(), out["msg"].cpu().numpy().tolist()
            assert lo == rd["legs"][p], (r, p, lo, rd["legs"][p])
            for e, rec in enumerate(rd["traffic"][p]):
                m = msg[e]
                assert all(m[i] == rec[i] for i in range(4) if rec[i] is not None), (r, p, e, m, rec)
                pk = [packet_size("syn", digest_len=m[0]), packet_size("synack", digest_len=m[1], delta_len=m[2]),
                      packet_size("ack", delta_len=m[3])]
                assert all(pk[i] == rec[4 + i] for i in range(3) if rec[4 + i] is not None), (r, p, e, pk, rec)
                outcomes[lo[e]] += 1
            delivered += out["delta_bytes_delivered"]
            gpu.run_phase(ticks[p], ph, out["legs_out"])
        gpu.liveness(ticks[-1], rd["up"], r)
        st = gpu.state()
        assert state_hash(st) == exp["hashes"][r], f"{name} round {r}: {first_diff(st, exp['states'][r])}"
    c = gpu.check()
    assert c["delta_bytes"] == delivered and c["exchanges"] == sum(outcomes)
    assert c["cut_exchanges"] == sum(outcomes[:3]) > 0
    print(f"{name} {kw}: outcomes {outcomes}, delta bytes {delivered}, truncated {c['truncated']}")
    gpu.close()
    return outcomes


def test_reference_frame10_general_layout_with_rings():
    """Cold, deletes, TTL writes, failure-detector GC, window 5: the frame limit alone cuts the exchanges."""
    outcomes = replay_framed("frame10", fd_ring=True)
    assert sum(1 for x in outcomes if x) >= 2


@pytest.mark.parametrize("layout", list(LAYOUTS_W))
def test_reference_framew12s(layout):
    """Warm, 13 keys: every layout; the frame limit on top of a network that loses a quarter of the messages."""
    outcomes = replay_framed("framew12s", **LAYOUTS_W[layout])
    assert min(outcomes) >= 10


# ---------------------------------------------------------------- 2. against trafficref over the oracle, mid-round
def midround_case(n, k, init, mtu, seed, rounds_before=1, extra_cfg=None, write_frac=0.3, **spec_kw):
    """The scenario, and the oracle's view of it stopped after phase 0 of round ``rounds_before``: the census pairs
    (the first 32 of phase 1 and one pair that reuses two of their nodes: census pairs need not be conflict-free),
    their legs, and trafficref's results over the oracle's export of the rows involved."""
    spec = WorkloadSpec(n=n, k=k, fanout=3, seed=seed, init=init, write_frac=write_frac, **spec_kw)
    scen = make_scenario(f"tc{n}k{k}", spec, rounds_before + 1, dict({"mtu": mtu}, **(extra_cfg or {})))
    orc = make_backend(OracleSim, scen, threads=8)
    t, pairs = advance(orc, scen, rounds_before)
    rows = sorted({x for p in pairs for x in p})
    ex = orc.export_rows(rows)
    ex["rows"] = rows
    ref = for_backend(orc, scen)
    legs = [int(x) for x in np.random.default_rng(seed).integers(0, 4, len(pairs))]
    want = {
        "plain": ref.phase(ex, pairs, t),
        "legs": ref.phase(ex, pairs, t, legs=legs),
        "limit": ref.phase(ex, pairs, t, legs=legs, frame_limit=True),
    }
    orc.close()
    return scen, rounds_before, t, pairs, legs, want


def advance(backend, scen, rounds_before):
    """Replay ``rounds_before`` rounds, then the next round's writes, round start and phase 0.  Returns the tick of
    phase 1 and the census pairs."""
    for r in range(rounds_before):
        replay_round(backend, scen, r)
    rd = scen["rounds"][rounds_before]
    t = round_tick(rounds_before)
    ticks = round_ticks(scen, rounds_before)
    for j, kk, op, v in rd["writes"]:
        backend.write(t, j, kk, op, v)
    backend.begin_round(t, rd["up"])
    backend.run_phase(ticks[0], rd["phases"][0])
    ph = [tuple(p) for p in rd["phases"][1][:32]]
    pairs = ph + [(ph[0][0], ph[-1][1])]
    return ticks[1], pairs


def run_midround(case, **kw):
    scen, rb, t, pairs, legs, want = case
    gpu = make_backend(GossipSim, scen, **kw)
    t2, pairs2 = advance(gpu, scen, rb)
    assert (t2, pairs2) == (t, pairs)
    assert_census(census(gpu, t, pairs), want["plain"], "all delivered")
    assert_census(census(gpu, t, pairs, legs=legs), want["legs"], "network legs")
    assert_census(census(gpu, t, pairs, legs=legs, frame_limit=True), want["limit"], "frame limit")
    gpu.check()
    gpu.close()
    return want


@pytest.fixture(scope="module")
def warm1100():
    return midround_case(1100, 4, "warm", 1500, seed=41)


@pytest.mark.parametrize("layout", list(LAYOUTS_W))
def test_midround_warm_1100(warm1100, layout):
    """N = 1,100: a second 1,024-column step (a third of 512 columns at 16-bit views), a partial last group
    (1,100 mod 16 = 12); mtu 1,500 truncates."""
    want = run_midround(warm1100, **LAYOUTS_W[layout])
    m = np.asarray(want["plain"]["msg"])
    assert (m[:, 2:] > 0).any() and m[:, 2:].max() <= 1500
    assert want["limit"]["totals"]["rejected"][0] > 0  # a 1,100-entry digest is far past the mtu


@pytest.fixture(scope="module")
def warm2100():
    return midround_case(2100, 4, "warm", 1100, seed=43)


@pytest.mark.parametrize("layout", ["prefix", "hb8", "hb8mv8_esc4"])
def test_midround_warm_2100(warm2100, layout):
    """N = 2,100: three 1,024-column steps, so both prefetch buffers are reused."""
    run_midround(warm2100, **LAYOUTS_W[layout])


@pytest.fixture(scope="module")
def wide1100():
    return midround_case(1100, 21, "warm", 900, seed=47)


@pytest.mark.parametrize("layout", ["general", "canonical_held", "prefix"])
def test_midround_wide_keys_1100(wide1100, layout):
    """K = 21: the wide-key instantiation (the 8-bit layouts stop at 16 keys)."""
    run_midround(wide1100, **LAYOUTS_W[layout])


@pytest.fixture(scope="module")
def cold96():
    return midround_case(96, 5, "cold", 400, seed=53, rounds_before=2, extra_cfg={"tombstone_grace_s": 3, "window": 1000},
                         delete_frac=0.15, ttl_frac=0.1)


def test_midround_cold_96_general(cold96):
    """Cold start, round 2: some owners are still unknown to one side of an exchange, so they enter the SynAck
    digest mid-exchange; deletes and TTL writes; mtu 400."""
    want = run_midround(cold96)
    scen, rb, t, pairs, _, _ = cold96
    m = np.asarray(want["plain"]["msg"])
    assert (m[:, 1] > m[:, 0]).any()  # a SynAck digest longer than the Syn's: owners entered it


@pytest.fixture(scope="module")
def small40():
    return midround_case(40, 4, "warm", 1500, seed=59, rounds_before=6, write_frac=0.6, down_frac=0.3, down_rounds=3)


@pytest.mark.parametrize("layout", list(LAYOUTS_W))
def test_midround_small_40_mixed_outcomes(small40, layout):
    """40 nodes, some back from an absence: a digest (1,380 bytes) fits the mtu, a SynAck that adds a delta to it
    often does not, so the frame limit itself cuts exchanges, beside the network's legs."""
    want = run_midround(small40, **LAYOUTS_W[layout])
    assert want["limit"]["totals"]["rejected"][1] > 0 and len(set(want["limit"]["legs_out"])) >= 3


# ---------------------------------------------------------------- 3. the emitter's byte counts
@pytest.mark.parametrize("layout,n,init", [("hb8mv8_esc4", 200, "warm"), ("general", 96, "cold")])
def test_sizes_equal_the_emitters(layout, n, init):
    kw = {"delete_frac": 0.15, "ttl_frac": 0.1} if init == "cold" else {}
    cfg = {"mtu": 500, "tombstone_grace_s": 3} if init == "cold" else {"mtu": 500}
    spec = WorkloadSpec(n=n, k=4, fanout=3, seed=61, init=init, write_frac=0.3, **kw)
    scen = make_scenario(f"em{n}", spec, 3, cfg)
    gpu = make_backend(GossipSim, scen, **(LAYOUTS_W[layout] if init == "warm" else {}))
    t, pairs = advance(gpu, scen, 2)
    pairs = pairs[:32]
    got = census(gpu, t, pairs)
    em = WireEmitter(gpu)
    for e, (a, b) in enumerate(pairs):
        assert got["msg"][e][0] == len(em.digest(a, t)), (e, "syn digest")
        assert got["msg"][e][2] == len(em.delta(b, a, t)), (e, "synack delta")
        assert got["msg"][e][3] == len(em.delta(a, b, t)), (e, "ack delta")
    assert max(m[2] for m in got["msg"]) > 0
    gpu.close()


# ---------------------------------------------------------------- 4. read-only
@pytest.mark.parametrize("layout", ["general", "prefix", "hb8mv8_esc4"])
def test_census_changes_nothing(layout):
    spec = WorkloadSpec(n=200, k=4, fanout=3, seed=67, init="warm", write_frac=0.3)
    scen = make_scenario("ro200", spec, 2, {"mtu": 700})
    gpu = make_backend(GossipSim, scen, **LAYOUTS_W[layout])
    t, pairs = advance(gpu, scen, 1)
    before, cb = state_regions(gpu), gpu.counters()
    legs = [e % 4 for e in range(len(pairs))]
    nodes = torch.zeros((2, gpu.n), dtype=torch.int64, device=gpu.device)
    one = gpu.traffic_census(t, pairs, legs=legs, frame_limit=True, per_exchange=True, nodes=nodes)
    n1 = nodes.clone()
    two = gpu.traffic_census(t, pairs, legs=legs, frame_limit=True, per_exchange=True, nodes=nodes)
    after, ca = state_regions(gpu), gpu.counters()
    assert before.keys() == after.keys() and not (set(before) & SCRATCH)
    for name in before:
        assert before[name] == after[name], f"region {name} changed"
    assert ca == cb
    assert torch.equal(one["msg"], two["msg"]) and torch.equal(one["legs_out"], two["legs_out"])
    for k in TOTAL_KEYS:
        assert one[k] == two[k], k
    assert int(n1.sum()) > 0 and torch.equal(nodes, 2 * n1)  # added to, not overwritten
    assert int(n1[0].sum()) == sum(one["bytes_sent"]) and int(n1[1].sum()) == sum(one["bytes_delivered"])
    # the asynchronous form (no totals) gives the same device outputs
    three = gpu.traffic_census(t, pairs, legs=legs, frame_limit=True, per_exchange=True, totals=False)
    assert set(three) == {"legs_out", "msg"} and torch.equal(three["msg"], one["msg"])
    assert torch.equal(three["legs_out"], one["legs_out"])
    gpu.close()


# ---------------------------------------------------------------- 5. escaped columns and lagging rows
def test_escaped_column_and_lagging_rows():
    """40 nodes, one round of 300 phases in which node 1 answers every phase and nodes 6 .. 39 take part in none:
    node 1's heartbeat passes 2^8, the idle rows' views of it lag by more than a byte holds, and the lag sweep moves
    column 1 to 16-bit escape slots.  The digests are sized on the decoded heartbeats."""
    n = 40
    ids, keys = synthetic_node_ids(n), key_names(2)
    init = {j: [(0, f"v{j}")] for j in range(n)}
    gpu = GossipSim(ids, keys, dict(DEFAULT_CFG), "warm", init, tombstones=False, fd_ring=False, hist_cap=8, hb8=True,
                    mv8=True, esc_cols=4)
    orc = OracleSim(ids, keys, dict(DEFAULT_CFG), "warm", init)
    up = np.ones(n, np.uint8)
    t0 = round_tick(0)
    for g in (gpu, orc):
        g.begin_round(t0, up)
        for p in range(300):
            g.run_phase(t0 + 1 + p, [(0, 1), (2, 3), (4, 5)] if p % 2 == 0 else [(2, 1), (4, 3), (0, 5)])
        g.liveness(t0 + 301, up)
    t1 = round_tick(6)
    for g in (gpu, orc):
        g.begin_round(t1, up)
    slot = gpu.region("ESC_SLOT", torch.int32, (gpu.np_,))[:n].cpu().numpy()
    assert slot[1] != -1, "column 1 should be escaped"
    want = orc.export()
    assert int(want["hb"][1, 1]) > 256 and int(want["hb"][1, 1]) - int(want["hb"][7, 1]) >= 256
    assert compare_exports(gpu.export(), want) is None
    nid = [nodeid_size(x.name, x.generation_id, *x.gossip_advertise_addr, x.tls_name) for x in ids]
    ref = TrafficRef(nid, [len(k.encode()) for k in keys], orc.values, DEFAULT_CFG)
    pairs = [(7, 1), (1, 6), (6, 7), (0, 1), (39, 2), (1, 38)]
    assert_census(census(gpu, t1 + 1, pairs), ref.phase(want, pairs, t1 + 1), "escaped column")
    gpu.check()
    gpu.close()
    orc.close()


# ---------------------------------------------------------------- 6. refusals and invalid exchanges
def raw(gpu, ini, res, legs, n, t, flags, msg, legs_out, nodes, tot, cid=15):
    def p(x):
        return C.c_void_p(x.data_ptr()) if x is not None else None

    return gpu.L.gs_traffic_census(gpu.h, p(ini), p(res), p(legs), n, t, cid, flags, p(msg), p(legs_out), p(nodes),
                                   C.byref(tot) if tot is not None else None)


def test_refusals():
    spec = WorkloadSpec(n=64, k=4, fanout=2, seed=3, init="warm", write_frac=0.5)
    scen = make_scenario("ref64", spec, 2, {})
    gpu = make_backend(GossipSim, scen, **PREFIX)
    replay_round(gpu, scen, 0)
    t = round_tick(1)
    ini, res = gpu._pairs_dev([0, 2], [1, 3])
    lo = torch.zeros(2, dtype=torch.uint8, device=gpu.device)
    tot = _lib.GsTrafficTotals()
    inv, uns = _lib.GS_E_INVALID, -5
    assert raw(gpu, None, res, None, 2, t, 0, None, lo, None, tot) == inv
    assert raw(gpu, ini, None, None, 2, t, 0, None, lo, None, tot) == inv
    assert raw(gpu, ini, res, None, 2, t, 2, None, lo, None, tot) == inv  # unknown flag bit
    assert raw(gpu, ini, res, None, 2, t, 0, None, None, None, None) == inv  # every output NULL
    latest = gpu.latest_tick()
    assert raw(gpu, ini, res, None, 2, latest - 1, 0, None, lo, None, tot) == inv
    assert raw(gpu, ini, res, None, 2, latest + (1 << 15), 0, None, lo, None, tot) == inv
    assert raw(gpu, ini, res, None, 2, latest, 0, None, lo, None, tot) == 0
    assert raw(gpu, None, None, None, 0, latest, 0, None, lo, None, tot) == 0 and tot.exchanges == 0
    gpu.close()
    sl = make_backend(GossipSim, scen, sliced=True, **PREFIX)
    assert raw(sl, ini, res, None, 2, 0, 0, None, lo, None, tot) == uns
    with pytest.raises(GsError, match="GS_E_UNSUPPORTED|one-slice"):
        sl.traffic_census(0, [(0, 1)])
    sl.close()


@pytest.mark.parametrize("layout", ["general", "hb8mv8_esc4"])
def test_invalid_exchanges_count_in_bad_index_only(layout):
    spec = WorkloadSpec(n=64, k=4, fanout=2, seed=3, init="warm", write_frac=0.5)
    scen = make_scenario("bad64", spec, 2, {"mtu": 600})
    gpu = make_backend(GossipSim, scen, **LAYOUTS_W[layout])
    t, pairs = advance(gpu, scen, 1)
    good = pairs[:6]
    mixed = [good[0], (3, 3), good[1], (-1, 2), (5, 64), good[2], good[3], (70000, 1), good[4], good[5]]
    legs = [3, 3, 2, 3, 3, 3, 7, 3, 1, 0]  # exchange 6 (a valid pair) has legs 7
    valid = [0, 2, 5, 8, 9]
    want = census(gpu, t, [mixed[i] for i in valid], legs=[legs[i] for i in valid], frame_limit=True)
    got = census(gpu, t, mixed, legs=legs, frame_limit=True)
    assert got["totals"]["bad_index"] == 5 and got["totals"]["exchanges"] == 5
    for i in range(len(mixed)):
        if i in valid:
            assert got["msg"][i] == want["msg"][valid.index(i)] and got["legs_out"][i] == want["legs_out"][valid.index(i)]
        else:
            assert got["msg"][i] == [0, 0, 0, 0] and got["legs_out"][i] == 0
    assert np.array_equal(got["nodes"], want["nodes"])
    for k in TOTAL_KEYS:
        if k != "bad_index":
            assert got["totals"][k] == want["totals"][k], k
    assert gpu.counters()["err_bad_index"] == 0  # the census counts in its own totals only
    gpu.close()


# ---------------------------------------------------------------- 7. the round driver
def test_driver_frame_limit_equals_the_manual_loop():
    """WorkloadSpec(frame_limit=True, loss=0.25): driver.run_round sizes every phase and runs it with the census's
    legs_out, asynchronously -- the same states and counters as the loop of test 1 written out by hand."""
    from aiocluster_amd import driver

    spec = WorkloadSpec(n=40, k=4, fanout=3, seed=59, init="warm", write_frac=0.6, down_frac=0.3, down_rounds=3,
                        loss=0.25, cut_seed=0xF4A3, frame_limit=True)
    scen = make_scenario("drv40", spec, 8, {"mtu": 1500})
    kw = dict(PREFIX, hb8=True, mv8=True)
    a, b = make_backend(GossipSim, scen, **kw), make_backend(GossipSim, scen, **kw)
    delivered, rejected = 0, 0
    for rd in driver.prepare(spec, 8, torch, a.device):
        assert rd["frame_limit"] and "legs" in rd
        rd["traffic_totals"] = True
        driver.run_round([a], rd)
        delivered += rd["traffic"]["delta_bytes_delivered"]
        rejected += sum(rd["traffic"]["rejected"])
    for rd in driver.prepare(spec, 8, torch, b.device):
        driver.begin([b], rd)
        for i, (x, y, n, t) in enumerate(rd["phases"]):
            if n:
                out = b.traffic_census(t, (x, y), legs=rd["legs"][i], frame_limit=True, totals=False)
                b.run_phase_arrays(t, x, y, out["legs_out"])
        driver.end([b], rd)
    ra, rb = state_regions(a), state_regions(b)
    for name in ra:
        assert ra[name] == rb[name], name
    ca, cb = a.check(), b.check()
    assert ca == cb and ca["delta_bytes"] == delivered and ca["cut_exchanges"] > 0 and rejected > 0
    a.close()
    b.close()


def test_driver_default_spec_is_gs_run_phase():
    """Without frame_limit (and without loss) run_round does what it did: gs_run_phase on every phase."""
    from aiocluster_amd import driver

    spec = WorkloadSpec(n=300, k=4, fanout=3, seed=21, init="warm", write_frac=0.2)
    assert spec.frame_limit is False
    scen = make_scenario("drv300", spec, 3, {"mtu": 1500})
    kw = dict(PREFIX, hb8=True, mv8=True)
    a, b = make_backend(GossipSim, scen, **kw), make_backend(GossipSim, scen, **kw)
    for rd in driver.prepare(spec, 3, torch, a.device):
        assert "frame_limit" not in rd and "legs" not in rd
        driver.run_round([a], rd)
        assert "traffic" not in rd
    for rd in driver.prepare(spec, 3, torch, b.device):
        driver.begin([b], rd)
        for x, y, n, t in rd["phases"]:
            if n:
                b._chk(b.L.gs_run_phase(b.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), n, t), "gs_run_phase")
        driver.end([b], rd)
    ra, rb = state_regions(a), state_regions(b)
    for name in ra:
        assert ra[name] == rb[name], name
    ca, cb = a.check(), b.check()
    assert ca == cb and ca["cut_exchanges"] == 0 and ca["exchanges"] > 0
    a.close()
    b.close()

"""gs_age_census and the write log (gs_note_writes), on the GPU.

Every expected value is ``tests/ageref.py`` (numpy, from the definition) over readback paths the rest of the suite
pins to the oracle -- ``mv_words``, GS_R_POS, GS_R_SELF_MV -- and the log copied out, or over the oracle's own export;
never a result of the kernel.  Every comparison is exact.

In the reference's terms: for observer o and owner j, how long ago owner j made the oldest write that
``cluster_state.node_state(j).max_version`` at o does not cover yet (``aiocluster/state.py:137-180`` are the writes,
``state.py:340-415`` the anti-entropy that carries them), and how long a write took to be covered everywhere.
"""

import ctypes as C

import numpy as np
import pytest
from ageref import GS_NONE, age_census_ref, assert_age_census, bucket
from test_gpu_view_census import LAYOUTS, SCHED, _eight, make, readback, spec_for

from aiocluster_amd import _lib, driver
from aiocluster_amd._lib import GsError
from aiocluster_amd.scenario import DEFAULT_CFG
from aiocluster_amd.shard import ShardGroup
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.staleness import new_log_host, note_writes_host
from aiocluster_amd.workload import (TICKS_PER_ROUND, key_names, liveness_tick, phase_tick, round_tick,
                                     synthetic_node_ids)

pytestmark = pytest.mark.gpu


def log_of(sim) -> np.ndarray:
    sim.sync()
    return sim.wlog.cpu().numpy().view(np.uint32)


def done_of(sim) -> np.ndarray:
    return sim.age_done.cpu().numpy().astype(np.int64)


def check(sim, up, what="", tick=None):
    """The census against ageref with up = None and with the mask, floor and rows whole, without ``done`` (twice:
    repeatable) and then with it (the sim's vector against the reference's).  Returns the all-rows census."""
    rb, log = readback(sim), log_of(sim)
    t = sim.latest_tick() if tick is None else tick
    res = None
    for u in (None, up):
        uh = None if u is None else u.cpu().numpy()
        want = age_census_ref(rb["ver"], rb["known"], rb["M"], log, t, up=uh)
        for _ in range(2):
            got = sim.age_census(up=u, tick=tick, per_owner=True, per_row=True, spread=False)
            assert_age_census(got, want, (what, "all rows" if u is None else "up mask"))
        res = got if res is None else res
    d0 = done_of(sim)
    want = age_census_ref(rb["ver"], rb["known"], rb["M"], log, t, up=up.cpu().numpy(), done=d0)
    got = sim.age_census(up=up, tick=tick, per_owner=True, per_row=True, spread=True)
    assert_age_census(got, want, (what, "with done"))
    assert np.array_equal(done_of(sim), want["done"]), what
    return res


# ---------------------------------------------------------------- 1. layouts at N = 200 (3 x 64 + 8 columns)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_age_census_matches_numpy_in_every_layout(layout):
    import torch

    n, K = 200, 4
    sim = make(n, K, layout, write_log=True)
    plans = driver.prepare(spec_for(n, K, layout), 4, torch, sim.device)
    cold = layout == "cold_general"
    for r in range(3):
        driver.run_round([sim], plans[r])
        if cold and r == 0:  # after round 1: most pairs still unknown, aged from version 1's tick
            got = check(sim, plans[r]["up"], what=f"{layout} round 1")
            assert got["unknown"] > 0 and got["unlogged"] == 0
            rb, log = readback(sim), log_of(sim)
            o, j = np.argwhere(~rb["known"])[0]
            assert rb["M"][j] > 0 and log[j, 1] == 0  # the boot write, logged at its tick
            assert got["row_max_age"][o].item() >= sim.latest_tick() - int(log[j, 1]) == got["max_age"]
    got = check(sim, plans[2]["up"], what=f"{layout} after 3 rounds")
    assert got["observers"] == n and got["pairs"] == n * n and got["unlogged"] == 0
    # mid-round: round 4's writes are in and logged, no exchange has carried them (each leaves n - 1 views behind)
    driver.begin([sim], plans[3])
    got = check(sim, plans[3]["up"], what=f"{layout} mid-round")
    assert got["behind"] > 0 and got["pending_writes"] > 0 and got["unlogged"] == 0 and got["unlogged_writes"] == 0
    assert plans[3]["nops"] > 0 and got["age_hist"][0] > 0  # the fresh writes: age 0 at the round's tick
    driver.run_phases([sim], plans[3])
    driver.end([sim], plans[3])
    sim.check()
    sim.close()


# ---------------------------------------------------------------- 2. the log
def test_log_follows_effective_writes_and_skipped_versions_are_unlogged():
    import torch

    n = 8
    keys = key_names(2)
    sim = GossipSim(synthetic_node_ids(n), keys, dict(DEFAULT_CFG), "warm", None, tombstones=True, fd_ring=True,
                    hist_cap=8, write_log=True)
    assert sim.wlog.shape == (n, sim.wlog_words) and sim.wlog_words == _lib.write_log_words(2, 8) == 16
    host = new_log_host(n, sim.wlog_words)
    assert np.array_equal(log_of(sim), host)  # gs_write_log_init
    M = lambda: sim.region("SELF_MV", torch.int32, (sim.np_,)).cpu().numpy()[:n]  # noqa: E731
    script = [
        (10, lambda t: (sim.set(t, 0, keys[0], "a"), sim.set(t, 2, keys[1], "b"))),
        (20, lambda t: sim.set(t, 0, keys[0], "a")),                 # same value: no-op
        (30, lambda t: (sim.delete(t, 0, keys[0]), sim.delete(t, 1, keys[0]))),  # owner 1: absent key, no-op
        (40, lambda t: sim.delete_after_ttl(t, 2, keys[1])),
        (45, lambda t: sim.delete_after_ttl(t, 3, keys[1])),         # absent key: no-op
        (50, lambda t: (sim.set(t, 0, keys[1], "c"), sim.set(t, 5, keys[0], "d"))),
    ]
    for t, step in script:
        step(t)
        sim._flush()
        note_writes_host(host, M(), t)
    dev = log_of(sim)
    assert np.array_equal(dev, host)
    N = GS_NONE
    assert dev[0, :5].tolist() == [N, 10, 30, 50, N] and dev[2, :4].tolist() == [N, 10, 40, N]
    assert dev[5, :3].tolist() == [N, 50, N] and (dev[[1, 3, 4, 6, 7]] == N).all()
    assert M().tolist() == [3, 0, 2, 0, 0, 1, 0, 0]
    # gossip until every view has everything
    up = torch.ones(n, dtype=torch.uint8, device=sim.device)
    for r in range(6):
        sim.begin_round(round_tick(r), up)
        for p in range(4):
            sim.run_phase(phase_tick(r, p), SCHED[p])
        sim.liveness(liveness_tick(r, 4), up)
        if sim.view_census()["converged"]:
            break
    assert sim.view_census()["converged"]
    got = check(sim, up, what="converged")
    assert got["behind"] == 0 and got["pending_writes"] == 0 and done_of(sim).tolist() == M().tolist()
    # one batch through raw gs_owner_writes, never noted (owner 0: version 4), then a noted batch (version 5)
    t4, t5 = round_tick(r + 1), round_tick(r + 1) + 3
    ops = torch.tensor([[0, 0, 0, sim.intern("e"), 1]], dtype=torch.int32, device=sim.device)
    sim._chk(sim.L.gs_owner_writes(sim.h, C.c_void_p(ops.data_ptr()), 1, t4), "gs_owner_writes")
    sim.set(t5, 0, keys[1], "f")
    sim._flush()
    dev = log_of(sim)
    assert M()[0] == 5 and dev[0, 4] == N and dev[0, 5] == t5
    note_writes_host(host, M(), t5)
    assert np.array_equal(dev, host)
    got = check(sim, up, what="skipped version", tick=t5 + 2)
    # the seven other views are at version 3: behind on the version nobody logged
    assert (got["behind"], got["unlogged"], got["max_age"], sum(got["age_hist"])) == (n - 1, n - 1, 0, 0)
    assert got["row_max_age"].count_nonzero().item() == 0 and got["owner_floor"][0].item() == 3
    assert (got["pending_writes"], got["unlogged_writes"], got["max_pending_age"]) == (1, 1, 2)
    sim.close()


# ---------------------------------------------------------------- 3. wrapped 8-bit versions
def test_ages_with_versions_past_2_7_span_an_absence():
    """The 150-round scenario of the view-census test: every node writes each round it is up, node 7 is away for
    20 rounds, owners' versions pass 2^7 (the 8-bit views wrap).  Node 7's views lack the writes of the round it
    left in: their age spans the whole absence."""
    import torch

    rounds, down0, down1 = 150, 120, 140
    sim = _eight(hist_cap=100, cfg={"mtu": 300}, write_log=True)
    n = sim.n
    seen = False
    for r in range(rounds):
        up = np.ones(n, np.uint8)
        if down0 <= r < down1:
            up[7] = 0
        up_dev = torch.from_numpy(up).to(sim.device)
        t = round_tick(r)
        for j in range(n):
            if up[j]:
                sim.write(t, j, r % 2, 0, f"v{j}.{r}")
        sim.begin_round(t, up_dev)
        for p in range(2):
            sim.run_phase(phase_tick(r, p), [(a, b) for a, b in SCHED[(r + p) % len(SCHED)] if up[a] and up[b]])
        sim.liveness(liveness_tick(r, 2), up_dev)
        if r in (down1 - 1, rounds - 1):
            M = sim.region("SELF_MV", torch.int32, (sim.np_,)).cpu().numpy()[:n]
            assert (M >= 128).any()
            got = check(sim, up_dev, what=f"round {r}")
            assert got["unlogged"] == 0 and got["unlogged_writes"] == 0
            if r == down1 - 1:
                # node 7 lacks the writes of round `down0` (and whatever had not reached it when it left)
                away = liveness_tick(r, 2) - round_tick(down0)
                assert got["max_age"] >= away >= (down1 - 1 - down0) * TICKS_PER_ROUND
                assert got["row_max_age"][7].item() == got["max_age"] and got["age_hist"][bucket(got["max_age"])] > 0
                # without done the oldest pending write of a column is the one its oldest view lacks
                assert got["max_pending_age"] == got["max_age"]
                seen = True
    assert seen and sim.check()["err_hb_lag"] == 0
    sim.close()


# ---------------------------------------------------------------- 4. spread latency
@pytest.mark.parametrize("down", [None, 7])
def test_a_write_is_credited_once_when_it_is_everywhere(down):
    """One write on 8 nodes under the fixed matching schedule, a census after every phase: the write is credited at
    the first census at which every counted observer has it, with latency = that tick - the write's tick, and never
    again.  With node 7 down and masked out, "every node" is the other seven."""
    import torch

    sim = _eight(hist_cap=8, write_log=True)
    n, owner = sim.n, 3
    uph = np.ones(n, np.uint8)
    if down is not None:
        uph[down] = 0
    up = torch.from_numpy(uph).to(sim.device)
    everyone = int(uph.sum())
    boot = sim.age_census(up=up)  # the boot writes are everywhere (warm start): credited here, at tick 0
    assert (boot["spread_writes"], boot["max_spread_latency"], boot["pending_writes"]) == (n, 0, 0)
    t0 = round_tick(0)
    sim.set(t0, owner, sim.keys[1], "fresh")
    sim.begin_round(t0, up)
    m_new = int(sim.region("SELF_MV", torch.int32, (sim.np_,))[owner].item())
    assert m_new == 2 and log_of(sim)[owner, 2] == t0
    got = sim.age_census(up=up)
    assert (got["spread_writes"], got["pending_writes"], got["behind"]) == (0, 1, everyone - 1)
    credited_at = None
    for p in range(8):
        t = phase_tick(0, p)
        sim.run_phase(t, [(a, b) for a, b in SCHED[p % 4] if uph[a] and uph[b]])
        reach = sim.view_census(up=up, probes=[(owner, m_new)])["reach"][0]
        got = sim.age_census(up=up)
        if reach == everyone and credited_at is None:
            credited_at = t
            assert (got["spread_writes"], got["pending_writes"], got["behind"]) == (1, 0, 0)
            assert got["max_spread_latency"] == t - t0 and got["spread_hist"][bucket(t - t0)] == 1
            assert int(sim.age_done[owner].item()) == m_new
        else:
            assert got["spread_writes"] == 0 and sum(got["spread_hist"]) == 0 and got["max_spread_latency"] == 0
            assert got["pending_writes"] == (0 if credited_at else 1)
            assert got["behind"] == everyone - reach
            if not credited_at:
                assert got["max_pending_age"] == got["max_age"] == t - t0
    assert credited_at is not None and credited_at > phase_tick(0, 0)  # not before the second phase: 2^p nodes at most
    sim.liveness(liveness_tick(0, 8), up)
    sim.close()


# ---------------------------------------------------------------- 5. chunk and band boundaries
def test_age_census_across_chunk_and_band_boundaries():
    """4,200 owner columns: one more column chunk than 4,096 (4,200 = 65 x 64 + 40: every tail is live); 4,200 rows:
    16 bands of 256 and a band of 104.  ``owner_floor`` and ``row_max_age`` are compared whole."""
    import torch

    n, K = 4200, 4
    sim = make(n, K, "hb8mv8", write_log=True)
    plans = driver.prepare(spec_for(n, K, "hb8mv8", seed=42, write_frac=0.1), 3, torch, sim.device)
    for r in range(2):
        driver.run_round([sim], plans[r])
    got = check(sim, plans[1]["up"], what="4200 after 2 rounds")
    assert got["behind"] > 0 and got["unlogged"] == 0
    driver.begin([sim], plans[2])
    got = check(sim, plans[2]["up"], what="4200 mid-round")
    assert 0 < got["behind"] < got["pairs"] == n * n and got["pending_writes"] > 0 and got["unlogged"] == 0
    driver.run_phases([sim], plans[2])
    driver.end([sim], plans[2])
    sim.close()


# ---------------------------------------------------------------- 6. read-only and repeatable
def test_age_census_is_read_only_and_repeatable():
    import torch

    n, K = 200, 4
    sim = make(n, K, "hb8mv8", write_log=True)
    plans = driver.prepare(spec_for(n, K, "hb8mv8"), 4, torch, sim.device)
    for rd in plans[:3]:
        driver.run_round([sim], rd)
    driver.begin([sim], plans[3])

    def snap():
        sim.sync()
        return {r: t.cpu().numpy().tobytes() for r, t in sim.regions.items()}, log_of(sim).tobytes()

    before, c0 = snap(), sim.counters()
    up = plans[3]["up"]
    a = sim.age_census(up=up, per_owner=True, per_row=True, spread=False)
    b = sim.age_census(up=up, per_owner=True, per_row=True, spread=False)
    after, c1 = snap(), sim.counters()
    assert set(before[0]) == set(sim.regions) and before == after
    assert c0 == c1
    assert a["behind"] > 0
    for k in a:
        if hasattr(a[k], "cpu"):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k
    driver.run_phases([sim], plans[3])
    driver.end([sim], plans[3])
    sim.close()


# ---------------------------------------------------------------- 7. slices
def test_three_slices_give_one_handles_age_census():
    """448 nodes in three slices of 192 / 192 / 64 owner columns, each with its own columns' log and done vector."""
    import torch

    n, K = 448, 4
    cfg = dict(DEFAULT_CFG)
    kw = dict(init="warm", tombstones=False, fd_ring=False, hist_cap=16, initial_ops=driver.boot_ops(n, K), hb8=True,
              mv8=True, write_log=True)
    ids, keys = synthetic_node_ids(n), key_names(K)
    one = GossipSim(ids, keys, cfg, **kw)
    grp = ShardGroup.in_process(ids, keys, cfg, shards=3, **kw)
    assert [s.ncol for s in grp.slices] == [192, 192, 64]
    plans = driver.prepare(spec_for(n, K, "hb8mv8", seed=21), 4, torch, one.device)

    def same(a, b):
        assert set(a) == set(b)
        for k in a:
            if hasattr(a[k], "cpu"):
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], (k, a[k], b[k])

    for r in range(3):
        driver.run_round([one], plans[r])
        driver.run_round(grp.slices, plans[r], group=grp)
        same(one.age_census(up=plans[r]["up"], per_owner=True, per_row=True),
             grp.age_census(up=plans[r]["up"], per_owner=True, per_row=True))
    driver.begin([one], plans[3])
    driver.begin(grp.slices, plans[3])
    assert np.array_equal(log_of(one), np.concatenate([log_of(s) for s in grp.slices]))
    up = plans[3]["up"]
    for u in (None, up):
        a = one.age_census(up=u, per_owner=True, per_row=True)
        same(a, grp.age_census(up=u, per_owner=True, per_row=True))
        assert a["behind"] > 0 and a["pending_writes"] > 0
    assert np.array_equal(done_of(one), np.concatenate([done_of(s) for s in grp.slices]))
    for s in grp.slices:  # each slice alone: its own columns
        check(s, up, what=f"slice {s.shard}")
    one.close()
    for s in grp.slices:
        s.close()


# ---------------------------------------------------------------- 8. against the oracle
def test_age_census_equals_the_oracles_after_every_lossy_round():
    """The N = 1,100 lossy composer run of tests/test_gpu_lossy.py.  The reference side is the oracle's alone: ageref
    over its exported versions, with a log kept by note_writes_host from its own max_versions (a round's writes all
    carry the round's tick, so an owner that moved by several versions is noted one version at a time, as the
    device's batches of distinct owners are)."""
    from helpers import initial_by_owner, make_backend
    from lossycases import warm_lossy
    from test_gpu_lossy import LAYOUTS_W, composer_exports

    from aiocluster_amd.scenario import replay_round, round_ticks

    scen = warm_lossy(rounds=2)
    want = composer_exports(scen)
    n = len(want[0]["mv"])
    gpu = make_backend(GossipSim, scen, write_log=True, **LAYOUTS_W["hb8mv8_esc4"])
    log = new_log_host(n, gpu.wlog_words)
    prev, done = np.zeros(n, np.int64), np.zeros(n, np.int64)

    def note(M, tick):
        nonlocal prev
        for step in range(1, int((M - prev).max()) + 1):
            note_writes_host(log, np.minimum(prev + step, M), tick)
        prev = M.copy()

    # the boot values: one write per initial key, at tick 0 (every view holds them: a warm start)
    init = initial_by_owner(scen)
    note(np.array([len(init.get(j, [])) for j in range(n)], dtype=np.int64), 0)
    for r, rd in enumerate(scen["rounds"]):
        replay_round(gpu, scen, r)
        M = np.diag(want[r]["mv"]).astype(np.int64)
        note(M, round_tick(r))
        tick = round_ticks(scen, r)[-1]
        assert gpu.latest_tick() == tick
        uph = np.asarray(rd["up"], dtype=np.uint8)
        up = gpu._dev(uph, gpu.torch.uint8)
        for u in (None, up):
            ref = age_census_ref(want[r]["mv"], want[r]["pos"] != -1, M, log, tick, up=None if u is None else uph)
            got = gpu.age_census(up=u, per_owner=True, per_row=True, spread=False)
            assert_age_census(got, ref, (r, u is None))
            assert got["unlogged"] == 0
        ref = age_census_ref(want[r]["mv"], want[r]["pos"] != -1, M, log, tick, up=uph, done=done)
        got = gpu.age_census(up=up, per_owner=True, per_row=True)
        assert_age_census(got, ref, (r, "done"))
        done = ref["done"]
        assert np.array_equal(done_of(gpu), done)
        assert got["pairs"] == int(uph.sum()) * n and got["behind"] > 0
        assert got["spread_writes"] > 0 or r > 0  # the boot writes are credited by the first census
    assert np.array_equal(log_of(gpu), log)
    gpu.check()
    gpu.close()


# ---------------------------------------------------------------- 9. refusals
def test_refusals():
    sim = _eight(hist_cap=8, write_log=True)
    up = sim.torch.ones(sim.n, dtype=sim.torch.uint8, device=sim.device)
    sim.begin_round(round_tick(0), up)
    sim.run_phase(phase_tick(0, 0), SCHED[0])
    sim.liveness(liveness_tick(0, 1), up)
    latest = sim.latest_tick()
    assert latest == liveness_tick(0, 1)
    before = done_of(sim)
    for tick in (latest - 1, 0, latest + (1 << 15), latest + (1 << 20)):
        with pytest.raises(GsError, match="gs_age_census.*tick"):
            sim.age_census(tick=tick)
    tot = _lib.GsAgeTotals()
    log = C.c_void_p(sim.wlog.data_ptr())
    inv = _lib.GS_E_INVALID
    assert sim.L.gs_age_census(sim.h, None, log, latest, 4, None, None, None, C.byref(tot)) == inv
    assert b"gs_age_census" in sim.L.gs_last_error(sim.h)
    assert sim.L.gs_age_census(sim.h, None, None, latest, 0, None, None, None, C.byref(tot)) == inv
    assert sim.L.gs_age_census(sim.h, None, log, latest, 0, None, None, None, None) == inv
    assert np.array_equal(done_of(sim), before)  # refused before any device work
    ok = sim.age_census(tick=latest + (1 << 15) - 1)  # the last tick allowed
    assert ok["observers"] == sim.n
    plain = _eight(hist_cap=8)
    with pytest.raises(GsError, match="write_log"):
        plain.age_census()
    with pytest.raises(GsError, match="write_log"):
        plain.note_writes(0)
    plain.close()
    sim.close()

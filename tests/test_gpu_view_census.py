"""gs_view_census, the device-side dissemination census (GPU only).

Every expected value is numpy over readback paths the rest of the suite pins to the oracle
(``mv_words``, ``decode_heartbeats``, GS_R_SELF_MV / SELF_HB, GS_R_POS), never the census itself; the
buckets are computed here (0 for lag 0, else min(19, bit length)); every comparison is exact.

What the census answers in the reference's terms: for observer o and owner j, whether
``cluster_state.node_state(j).max_version`` at o has reached the owner's own (``aiocluster/state.py:340-415``
is the anti-entropy that makes it so), and how far o's copy of j's heartbeat trails (``state.py:197-204``).
"""

import socket

import numpy as np
import pytest

from aiocluster_amd import driver
from aiocluster_amd._lib import GS_NONE
from aiocluster_amd.scenario import DEFAULT_CFG
from aiocluster_amd.shard import DistComm, ShardGroup
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.workload import (WorkloadSpec, key_names, liveness_tick, phase_tick, round_tick,
                                     synthetic_node_ids)

pytestmark = pytest.mark.gpu

BUCKETS = 20
TOTALS = ("observers", "views", "unknown", "behind", "inexact", "max_version_lag", "max_heartbeat_lag")

LAYOUTS = {
    "u16_tombstones": dict(init="warm", tombstones=True),
    "hb8": dict(init="warm", tombstones=False, hb8=True),
    "hb8mv8": dict(init="warm", tombstones=False, hb8=True, mv8=True),
    "cold_general": dict(init="cold", tombstones=True),
    "no_held": dict(init="warm", tombstones=False, held=False),
}


def bucket(lag: int) -> int:
    return 0 if lag == 0 else min(BUCKETS - 1, int(lag).bit_length())


def hist_of(lags: np.ndarray) -> list[int]:
    out = [0] * BUCKETS
    cnt = np.bincount(lags.ravel())
    for v in np.flatnonzero(cnt).tolist():
        out[bucket(v)] += int(cnt[v])
    return out


def readback(sim) -> dict:
    """The state the census reads, through the readback paths only (shared by the references of one state)."""
    torch = sim.torch
    sim.sync()
    nc, n = sim.ncol, sim.n
    w = sim.mv_words().cpu().numpy()[:, :nc]
    rb = {"ver": (w & 0x7FFF).astype(np.int32), "inex": (w >> 15).astype(bool),
          "M": sim.region("SELF_MV", torch.int32, (sim.np_,)).cpu().numpy()[:nc].astype(np.int32),
          "R": sim.region("SELF_HB", torch.int32, (sim.np_,)).cpu().numpy()[:nc].astype(np.int64)}
    if sim.canonical:
        rb["known"] = np.ones((n, nc), bool)
    else:
        rb["known"] = sim.region("POS", torch.int32, (n, sim.np_)).cpu().numpy().view(np.uint32)[:, :nc] != GS_NONE
    rb["hb"] = sim.decode_heartbeats(sim.hb_region().cpu().numpy())[:, :nc].astype(np.int64)
    return rb


def reference(sim, up=None, heartbeats=False, probes=(), rb=None):
    """The census of ``sim``'s columns from readback alone."""
    rb = readback(sim) if rb is None else rb
    nc, n = sim.ncol, sim.n
    ver, inex, M, known = rb["ver"], rb["inex"], rb["M"], rb["known"]
    rows = np.ones(n, bool) if up is None else np.asarray(up).astype(bool)
    cnt = known & rows[:, None]
    lag = M[None, :] - ver
    assert (lag[cnt] >= 0).all()
    behind = cnt & (lag > 0)
    unknown = ~known & rows[:, None]
    out = {
        "observers": int(rows.sum()), "views": int(cnt.sum()), "unknown": int(unknown.sum()),
        "behind": int(behind.sum()), "inexact": int((inex & cnt).sum()),
        "max_version_lag": int(lag[cnt].max()) if cnt.any() else 0, "max_heartbeat_lag": 0,
        "version_lag_hist": hist_of(lag[cnt]), "heartbeat_lag_hist": [0] * BUCKETS,
    }
    if heartbeats:
        hl = (rb["R"][None, :] - rb["hb"])[cnt]
        assert (hl >= 0).all()
        out["max_heartbeat_lag"] = int(hl.max()) if cnt.any() else 0
        out["heartbeat_lag_hist"] = hist_of(hl)
    out["converged"] = out["behind"] == 0 and out["unknown"] == 0
    out["reach"] = []
    for j, v in probes:
        jl = j - sim.col_lo
        out["reach"].append(int((cnt[:, jl] & (ver[:, jl] >= v)).sum()) if 0 <= jl < nc else 0)
    out["owner_behind"] = behind.sum(0)
    out["owner_unknown"] = unknown.sum(0)
    out["owner_max_lag"] = np.where(cnt, lag, 0).max(0)
    out["row_stale"] = (behind | unknown).sum(1)
    return out


def assert_census(got, want, what=""):
    for k in TOTALS + ("version_lag_hist", "heartbeat_lag_hist", "converged", "reach"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("owner_behind", "owner_unknown", "owner_max_lag", "row_stale"):
        if k in got:
            g = got[k].cpu().numpy().astype(np.int64)
            assert g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k, np.flatnonzero(g != want[k])[:8])
    assert sum(got["version_lag_hist"]) == got["views"]


def check_all(sim, up, probes=(), what=""):
    """Totals, both histograms, per-owner planes, per-row counts, with up = None and with the mask."""
    res = []
    rb = readback(sim)
    for u in (None, up):
        for hbs in (False, True):
            got = sim.view_census(up=u, heartbeats=hbs, probes=probes, per_owner=True, per_row=True)
            want = reference(sim, None if u is None else u.cpu().numpy(), hbs, probes, rb)
            assert_census(got, want, (what, "all rows" if u is None else "up mask", hbs))
            if hbs:
                assert sum(got["heartbeat_lag_hist"]) == got["views"]
            res.append(got)
    return res[1]  # all rows, heartbeats on


def make(n, K, layout, cfg=None, **over):
    kw = dict(LAYOUTS[layout], fd_ring=False, hist_cap=16, initial_ops=driver.boot_ops(n, K))
    kw.update(over)
    c = dict(DEFAULT_CFG)
    if layout == "no_held":
        c["mtu"] = 1 << 30  # version-only views: no NodeDelta may be cut
    c.update(cfg or {})
    return GossipSim(synthetic_node_ids(n), key_names(K), c, **kw)


def spec_for(n, K, layout, seed=7, **over):
    tomb = LAYOUTS[layout].get("tombstones", False)
    kw = dict(n=n, k=K, fanout=1 if layout == "cold_general" else 3, seed=seed, init=LAYOUTS[layout]["init"],
              write_frac=0.3, delete_frac=0.1 if tomb else 0.0, down_frac=0.15, down_rounds=3)
    kw.update(over)
    return WorkloadSpec(**kw)


# ---------------------------------------------------------------- 1. layouts at N = 200 (3 x 64 + 8 columns)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_census_matches_numpy_in_every_layout(layout):
    import torch

    n, K = 200, 4
    sim = make(n, K, layout)
    plans = driver.prepare(spec_for(n, K, layout), 4, torch, sim.device)
    cold = layout == "cold_general"
    for r in range(3):
        driver.run_round([sim], plans[r])
        if cold and r in (0, 2):  # after rounds 1 and 3: views still unknown
            got = check_all(sim, plans[r]["up"], what=f"{layout} round {r + 1}")
            assert got["unknown"] > 0 and got["views"] < got["observers"] * n
            assert got["views"] + got["unknown"] == got["observers"] * n
    got = check_all(sim, plans[2]["up"], what=f"{layout} after 3 rounds")
    assert got["observers"] == n
    # mid-round: round 4's writes are in, no exchange has carried them yet (each leaves n - 1 views behind)
    driver.begin([sim], plans[3])
    got = check_all(sim, plans[3]["up"], what=f"{layout} mid-round")
    assert 0 < got["behind"] < got["views"]
    assert not got["converged"] and got["max_version_lag"] >= 1
    if not cold:
        assert got["unknown"] == 0 and got["views"] == n * n
    driver.run_phases([sim], plans[3])
    driver.end([sim], plans[3])
    sim.check()
    sim.close()


# ---------------------------------------------------------------- 2. holes
@pytest.mark.parametrize("layout", ["u16_prefix", "hb8mv8", "u16_tombstones"])
def test_census_counts_views_with_holes(layout):
    """An mtu of 200 cuts NodeDeltas: the receiving views get holes (GS_MV_INEXACT).  With GS_TOMBSTONES the flag
    does not exist (bit 15 is always 0, GS_R_HELD always kept): the census reports 0 there, as inexact_views does."""
    import torch

    n, K = 200, 4
    if layout == "u16_prefix":
        sim = make(n, K, "hb8", cfg={"mtu": 200}, hb8=False)
    else:
        sim = make(n, K, layout, cfg={"mtu": 200})
    # nodes away for three rounds while most owners write a key a round: they return two or more keys behind, and
    # such a NodeDelta is what the mtu cuts
    spec = spec_for(n, K, "hb8" if layout == "u16_prefix" else layout, seed=3, write_frac=0.8, down_frac=0.3)
    plans = driver.prepare(spec, 4, torch, sim.device)
    for rd in plans:
        driver.run_round([sim], rd)
    c = sim.check()
    assert c["truncated"] > 0
    got = check_all(sim, plans[-1]["up"], what=layout)
    assert got["inexact"] == sim.inexact_views()
    if layout == "u16_tombstones":
        assert got["inexact"] == 0
    else:
        assert got["inexact"] > 0
    sim.close()


# ---------------------------------------------------------------- 3. escaped columns and wide lags
SCHED = [[(0, 1), (2, 3), (4, 5), (6, 7)], [(1, 2), (3, 4), (5, 6), (7, 0)], [(0, 4), (1, 5), (2, 6), (3, 7)],
         [(5, 0), (6, 1), (7, 2), (4, 3)]]


def _eight(cfg=None, **kw):
    n = 8
    ids, keys = synthetic_node_ids(n), key_names(2)
    init = {j: [(0, f"v{j}")] for j in range(n)}
    return GossipSim(ids, keys, dict(DEFAULT_CFG, **(cfg or {})), "warm", init, tombstones=False, fd_ring=True,
                     hb8=True, mv8=True, **kw)


def test_census_reads_escaped_columns():
    """A 300-phase round in which nodes 6 and 7 take no part: their views of node 1 fall ~300 heartbeats behind,
    the lag sweep moves the column to 16-bit escape slots, and the census reads those views from GS_R_ESC16."""
    import torch

    sim = _eight(hist_cap=8)
    n = sim.n
    up = torch.ones(n, dtype=torch.uint8, device=sim.device)
    t0 = round_tick(0)
    sim.begin_round(t0, up)
    for p in range(300):
        sim.run_phase(t0 + 1 + p, [(0, 1), (2, 3), (4, 5)] if p % 2 == 0 else [(2, 1), (4, 3), (0, 5)])
    sim.liveness(t0 + 301, up)
    slot = sim.region("ESC_SLOT", torch.int32, (sim.np_,)).cpu().numpy().view(np.uint32)[:n]
    assert (slot != GS_NONE).any()
    got = check_all(sim, up, what="escaped")
    assert got["max_heartbeat_lag"] >= 128
    assert got["heartbeat_lag_hist"][9] > 0 or got["heartbeat_lag_hist"][8] > 0
    assert sim.check()["err_hb_lag"] == 0
    sim.close()


def test_census_version_lags_with_versions_past_2_7():
    """Every node writes each round it is up; node 7 is away for 20 rounds: its views fall 20 versions behind owners
    whose max_version has passed 2^7 (the 8-bit views have wrapped), and the census still gives the true lags."""
    import torch

    rounds, down0, down1 = 150, 120, 140
    sim = _eight(hist_cap=100, cfg={"mtu": 300})
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
            got = check_all(sim, up_dev, what=f"round {r}")
            if r == down1 - 1:
                assert got["max_version_lag"] >= 16 and got["version_lag_hist"][5] > 0
                seen = True
    assert seen and sim.check()["err_hb_lag"] == 0
    sim.close()


# ---------------------------------------------------------------- 4. chunk and band boundaries
def test_census_across_chunk_and_band_boundaries():
    """4,200 owner columns: one more column chunk than 4,096 (and 4,200 = 65 x 64 + 40: every tail is live);
    4,200 rows: 16 bands of 256 and a band of 104."""
    import torch

    n, K = 4200, 4
    sim = make(n, K, "hb8mv8")
    plans = driver.prepare(spec_for(n, K, "hb8mv8", seed=42, write_frac=0.1), 3, torch, sim.device)
    for r in range(2):
        driver.run_round([sim], plans[r])
    driver.begin([sim], plans[2])
    M = sim.region("SELF_MV", torch.int32, (sim.np_,)).cpu().numpy()
    probes = [(j, int(M[j]) - d) for j in (0, 4095, 4096, 4199) for d in (0, 1)]
    got = check_all(sim, plans[2]["up"], probes=probes, what="4200")
    assert 0 < got["behind"] < got["views"] == n * n
    assert all(0 < x <= n for x in got["reach"])
    driver.run_phases([sim], plans[2])
    driver.end([sim], plans[2])
    sim.close()


# ---------------------------------------------------------------- 5. probes
@pytest.mark.parametrize("layout", ["hb8mv8", "u16_tombstones", "cold_general"])
def test_probes_match_numpy(layout):
    import torch

    n, K = 200, 4
    sim = make(n, K, layout)
    spec = spec_for(n, K, layout, seed=11)
    plans = driver.prepare(spec, 4, torch, sim.device)
    for r in range(3):
        driver.run_round([sim], plans[r])
    driver.begin([sim], plans[3])
    M = sim.region("SELF_MV", torch.int32, (sim.np_,)).cpu().numpy()[:n]
    # an owner that wrote during the churn rounds (its version moved past the K boot writes)
    wrote = [j for j in range(n) if M[j] >= K + 2 and plans[3]["up_host"][j]]
    assert wrote
    j = wrote[len(wrote) // 2]
    probes = [(j, 0), (j, int(M[j])), (j, int(M[j]) + 1), (j, int(M[j]) - 1), (j, K + 1)]
    up = plans[3]["up"]
    for u in (None, up):
        got = sim.view_census(up=u, probes=probes)
        want = reference(sim, None if u is None else u.cpu().numpy(), False, probes)
        assert got["reach"] == want["reach"], (layout, got["reach"], want["reach"])
        assert got["reach"][2] == 0 and got["reach"][1] >= 1 and got["reach"][0] >= got["reach"][3] >= got["reach"][1]
    assert sim.reach(j) == reference(sim, None, False, [(j, int(M[j]))])["reach"][0]
    # 64 probes, duplicates included
    rng = np.random.default_rng(5)
    many = [(int(o), int(rng.integers(0, M[o] + 2))) for o in rng.integers(0, n, 60)] + probes[:4]
    many[63] = many[0]
    assert len(many) == 64 and len(set(many)) < 64
    got = sim.view_census(up=up, probes=many)
    want = reference(sim, up.cpu().numpy(), False, many)
    assert got["reach"] == want["reach"]
    assert got["reach"][63] == got["reach"][0]
    driver.run_phases([sim], plans[3])
    driver.end([sim], plans[3])
    sim.close()


# ---------------------------------------------------------------- 6. dissemination curve
def test_dissemination_curve_of_one_write():
    import torch

    n, K, owner = 1024, 4, 321
    sim = make(n, K, "hb8mv8")
    spec = WorkloadSpec(n=n, k=K, fanout=3, seed=9, init="warm", write_frac=0.0, quiet_from=0)
    plans = driver.prepare(spec, 12, torch, sim.device)
    sim.set(round_tick(0), owner, key_names(K)[1], "fresh")
    assert sim.reach(owner) == 1  # before the first round: only the owner's own row
    m_new = int(sim.region("SELF_MV", torch.int32, (sim.np_,))[owner].item())
    assert m_new == K + 1
    curve = [1]
    for rd in plans:
        driver.run_round([sim], rd)
        got = sim.view_census(probes=[(owner, m_new)])
        want = reference(sim, None, False, [(owner, m_new)])
        assert got["reach"] == want["reach"]
        assert got["behind"] == want["behind"] == n - got["reach"][0]
        curve.append(got["reach"][0])
    assert all(b >= a for a, b in zip(curve, curve[1:])), curve
    assert curve[-1] == n and curve[1] > 1, curve
    end = sim.view_census()
    assert end["converged"] and end["version_lag_hist"][0] == end["views"] == n * n
    sim.close()


# ---------------------------------------------------------------- 7. read-only and repeatable
def test_census_is_read_only_and_repeatable():
    import torch

    n, K = 200, 4
    sim = make(n, K, "hb8mv8")
    plans = driver.prepare(spec_for(n, K, "hb8mv8"), 3, torch, sim.device)
    for rd in plans:
        driver.run_round([sim], rd)

    def snap():
        sim.sync()
        return {r: sim.regions[r].cpu().numpy().tobytes() for r in ("HB", "MV", "ESC16", "SELF_HB", "SELF_MV", "ROW")}

    before, c0 = snap(), sim.counters()
    probes = [(5, 0), (17, K)]
    a = sim.view_census(up=plans[-1]["up"], heartbeats=True, probes=probes, per_owner=True, per_row=True)
    b = sim.view_census(up=plans[-1]["up"], heartbeats=True, probes=probes, per_owner=True, per_row=True)
    after, c1 = snap(), sim.counters()
    assert before == after
    assert c0 == c1
    for k in a:
        if hasattr(a[k], "cpu"):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k
    sim.close()


# ---------------------------------------------------------------- 8. slices
@pytest.fixture(scope="module")
def nccl_world1():
    import torch
    import torch.distributed as dist

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


def test_three_slices_give_one_handles_census():
    """Slices are blocks of 64-column multiples, so three of them need more than 256 nodes: 301 nodes give
    128 / 128 / 45 owner columns (the last one ragged in every tail)."""
    import torch

    n, K = 301, 4
    cfg = dict(DEFAULT_CFG)
    kw = dict(init="warm", tombstones=False, fd_ring=False, hist_cap=16, initial_ops=driver.boot_ops(n, K), hb8=True,
              mv8=True)
    ids, keys = synthetic_node_ids(n), key_names(K)
    one = GossipSim(ids, keys, cfg, **kw)
    grp = ShardGroup.in_process(ids, keys, cfg, shards=3, **kw)
    assert [s.ncol for s in grp.slices] == [128, 128, 45]
    plans = driver.prepare(spec_for(n, K, "hb8mv8", seed=21), 4, torch, one.device)
    for r in range(3):
        driver.run_round([one], plans[r])
        driver.run_round(grp.slices, plans[r], group=grp)
    driver.begin([one], plans[3])
    driver.begin(grp.slices, plans[3])
    M = one.region("SELF_MV", torch.int32, (one.np_,)).cpu().numpy()
    probes = [(0, int(M[0])), (127, int(M[127])), (128, int(M[128])), (255, 1), (256, int(M[256])), (300, int(M[300])),
              (300, int(M[300]) + 1)]
    up = plans[3]["up"]
    for u in (None, up):
        a = one.view_census(up=u, heartbeats=True, probes=probes, per_owner=True, per_row=True)
        b = grp.view_census(up=u, heartbeats=True, probes=probes, per_owner=True, per_row=True)
        assert set(a) == set(b)
        for k in a:
            if hasattr(a[k], "cpu"):
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], (k, a[k], b[k])
        assert_census(a, reference(one, None if u is None else u.cpu().numpy(), True, probes), "one handle")
        assert 0 < a["behind"] < a["views"]
    # each slice alone: its own columns (a probe of another slice's owner reaches nobody there)
    for s in grp.slices:
        got = s.view_census(up=up, heartbeats=True, probes=probes, per_owner=True, per_row=True)
        assert_census(got, reference(s, up.cpu().numpy(), True, probes), f"slice {s.shard}")
    one.close()
    for s in grp.slices:
        s.close()


def test_world1_distcomm_gives_the_slices_own_census(nccl_world1):
    import torch

    n, K = 200, 4
    cfg = dict(DEFAULT_CFG)
    one = GossipSim(synthetic_node_ids(n), key_names(K), cfg, init="warm", tombstones=False, fd_ring=False,
                    hist_cap=16, initial_ops=driver.boot_ops(n, K), hb8=True, mv8=True, sliced=True)
    grp = ShardGroup([one], DistComm(), cfg["mtu"])
    plans = driver.prepare(spec_for(n, K, "hb8mv8", seed=2), 3, torch, one.device)
    for r in range(2):
        driver.run_round([one], plans[r], group=grp)
    driver.begin([one], plans[2])
    probes = [(0, K), (199, K), (64, K + 1)]
    up = plans[2]["up"]
    a = one.view_census(up=up, heartbeats=True, probes=probes, per_owner=True, per_row=True)
    b = grp.view_census(up=up, heartbeats=True, probes=probes, per_owner=True, per_row=True)
    assert set(a) == set(b)
    for k in a:
        if hasattr(a[k], "cpu"):
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])
    assert_census(a, reference(one, up.cpu().numpy(), True, probes), "world-1")
    assert a["behind"] > 0
    one.close()

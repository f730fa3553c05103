"""Cut exchanges on the device (gs_run_phase_cut, gs_draw_cuts; GPU only).

1. the reference's fixtures of tools/gen_lossy_fixture.py (state after every round; hook events) in every layout
   that can replay them;
2. legs = NULL and legs all 3 are gs_run_phase, bit for bit;
3. lockstep with the oracle composer of tests/lossycases.py at sizes that reach k_pass1v's second row half, the
   partial last group, the general layout and the wide-key instantiation;
4. a phase of legs 0 changes the responders' own heartbeats and nothing else (the report planes are never
   cleared: a row stamped over stale bits would show in the next liveness sweep);
5. the device draw equals aiocluster_amd.cuts.draw_cuts;
6. refusals: sliced handles, legs values above 3;
7. data still converges under loss, in as many rounds as on the composer.
"""

import ctypes as C

import numpy as np
import pytest
import torch
from helpers import compare_exports, load_scenario, make_backend, replay_and_compare
from lossycases import CutOracleSim, add_legs, cold_lossy, legs_counts, warm_lossy
from test_events import golden_events

from aiocluster_amd import _lib
from aiocluster_amd._lib import GsError
from aiocluster_amd.cuts import draw_cuts_q32, loss_q32
from aiocluster_amd.scenario import make_scenario, replay_round, round_tick
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.workload import WorkloadSpec

pytestmark = pytest.mark.gpu

PREFIX = dict(tombstones=False, fd_ring=False)
LAYOUTS_W = {
    "general": dict(canonical=False),
    "canonical_held": dict(fd_ring=False),
    "prefix": dict(PREFIX),
    "hb8": dict(PREFIX, hb8=True),
    "hb8mv8_esc4": dict(PREFIX, hb8=True, mv8=True, esc_cols=4),
}
# regions that hold no state: counters, per-phase scratch, and the report planes (rows without a stamp are never
# written: GS_R_PEND_STAMP and the windows after the sweep are compared instead)
SCRATCH = {"COUNTERS", "CAND", "CAND_N", "SLICE_BITS", "SLOT_STAT", "PEND", "ESC_REQ"}


# ---------------------------------------------------------------- 1. the reference's fixtures
def replay_fixture(name, **kw):
    scen = load_scenario(name)
    exp = scen["expect"]
    gpu = make_backend(GossipSim, scen, **kw)
    bad = replay_and_compare(gpu, scen, expect_states=exp["states"], expect_hashes=exp["hashes"])
    assert bad is None, f"{name} round {bad[0]}: {bad[1]}"
    c = gpu.check()
    counts = legs_counts(scen)
    assert c["exchanges"] == sum(counts) and c["cut_exchanges"] == sum(counts[:3]) > 0, (c["exchanges"], counts)
    print(f"{name} {kw}: legs {counts}, truncated {c['truncated']}, node_deltas {c['node_deltas']}, "
          f"lite_slots {c['lite_slots']}")
    gpu.close()
    return c


def test_reference_cut8_general_layout_with_rings():
    """Window 5: ring eviction together with Ack-lost cuts, which only the reference pins."""
    c = replay_fixture("cut8", fd_ring=True)
    assert c["truncated"] > 0 and c["tomb_gc"] > 0


def test_reference_cutgc12_general_layout():
    c = replay_fixture("cutgc12")
    assert c["fd_gc"] > 0


@pytest.mark.parametrize("layout", ["general", "canonical_held", "prefix"])
def test_reference_cutw12(layout):
    """21 keys: the wide-key instantiations of the canonical layouts."""
    c = replay_fixture("cutw12", **LAYOUTS_W[layout])
    assert c["truncated"] > 0


@pytest.mark.parametrize("layout", list(LAYOUTS_W))
def test_reference_cutw12s(layout):
    """13 keys (GS_HB8 stops at 16): every layout, the 8-bit ones included."""
    c = replay_fixture("cutw12s", **LAYOUTS_W[layout])
    assert c["truncated"] > 0


def test_reference_events_cut8():
    """A cut phase emits apply records for delivered deltas only, in the reference's order."""
    scen = load_scenario("cut8")
    want = golden_events("cut8")
    gpu = make_backend(GossipSim, scen, fd_ring=True)
    gpu.enable_events()
    kinds = set()
    for r in range(len(scen["rounds"])):
        replay_round(gpu, scen, r)
        got = gpu.drain_events().astype(np.int64).tolist()
        assert got == want[r], f"round {r}: {len(got)} events vs {len(want[r])}"
        kinds |= {e[2] >> 8 for e in got}
    assert 0 in kinds
    gpu.check()
    gpu.close()


# ---------------------------------------------------------------- 2. identity
def run_cut_raw(gpu, t, pairs, legs):
    """gs_run_phase_cut with ``legs`` = None (NULL) or a device tensor."""
    arr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    gpu._flush()
    ini, res = gpu._pairs_dev(arr[:, 0], arr[:, 1])
    gpu._chk(gpu.L.gs_run_phase_cut(gpu.h, C.c_void_p(ini.data_ptr()), C.c_void_p(res.data_ptr()),
                                    C.c_void_p(legs.data_ptr()) if legs is not None else None, len(arr), t),
             "gs_run_phase_cut")


class RawCut:
    """A backend whose phases go through gs_run_phase_cut: ``mode`` "null" (legs = NULL) or "threes"."""

    def __init__(self, gpu, mode):
        self.gpu, self.mode = gpu, mode

    def __getattr__(self, name):
        return getattr(self.gpu, name)

    def run_phase(self, t, pairs):
        if len(pairs) == 0:
            return
        legs = None
        if self.mode == "threes":
            legs = torch.full((len(pairs),), 3, dtype=torch.uint8, device=self.gpu.device)
        run_cut_raw(self.gpu, t, pairs, legs)


def state_regions(gpu):
    out = {}
    for name in gpu.regions:
        if name in SCRATCH:
            continue
        try:
            out[name] = gpu.read_rows(name, 0, gpu.n)
        except GsError:  # a region that is not indexed by observer row (per owner, per write): the whole region
            gpu.sync()
            out[name] = gpu.regions[name].cpu().numpy().tobytes()
    return out


@pytest.mark.parametrize("layout", ["hb8mv8", "prefix"])
def test_null_and_all_three_legs_are_run_phase(layout):
    """N = 1,100 > 1,024 puts columns in k_pass1v's second row half; 1,100 mod 16 != 0 leaves a partial group."""
    kw = dict(PREFIX, hb8=True, mv8=True) if layout == "hb8mv8" else dict(PREFIX)
    spec = WorkloadSpec(n=1100, k=4, fanout=3, seed=31, init="warm", write_frac=0.3)
    scen = make_scenario("ident1100", spec, 2, {"mtu": 1500})
    plain = make_backend(GossipSim, scen, **kw)
    others = {m: RawCut(make_backend(GossipSim, scen, **kw), m) for m in ("null", "threes")}
    for r in range(len(scen["rounds"])):
        replay_round(plain, scen, r)
        want, cw = state_regions(plain), plain.check()
        for m, b in others.items():
            replay_round(b, scen, r)
            got = state_regions(b.gpu)
            assert got.keys() == want.keys()
            for name in want:
                assert got[name] == want[name], f"round {r}, legs {m}: region {name} differs"
            cg = b.gpu.check()
            assert cg["cut_exchanges"] == 0
            for k in cw:
                if k != "cut_exchanges":
                    assert cg[k] == cw[k], (r, m, k, cg[k], cw[k])
    assert cw["truncated"] > 0 and cw["lite_slots"] > 0
    plain.close()
    for b in others.values():
        b.gpu.close()


# ---------------------------------------------------------------- 3. lockstep with the composer
def composer_exports(scen):
    orc = make_backend(CutOracleSim, scen)
    out = []
    for r in range(len(scen["rounds"])):
        replay_round(orc, scen, r)
        out.append(orc.export())
    orc.close()
    return out


def lockstep(scen, want, **kw):
    gpu = make_backend(GossipSim, scen, **kw)
    for r in range(len(scen["rounds"])):
        replay_round(gpu, scen, r)
        diff = compare_exports(gpu.export(), want[r])
        assert diff is None, f"round {r}: device vs composer: {diff}"
    c = gpu.check()
    counts = legs_counts(scen)
    assert c["exchanges"] == sum(counts) and c["cut_exchanges"] == sum(counts[:3])
    assert c["truncated"] > 0
    print(f"{scen['name']} {kw}: legs {counts}, truncated {c['truncated']}, node_deltas {c['node_deltas']}")
    gpu.close()
    return c


@pytest.fixture(scope="module")
def warm1100():
    scen = warm_lossy(rounds=2)
    return scen, composer_exports(scen)


@pytest.mark.parametrize("layout", ["prefix", "hb8mv8_esc4"])
def test_lockstep_warm_1100(warm1100, layout):
    scen, want = warm1100
    lockstep(scen, want, **LAYOUTS_W[layout])


@pytest.mark.parametrize("K", [5, 20])
def test_lockstep_cold_general(K):
    """Cold with deletes and TTL writes, mtu 400, window 1000; K = 20: the wide-key instantiation."""
    scen = cold_lossy(k=K)
    c = lockstep(scen, composer_exports(scen))
    assert c["tomb_gc"] > 0 or c["node_deltas"] > 0


# ---------------------------------------------------------------- 4. all legs 0
DELIVERED = ("hb_reports", "node_deltas", "kvs_sent", "truncated", "delta_bytes", "candidates", "tomb_gc",
             "plane_flushes", "live_pairs")


@pytest.mark.parametrize("layout", ["general", "prefix", "hb8mv8_esc4"])
def test_all_legs_zero_only_raises_the_responders_heartbeats(layout):
    """Two sims run round 0 and the first q phases of round 1; one of them then runs, as phase q of round 1, the
    pairs of round 0's phase q with every leg 0.  That phase takes plane q of exactly the rows that round 0's
    phase q filled with reports.  Only the responders' own heartbeats (GS_R_SELF_HB, the diagonal views) and the
    counters exchanges, cut_exchanges and hb_writes may differ, and the liveness sweep must leave GS_R_FD /
    GS_R_FD_LAST as without that phase: a plane row stamped over round 0's bits would replay them."""
    n = 200
    spec = WorkloadSpec(n=n, k=4, fanout=3, seed=8, init="warm", write_frac=0.3)
    scen = make_scenario("zero200", spec, 2, {"mtu": 1500})
    kw = LAYOUTS_W[layout]
    a, b = make_backend(GossipSim, scen, **kw), make_backend(GossipSim, scen, **kw)
    replay_round(a, scen, 0)
    replay_round(b, scen, 0)
    assert a.counters()["hb_reports"] > 0
    rd = scen["rounds"][1]
    q = min(len(rd["phases"]), len(scen["rounds"][0]["phases"])) // 2
    extra = scen["rounds"][0]["phases"][q]
    assert q > 0 and len(extra) > 0
    responders = sorted({y for _, y in extra})
    t = round_tick(1)
    for g in (a, b):
        for j, k, op, v in rd["writes"]:
            g.write(t, j, k, op, v)
        g.begin_round(t, rd["up"])
        for p, ph in enumerate(rd["phases"][:q]):
            g.run_phase(t + 1 + p, ph)
        if g is b:
            g.run_phase(t + 1 + q, extra, [0] * len(extra))
        g.liveness(t + 2 + q, rd["up"], 1)
    ca, cb = a.check(), b.check()
    for k in ca:
        if k in ("exchanges", "cut_exchanges", "hb_writes"):
            assert cb[k] == ca[k] + len(extra), (k, cb[k], ca[k])
        elif k in DELIVERED or k.startswith("err_"):
            assert cb[k] == ca[k], (k, cb[k], ca[k])
    for name in ("FD", "FD_LAST", "FD_STATE"):
        assert a.read_rows(name, 0, n) == b.read_rows(name, 0, n), name
    ea, eb = a.export(), b.export()
    hb = ea["hb"].copy()
    hb[responders, responders] += 1
    assert np.array_equal(eb["hb"], hb)
    for name in ea:
        if name != "hb":
            assert np.array_equal(ea[name], eb[name]), name
    sa = a.region("SELF_HB", torch.int32, (a.np_,))[:n].cpu().numpy().copy()
    sb = b.region("SELF_HB", torch.int32, (b.np_,))[:n].cpu().numpy()
    sa[responders] += 1
    assert np.array_equal(sa, sb)
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. the device draw
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_device_draw_equals_the_mirror(n):
    spec = WorkloadSpec(n=16, k=2, fanout=2, seed=1, init="warm")
    scen = make_scenario("draw16", spec, 1, {})
    gpu = make_backend(GossipSim, scen, **PREFIX)
    rng = np.random.default_rng(n)
    ini = rng.integers(0, 70000, n).astype(np.int32)
    res = rng.integers(0, 70000, n).astype(np.int32)
    seed = 0xDEADBEEF_0BADF00D
    for loss in (0.0, 0.25, 0.9):
        q = loss_q32(loss)
        got = gpu.draw_cuts(ini, res, seed, 7, 3, q).cpu().numpy()
        assert np.array_equal(got, draw_cuts_q32(ini, res, seed, 7, 3, q)), (n, loss)
    assert (gpu.draw_cuts(ini, res, seed, 7, 3, 0).cpu().numpy() == 3).all()
    gpu.close()


# ---------------------------------------------------------------- 6. refusals
def test_sliced_handle_refuses_legs():
    spec = WorkloadSpec(n=128, k=4, fanout=2, seed=3, init="warm", write_frac=0.2)
    scen = make_scenario("sl128", spec, 1, {})
    gpu = make_backend(GossipSim, scen, sliced=True, **PREFIX)
    rd = scen["rounds"][0]
    gpu.begin_round(round_tick(0), rd["up"])
    legs = torch.full((len(rd["phases"][0]),), 3, dtype=torch.uint8, device=gpu.device)
    with pytest.raises(GsError, match="GS_E_UNSUPPORTED|one-slice"):
        run_cut_raw(gpu, round_tick(0) + 1, rd["phases"][0], legs)
    gpu.close()


@pytest.mark.parametrize("layout", ["general", "prefix", "hb8mv8_esc4"])
def test_legs_value_above_three_is_a_bad_index(layout):
    spec = WorkloadSpec(n=64, k=4, fanout=2, seed=3, init="warm", write_frac=0.5)
    scen = make_scenario("bad64", spec, 2, {})
    kw = LAYOUTS_W[layout]
    gpu, ctl = make_backend(GossipSim, scen, **kw), make_backend(GossipSim, scen, **kw)
    replay_round(gpu, scen, 0)
    replay_round(ctl, scen, 0)
    rd = scen["rounds"][1]
    t = round_tick(1)
    pairs = rd["phases"][0]
    for g in (gpu, ctl):
        for j, k, op, v in rd["writes"]:
            g.write(t, j, k, op, v)
        g.begin_round(t, rd["up"])
    legs = [3] * len(pairs)
    legs[1] = 4
    gpu.run_phase(t + 1, pairs, legs)
    ctl.run_phase(t + 1, pairs[:1] + pairs[2:])
    c = gpu.counters()
    assert c["err_bad_index"] == 1 and c["exchanges"] == ctl.counters()["exchanges"]
    eg, ec = gpu.export(), ctl.export()
    for name in eg:  # the two rows of the bad exchange are unchanged, the others ran
        assert np.array_equal(eg[name], ec[name]), name
    rows = list(pairs[1])
    for name in ("HB", "MV", "FD", "FD_LAST", "ROW"):
        got = np.frombuffer(gpu.read_rows(name, 0, gpu.n), np.uint8).reshape(gpu.n, -1)
        want = np.frombuffer(ctl.read_rows(name, 0, ctl.n), np.uint8).reshape(ctl.n, -1)
        assert np.array_equal(got[rows], want[rows]), name
    gpu.sync()
    ctl.sync()  # the report plane stamps: the bad exchange's rows took no plane
    assert torch.equal(gpu.regions["PEND_STAMP"], ctl.regions["PEND_STAMP"])
    gpu.close()
    ctl.close()


# ---------------------------------------------------------------- 7. convergence under loss
def test_data_converges_under_loss():
    """N = 1,100, loss 0.3: writes for 3 rounds, then quiet rounds until nothing is behind.  The bound on the
    number of rounds is the composer's own count for the same scenario (the same exchanges and cuts: the device
    must need exactly as many), not a constant."""
    spec = WorkloadSpec(n=1100, k=4, fanout=3, seed=55, init="warm", write_frac=0.1, quiet_from=3)
    scen = add_legs(make_scenario("conv1100", spec, 14, {"mtu": 1500}), 0.3)
    orc = make_backend(CutOracleSim, scen)
    bound = None
    for r in range(len(scen["rounds"])):
        replay_round(orc, scen, r)
        if r >= 3:
            mv = orc.export()["mv"]
            if (mv == np.diag(mv)[None, :]).all():
                bound = r + 1
                break
    orc.close()
    assert bound is not None, "the composer did not converge within the scenario"
    gpu = make_backend(GossipSim, scen, **dict(PREFIX, hb8=True, mv8=True))
    rounds = None
    for r in range(bound):
        replay_round(gpu, scen, r)
        if r >= 3 and gpu.view_census()["behind"] == 0:
            rounds = r + 1
            break
    c = gpu.check()  # every err_* is 0
    assert rounds is not None and rounds <= bound, (rounds, bound)
    assert c["cut_exchanges"] > 0
    print(f"converged after {rounds} rounds (composer: {bound}), cut {c['cut_exchanges']} of {c['exchanges']}")
    gpu.close()


# ---------------------------------------------------------------- 8. the round driver under loss
def test_driver_rounds_under_loss():
    """driver.prepare / run_round with WorkloadSpec.loss: the explicit schedule runs the mirror's legs (equal to a
    scenario replay with the same legs); peer-selected rounds draw theirs on the device (gs_draw_cuts)."""
    from aiocluster_amd import driver
    from aiocluster_amd.peers import PeerSelector

    spec = WorkloadSpec(n=300, k=4, fanout=3, seed=21, init="warm", write_frac=0.2, loss=0.25, cut_seed=0xC07)
    scen = add_legs(make_scenario("drv300", spec, 3, {"mtu": 1500}), 0.25, 0xC07)
    kw = dict(PREFIX, hb8=True, mv8=True)
    a, b, s = (make_backend(GossipSim, scen, **kw) for _ in range(3))
    for r in range(3):
        replay_round(a, scen, r)
    # the driver interns its values itself (other ids, the same lengths): compare everything but the value ids
    plans = driver.prepare(spec, 3, torch, b.device)
    for rd in plans:
        driver.run_round([b], rd)
    ea, eb = a.export(), b.export()
    for name in ea:
        if name != "kv_value_id":
            assert np.array_equal(ea[name], eb[name]), name
    ca, cb = a.check(), b.check()
    for k in ("exchanges", "cut_exchanges", "node_deltas", "kvs_sent", "truncated", "delta_bytes", "hb_reports"):
        assert ca[k] == cb[k], (k, ca[k], cb[k])
    assert cb["cut_exchanges"] > 0
    sel = PeerSelector(s, fanout=3, seed=4)
    for rd in driver.prepare(spec, 3, torch, s.device):
        driver.run_round([s], rd, sel=sel)
    cs = s.check()
    frac = cs["cut_exchanges"] / cs["exchanges"]
    sd = (0.578125 * 0.421875 / cs["exchanges"]) ** 0.5  # P(legs < 3) = 1 - 0.75^3
    assert abs(frac - 0.578125) <= 5 * sd, (frac, cs["exchanges"])
    for g in (a, b, s):
        g.close()

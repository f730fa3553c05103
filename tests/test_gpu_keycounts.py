"""Every key count in every layout, against the C oracle (GPU only).

The kernels keep four keys to a 32-bit word and are compiled for 4 words (K <= 16) and for 16 (17 <= K <= 64); the
key regions are strided by KP = round_up(K, 4), the histories by K.  Elsewhere the suite runs K in {2, 4, 8, 16, 64}
only, and K > 16 only in the general layout.  Here the scenarios of tests/keycases.py -- K in {1, 3, 5, 7, 13, 15}
and {17, 20, 33, 47, 63, 64}, each with an mtu that cuts NodeDeltas (tests/test_keycases_host.py) -- run in lockstep
with the oracle in the general layout, the canonical layout with tombstones, canonical prefix views (16-bit and the
8-bit layouts), the version-only layout, through the heavy-slot kernel, and as owner-column slices; the single-view
readers are compared at K = 5 and 37.  After every round the whole export must equal the oracle's, bit for bit; at
the end the counters.

What these cases found: apply_cand stored all KW words of a receiver's HELD row when a prefix view got its first
hole, so with KP / 4 < KW (every K but 13-16 and 61-64) it zeroed the first keys of the views that follow it in the
observer's row (and, past the last column, of the next row).  Only a following view that has holes itself keeps a
HELD row, so it takes many truncated NodeDeltas in one row to see it: the partition scenarios have them.
"""

import os
import random
import subprocess
import sys

import numpy as np
import pytest
from helpers import compare_exports, make_backend
from keycases import KEYS_ALL, KEYS_SMALL, cold, part_prefix, part_tomb, warm_prefix, warm_tomb
from oracle import OracleSim
from test_gpu_parity import lockstep_vs_oracle
from test_gpu_shard import sharded

from aiocluster_amd._lib import GsError
from aiocluster_amd.scenario import DEFAULT_CFG, replay_round
from aiocluster_amd.shard import LocalComm, ShardGroup
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.workload import key_names, synthetic_node_ids

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

STAT_KEYS = ("exchanges", "hb_reports", "node_deltas", "kvs_sent", "truncated", "delta_bytes")
WARM = {"warm": (warm_tomb, warm_prefix), "part": (part_tomb, part_prefix)}


def run(what, scen, **kw):
    """``scen`` on one handle in lockstep with the oracle (every round's export, then the counters)."""
    gpu, orc, c = lockstep_vs_oracle(scen, **kw)
    s = orc.stats()
    for k in STAT_KEYS:
        assert c[k] == s[k], (k, c[k], s[k])
    if scen["k"] != 1:  # with one key a NodeDelta is sent whole or not at all
        assert c["truncated"] > 0
    print(f"{what} K={scen['k']}: truncated {c['truncated']}, tomb_gc {c['tomb_gc']}, node_deltas {c['node_deltas']}, "
          f"kvs_sent {c['kvs_sent']}, lite_slots {c['lite_slots']}")
    orc.close()
    return gpu, c


# ---------------------------------------------------------------- general layout
@pytest.mark.parametrize("K", KEYS_ALL)
def test_general_layout(K):
    gpu, c = run("general", cold(K), fd_ring=True)
    assert not gpu.canonical and c["tomb_gc"] > 0
    gpu.close()


# ---------------------------------------------------------------- canonical layout with tombstones
@pytest.mark.parametrize("K", KEYS_ALL)
@pytest.mark.parametrize("kind", list(WARM))
def test_canonical_with_tombstones(kind, K):
    gpu, c = run(f"canonical tombstones {kind}", WARM[kind][0](K), fd_ring=False)
    assert gpu.canonical and c["tomb_gc"] > 0
    gpu.close()


# ---------------------------------------------------------------- canonical prefix views, 16-bit
@pytest.mark.parametrize("K", KEYS_ALL)
@pytest.mark.parametrize("kind", list(WARM))
def test_canonical_prefix_views(kind, K):
    """k_lite over the version log (round_up(K * (C - 1) + 1, 4) entries), GS_R_LATEST, and the HELD path for the
    views that the mtu left with holes."""
    gpu, c = run(f"prefix {kind}", WARM[kind][1](K), tombstones=False, fd_ring=False)
    if K != 1:
        assert c["lite_slots"] > 0 and gpu.inexact_views() > 0
    gpu.close()


# ---------------------------------------------------------------- 8-bit views (K <= 16)
LAYOUTS8 = {"hb8": dict(hb8=True), "hb8mv8": dict(hb8=True, mv8=True), "esc4": dict(hb8=True, mv8=True, esc_cols=4)}


@pytest.mark.parametrize("layout", list(LAYOUTS8))
@pytest.mark.parametrize("K", KEYS_SMALL)
@pytest.mark.parametrize("kind", list(WARM))
def test_eight_bit_prefix_views(kind, K, layout):
    gpu, c = run(f"{layout} {kind}", WARM[kind][1](K), tombstones=False, fd_ring=False, **LAYOUTS8[layout])
    if K != 1:
        assert c["lite_slots"] > 0 and gpu.inexact_views() > 0
    gpu.close()


def test_hb8_refuses_17_keys():
    """GS_HB8 stops at K = 16 (tests/test_gpu_hb8.py checks K = 20): the first K of the wide kernels must refuse."""
    with pytest.raises(GsError):
        GossipSim(synthetic_node_ids(8), key_names(17), dict(DEFAULT_CFG), "warm", None, tombstones=False, hb8=True)


# ---------------------------------------------------------------- version-only (GS_NO_HELD)
@pytest.mark.parametrize("K", [3, 13, 17, 63])
def test_version_only_layout(K):
    scen = warm_prefix(K, mtu=1 << 30)
    gpu, orc, c = lockstep_vs_oracle(scen, tombstones=False, held=False, fd_ring=False)
    assert "HELD" not in gpu.regions
    s = orc.stats()
    for k in STAT_KEYS:
        assert c[k] == s[k], (k, c[k], s[k])
    assert c["err_holes"] == 0 and c["truncated"] == 0 and c["node_deltas"] > 0
    print(f"version-only K={K}: node_deltas {c['node_deltas']}, kvs_sent {c['kvs_sent']}")
    gpu.close()
    orc.close()


# ---------------------------------------------------------------- heavy-slot kernel
def heavy_run(K):
    """part_prefix(K) with GS_HEAVY_T=48 (read once per process: a child process runs this)."""
    gpu, c = run("heavy", part_prefix(K), tombstones=False, fd_ring=False)
    print("ok heavy_slots %d truncated %d" % (c["heavy_slots"], c["truncated"]))


@pytest.mark.parametrize("K", [5, 15])
def test_heavy_slot_kernel(K):
    """After the heal a node has more than 48 stale owners (the other half): those slots go to k_pack_heavy."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "from test_gpu_keycounts import heavy_run\n"
            "heavy_run(%d)\n") % (HERE, REPO, os.path.join(REPO, "oracle"), K)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GS_HEAVY_T="48"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("ok"), line
    print(r.stdout.strip())
    st = dict(zip(line.split()[1::2], (int(x) for x in line.split()[2::2])))
    assert st["heavy_slots"] > 0 and st["truncated"] > 0, st


# ---------------------------------------------------------------- owner-column slices
def lockstep_three(what, scen, grp, kw):
    """``grp`` (slices) against one handle and against the oracle, every round; then the counters."""
    one = make_backend(GossipSim, scen, **kw)
    orc = make_backend(OracleSim, scen)
    for r in range(len(scen["rounds"])):
        for b in (grp, one, orc):
            replay_round(b, scen, r)
        got, want = grp.export(), orc.export()
        diff = compare_exports(got, want)
        assert diff is None, f"round {r}: slices vs oracle: {diff}"
        diff = compare_exports(got, one.export())
        assert diff is None, f"round {r}: slices vs one handle: {diff}"
    c1, cg, s = one.check(), grp.check(), orc.stats()
    for k in STAT_KEYS:
        assert cg[k] == c1[k] == s[k], (k, cg[k], c1[k], s[k])
    assert cg["tomb_gc"] == c1["tomb_gc"] and cg["truncated"] > 0
    print(f"{what} K={scen['k']}: truncated {cg['truncated']}, tomb_gc {cg['tomb_gc']}, chain_phases "
          f"{grp.chain_phases}")
    one.close()
    orc.close()
    for sl in grp.slices:
        sl.close()
    return cg


@pytest.mark.parametrize("native", [False, True], ids=["shard_py", "library"])
@pytest.mark.parametrize("K", [3, 13, 20, 37, 64])
@pytest.mark.parametrize("tomb", [False, True], ids=["part_prefix", "part_tomb"])
def test_two_slices(tomb, K, native):
    """n = 128 as two slices of 64 columns: gs_phase_count / gs_phase_pack / gs_phase_chain, or the library's
    group driver (one launch per slice past KP = 16), with deltas that the mtu cuts across the slice boundary."""
    scen = (part_tomb if tomb else part_prefix)(K)
    kw = dict(tombstones=tomb, fd_ring=False)
    grp = sharded(scen, 2, native=native, **kw)
    c = lockstep_three(f"slices {'library' if native else 'shard_py'} {'tomb' if tomb else 'prefix'}", scen, grp, kw)
    if tomb:
        assert c["tomb_gc"] > 0
    if not native:
        assert grp.chain_phases > 0  # k_pack_slice and k_chain_step cut a delta across the boundary


def test_one_handle_sliced_with_37_keys():
    """GS_SLICED on a single handle: the sliced phase path with one slice of all 128 columns."""
    scen = part_prefix(37)
    kw = dict(tombstones=False, fd_ring=False)
    one = make_backend(GossipSim, scen, sliced=True, **kw)
    lockstep_three("GS_SLICED", scen, ShardGroup([one], LocalComm(1), scen["config"]["mtu"]), kw)


# ---------------------------------------------------------------- readers
@pytest.mark.parametrize("K", [5, 37])
def test_readers(K):
    """k_materialize and the KP-strided copies: single views (node_state) against the oracle's, and gs_read_rows of
    GS_R_HELD against the whole-matrix readback."""
    scen = part_tomb(K)
    gpu, orc, c = lockstep_vs_oracle(scen, fd_ring=False)
    n = scen["n"]
    rng = random.Random(K)
    for _ in range(8):
        o, j = rng.sample(range(n), 2)
        ns = gpu.node_state(o, j)
        assert (ns.heartbeat, ns.max_version, ns.last_gc_version) == orc.view(o, j), (o, j)
        got = sorted([k, v.value, v.version, int(v.status), v.status_change_ts] for k, v in ns.key_values.items())
        assert got == orc.view_kvs(o, j), (o, j)
    lo, hi = 37, 70
    held = np.frombuffer(gpu.read_rows("HELD", lo, hi), np.uint8).reshape(hi - lo, gpu.np_, gpu.kp)
    assert np.array_equal(held, gpu._host(list(range(lo, hi)))["HELD"])
    assert held[:, :n, K - 1].any()  # the last key, next to the padding of the KP stride
    gpu.close()
    orc.close()

"""Cut exchanges (gs_run_phase_cut): scenario builders and the oracle composer.

TEST INFRASTRUCTURE.  A lossy scenario is an ordinary scenario whose rounds carry ``"legs"``: one list per phase,
parallel to ``"phases"`` -- the messages delivered of each exchange, drawn by ``aiocluster_amd.cuts.draw_cuts``.

``CutOracleSim`` is the checker for cut phases: the C oracle, driven through entry points it already has, so that
a cut exchange leaves exactly what the reference's handlers leave when the exchange stops after ``legs`` messages
(aiocluster/server.py:334-376, 523-568):

    legs 3  ``orc_exchange``
    legs 2  the Ack is lost: a's Syn digest is read, b's row saved (``orc_snapshot_row``), the whole exchange run
            (a ends exactly as after the SynAck: the Ack only changes b), b's row put back
            (``orc_restore_row``), and the Syn alone replayed on b
    legs 1  the Syn alone on b: b's own heartbeat + 1, then ``_report_heartbeat`` (server.py:599-604) for every
            entry of a's digest -- a's known nodes but those scheduled for deletion (327-332), b itself skipped:
            ``orc_kat_apply_heartbeat`` (node_state_or_default + apply_heartbeat) and, where it returns true,
            ``orc_kat_fd_report``
    legs 0  b's own heartbeat + 1 (server.py:524) only

Its one limit: ``orc_snapshot_row`` does not keep the contents of the interval rings, so an Ack-lost cut (legs 2)
is exact only while no sampling window of the responder has rolled over -- scenarios for the composer use a
``window`` that no window reaches (``windows_below_capacity``).  The ring eviction together with Ack-lost cuts is
pinned by the reference itself (tests/golden/scen_cut8.json.gz, window 5).

Its ``stats()`` are the oracle's: under legs 2 they include the Ack delta that was computed and dropped, and the
composed parts are not counted, so they are not compared against the device's counters.
"""

import ctypes as C

import numpy as np
from oracle import TICK_US, OracleSim

from aiocluster_amd.cuts import draw_cuts
from aiocluster_amd.scenario import make_scenario
from aiocluster_amd.workload import WorkloadSpec

CUT_SEED = 0xC07
LOSS = 0.25


def add_legs(scen: dict, loss: float = LOSS, seed: int = CUT_SEED) -> dict:
    """``scen`` with ``"legs"`` drawn for every phase of every round (in place; returns it)."""
    for r, rd in enumerate(scen["rounds"]):
        rd["legs"] = []
        for p, ph in enumerate(rd["phases"]):
            arr = np.asarray(ph, dtype=np.int64).reshape(-1, 2)
            rd["legs"].append([int(x) for x in draw_cuts(arr[:, 0], arr[:, 1], seed, r, p, loss)])
    return scen


def legs_counts(scen: dict) -> list[int]:
    """Exchanges of ``scen`` by legs value."""
    c = [0, 0, 0, 0]
    for rd in scen["rounds"]:
        for lg in rd.get("legs", []):
            for x in lg:
                c[x] += 1
    return c


# ------------------------------------------------------------------ scenarios
CUT8_CFG = {"mtu": 300, "tombstone_grace_s": 3, "window": 5, "max_interval_s": 1.0, "initial_interval_s": 1.0,
            "phi_threshold": 3.0}


def cut8(window: int = 5) -> dict:
    """The trunc8 shape: cold, deletes, TTL writes, mtu 300, up / down churn; window 5 rolls the rings over."""
    spec = WorkloadSpec(n=8, k=8, fanout=2, seed=2, init="cold", write_frac=0.5, delete_frac=0.25, ttl_frac=0.1,
                        down_frac=0.3, down_rounds=4)
    return add_legs(make_scenario("cut8", spec, 40, dict(CUT8_CFG, window=window)))


def cutw12() -> dict:
    """The keys21w shape: warm, 21 keys, no deletes (the prefix-view and 8-bit layouts replay it), mtu 460."""
    spec = WorkloadSpec(n=12, k=21, fanout=2, seed=621, init="warm", write_frac=0.5, down_frac=0.3, down_rounds=4)
    return add_legs(make_scenario("cutw12", spec, 30, {"mtu": 460, "initial_interval_s": 1.0, "phi_threshold": 3.0}))


def cutw12s() -> dict:
    """cutw12 with 13 keys and mtu 300: GS_HB8 stops at 16 keys, so the 8-bit layouts replay this one."""
    spec = WorkloadSpec(n=12, k=13, fanout=2, seed=613, init="warm", write_frac=0.5, down_frac=0.3, down_rounds=4)
    return add_legs(make_scenario("cutw12s", spec, 30, {"mtu": 300, "initial_interval_s": 1.0, "phi_threshold": 3.0}))


def cutgc12() -> dict:
    """The fdgc12 shape: failure-detector garbage collection, remove_node and re-insertion."""
    spec = WorkloadSpec(n=12, k=4, fanout=2, seed=4, init="cold", write_frac=0.25, down_frac=0.3, down_rounds=12)
    return add_legs(make_scenario("cutgc12", spec, 45, {"dead_grace_s": 8.0, "phi_threshold": 2.0,
                                                        "initial_interval_s": 1.0}))


def warm_lossy(n: int = 1100, k: int = 4, rounds: int = 3, mtu: int = 1500, loss: float = LOSS, seed: int = 77) -> dict:
    """Warm prefix-view workload at a size that puts columns in k_pass1v's second row half (n > 1,024) and leaves
    a partial last group (n mod 16 != 0)."""
    spec = WorkloadSpec(n=n, k=k, fanout=3, seed=seed, init="warm", write_frac=0.3)
    return add_legs(make_scenario(f"lossyw{n}", spec, rounds, {"mtu": mtu}), loss)


def cold_lossy(k: int = 5, n: int = 96, rounds: int = 8, mtu: int = 400) -> dict:
    """Cold start with deletes and TTL writes, window 1000 (no window rolls over): the general layout."""
    spec = WorkloadSpec(n=n, k=k, fanout=3, seed=900 + k, init="cold", write_frac=0.3, delete_frac=0.15,
                        ttl_frac=0.1)
    return add_legs(make_scenario(f"lossyc{n}k{k}", spec, rounds, {"mtu": mtu, "tombstone_grace_s": 3,
                                                                 "window": 1000}))


# ------------------------------------------------------------------ the composer
class CutOracleSim(OracleSim):
    """The C oracle with cut exchanges composed from its entry points (see the module docstring)."""

    def __init__(self, *a, **kw):
        kw["threads"] = 1  # the composer drives single exchanges
        super().__init__(*a, **kw)
        self._sched = (C.c_int32 * self.n)()
        self._ord = (C.c_int32 * self.n)()
        self._view = (C.c_uint32 * 3)()
        self.cut_exchanges = 0

    def _digest(self, a: int, now: int):
        """a's Syn digest as [(node, heartbeat)]: compute_digest without the nodes scheduled for deletion."""
        L, h = self.L, self.h
        ns = L.orc_kat_fd_scheduled(h, a, now, self._sched)
        skip = set(self._sched[:ns])
        cnt = L.orc_node_count(h, a)
        L.orc_node_order(h, a, self._ord)
        out = []
        v = self._view
        for j in self._ord[:cnt]:
            if j not in skip:
                L.orc_view(h, a, j, v)
                out.append((j, v[0]))
        return out

    def _syn_only(self, b: int, digest, now: int):
        """b's side of a Syn: inc_heartbeat (server.py:524), then _report_heartbeat over the digest (334-337)."""
        L, h = self.L, self.h
        v = self._view
        L.orc_view(h, b, b, v)
        L.orc_kat_set_view(h, b, b, v[0] + 1, v[1], v[2])
        if digest is None:
            return
        for j, hb in digest:
            if j != b and L.orc_kat_apply_heartbeat(h, b, j, hb):
                L.orc_kat_fd_report(h, b, j, now)

    def run_phase(self, t: int, pairs, legs=None):
        if legs is None:
            return super().run_phase(t, pairs)
        now = t * TICK_US
        L, h = self.L, self.h
        if len(legs) != len(pairs):
            raise ValueError(f"{len(legs)} legs for {len(pairs)} exchanges")
        for (a, b), lg in zip(pairs, legs):
            a, b, lg = int(a), int(b), int(lg)
            if lg == 3:
                L.orc_exchange(h, a, b, now)
                continue
            self.cut_exchanges += 1
            if lg == 0:
                self._syn_only(b, None, now)
                continue
            dg = self._digest(a, now)
            if lg == 2:
                L.orc_snapshot_row(h, b)
                L.orc_exchange(h, a, b, now)
                L.orc_restore_row(h, b)
            self._syn_only(b, dg, now)


def windows_below_capacity(orc: OracleSim, window: int) -> bool:
    """No sampling window of ``orc`` holds ``window`` intervals yet (the composer's limit)."""
    return int(orc.export()["fd_len"].max()) < window

"""Scenarios with many phases per round and several phases at one tick (sub-phases).

``Workload`` makes rounds of 3 x fanout matchings, one per tick.  The reference's own peer selection needs more
phases than a round has ticks, and runs several of them at one time (sub-phases); the device then
keeps more reports per round than one base of report planes holds (GS_PLANES = 32) and replays them mid-round.  The
builders here post-process a finished ``make_scenario`` dict so that small clusters reach all of that:

* ``chunk_phases(scen, sizes)`` cuts every matching into consecutive chunks (a subset of a matching is a matching),
  with a chunk size that cycles by round, so rounds of very different phase counts follow one another;
* ``with_ticks(scen, kind)`` sets each round's ``"ticks"`` (``aiocluster_amd.scenario.round_ticks``) to one of the
  maps of ``TICK_MAPS``.

Used by ``oracle/gen_golden.py`` (fixtures ``scen_subring24``, ``scen_subfront40``), ``tests/test_manyphases_host.py``
and ``tests/test_gpu_subphases.py``.
"""

from aiocluster_amd.scenario import make_scenario
from aiocluster_amd.workload import MAX_PHASES_PER_ROUND, WorkloadSpec

PLANES = 32  # GS_PLANES (include/gossip_sim.h): report planes, i.e. phases, per plane base
LAST = MAX_PHASES_PER_ROUND - 1  # offset of the budget's last phase tick, less one

# phase index -> tick offset from the round's start
TICK_MAPS = {
    # workload.phase_tick: one phase per tick, those past the budget at its last tick
    "budget": lambda p: 1 + min(p, LAST),
    # three phases per tick: every tick has sub-phases, and every new tick after them forces a replay and a new base
    "triples": lambda p: 1 + min(p // 3, LAST),
    # the first 41 phases at the round's first tick (more than GS_PLANES sub-phases at once), then one per tick
    "front": lambda p: 1 + max(0, min(p - 40, LAST)),
}


def chunk_phases(scen: dict, sizes) -> dict:
    """Cut, in place, every phase of round r into consecutive chunks of ``sizes[r % len(sizes)]`` pairs, in order:
    no phase is empty (an empty matching disappears) and no exchange is lost.  Returns ``scen``."""
    for r, rd in enumerate(scen["rounds"]):
        size = int(sizes[r % len(sizes)])
        assert size >= 1
        rd["phases"] = [ph[i:i + size] for ph in rd["phases"] for i in range(0, len(ph), size)]
    return scen


def with_ticks(scen: dict, kind) -> dict:
    """Set, in place, every round's ``"ticks"`` from ``TICK_MAPS[kind]`` (a tuple of kinds alternates by round);
    the liveness sweep is one tick after the last phase.  Returns ``scen``."""
    kinds = (kind,) if isinstance(kind, str) else tuple(kind)
    for r, rd in enumerate(scen["rounds"]):
        f = TICK_MAPS[kinds[r % len(kinds)]]
        offs = [f(p) for p in range(len(rd["phases"]))]
        rd["ticks"] = offs + [(offs[-1] if offs else 0) + 1]
    return scen


# ---------------------------------------------------------------- golden fixtures (oracle/gen_golden.py)
def _golden_spec(n: int, seed: int) -> WorkloadSpec:
    return WorkloadSpec(n=n, k=8, fanout=3, seed=seed, init="cold", write_frac=0.3, delete_frac=0.15, ttl_frac=0.1,
                        down_frac=0.2, down_rounds=3)


def subring24() -> dict:
    """24 nodes, cold, deletes + TTL writes + churn; ring windows of 5 that roll over, max_interval 0.25 s (16
    ticks: intervals between the reports of one round are dropped or kept), three phases per tick."""
    cfg = {"window": 5, "max_interval_s": 0.25, "initial_interval_s": 1.0, "phi_threshold": 3.0, "mtu": 400,
           "tombstone_grace_s": 3, "dead_grace_s": 8}
    scen = make_scenario("subring24", _golden_spec(24, 24), 9, cfg)
    return with_ticks(chunk_phases(scen, (1, 4, 2)), "triples")


def subfront40() -> dict:
    """40 nodes, the same workload with compact-window defaults; rounds of about 95 / 48 / 14 phases, alternately
    with the first 41 at the round's first tick and with those past the budget at its last."""
    cfg = {"mtu": 900, "phi_threshold": 3.0, "initial_interval_s": 1.0}
    scen = make_scenario("subfront40", _golden_spec(40, 40), 9, cfg)
    return with_ticks(chunk_phases(scen, (1, 2, 8)), ("front", "budget"))


# ---------------------------------------------------------------- device-vs-oracle scenarios (GPU tests)
ROUNDS = 9
MAX_INTERVAL_TICKS = 16  # max_interval_s 0.25

# layout -> (workload overrides, config, GossipSim keywords, ring windows on every row?)
LAYOUTS = {
    # 16-bit views, tombstones, general (cold) layout; ring windows, short max_interval
    "general": (dict(init="cold", delete_frac=0.15, ttl_frac=0.1),
                {"tombstone_grace_s": 2, "window": 5, "max_interval_s": 0.25, "mtu": 700},
                dict(fd_ring=True), True),
    # 16-bit views, canonical warm, prefix views, compact windows
    "canonical": (dict(), {"mtu": 900}, dict(tombstones=False, fd_ring=False), False),
    # 8-bit heartbeats only: ring windows, short max_interval
    "hb8": (dict(), {"window": 6, "max_interval_s": 0.25, "mtu": 800}, dict(hb8=True, fd_ring=True), True),
    # the headline layout (k_pass1v, 16-column report planes), binding mtu
    "hb8mv8": (dict(), {"mtu": 800}, dict(tombstones=False, fd_ring=False, hb8=True, mv8=True), False),
    # the same with sampled rings: a small window, interval rings on RING_ROWS only
    "sampled": (dict(), {"mtu": 800, "window": 6}, dict(tombstones=False, fd_ring=False, hb8=True, mv8=True), False),
}
RING_ROWS = (3, 17, 64, 90, 127)  # the sampled layout's ring rows (n = 128)
CHUNKS = (3, 7, 32)  # at 128 nodes a matching has ~40 pairs: rounds of ~125 / ~55 / ~15 phases


def device_scenario(layout: str, kind: str, n: int = 128, rounds: int = ROUNDS, chunks=CHUNKS, **cfg_over) -> dict:
    """The scenario of the GPU tests' ``layout`` under tick map ``kind``: k = 8, fanout 3, writes 0.3, 8 % of the
    nodes down for 3 rounds each."""
    over, cfg, _, _ = LAYOUTS[layout]
    kw = dict(n=n, k=8, fanout=3, seed=n + len(layout), init="warm", write_frac=0.3, down_frac=0.08, down_rounds=3)
    kw.update(over)
    c = {"phi_threshold": 3.0, "initial_interval_s": 1.0}
    c.update(cfg)
    c.update(cfg_over)
    scen = make_scenario(f"sub_{layout}_{kind}_{n}", WorkloadSpec(**kw), rounds, c)
    return with_ticks(chunk_phases(scen, chunks), kind)


def sliced_scenario(row: str, kind: str, n: int) -> dict:
    """The sliced GPU tests' scenarios: ``row`` = "py" (shard.py's driver: tombstones, ring windows), "native"
    (gs_run_phase_group per slice: tombstones) or "batched" (its batched path: 8-bit views, no tombstones); all warm
    (sliced phases need the canonical layout) with a binding mtu, so chain steps run."""
    tomb = row != "batched"
    kw = dict(n=n, k=8, fanout=3, seed=n + len(row), init="warm", write_frac=0.3, down_frac=0.08, down_rounds=3,
              delete_frac=0.1 if tomb else 0.0, ttl_frac=0.05 if tomb else 0.0)
    cfg = {"phi_threshold": 3.0, "initial_interval_s": 1.0, "mtu": 1200 if tomb else 900, "tombstone_grace_s": 2}
    if row == "py":
        cfg["window"] = 6
    scen = make_scenario(f"sub_{row}_{kind}_{n}", WorkloadSpec(**kw), ROUNDS, cfg)
    # a matching of n nodes has ~n/3 pairs: the same phases per round at 128 and at 256 nodes
    return with_ticks(chunk_phases(scen, tuple(c * n // 128 for c in CHUNKS)), kind)


SLICED_KW = {
    "py": dict(tombstones=True, fd_ring=True),
    "native": dict(tombstones=True, fd_ring=False),
    "batched": dict(tombstones=False, fd_ring=False, hb8=True, mv8=True),
}


# ---------------------------------------------------------------- what a schedule asks of the report planes
def rounds_past_a_base(scen: dict) -> int:
    """Rounds with more phases than one plane base holds: each needs at least one mid-round replay."""
    return sum(len(rd["phases"]) > PLANES for rd in scen["rounds"])


def ticks_after_subphases(scen: dict) -> int:
    """Distinct (round, tick) pairs that hold a phase and follow a tick with two or more phases: each is a forced
    replay (a base whose planes clamp to the shared tick cannot take a later tick)."""
    total = 0
    for rd in scen["rounds"]:
        offs = rd["ticks"][:-1]
        ticks = sorted(set(offs))
        total += sum(offs.count(a) > 1 for a in ticks[:-1])
    return total


# every scenario the GPU tests replay (tests/test_manyphases_host.py checks each one's properties on the oracle)
DEVICE_CASES = [(layout, kind) for layout in LAYOUTS for kind in TICK_MAPS]
SLICED_CASES = [(row, kind, n) for row in SLICED_KW for kind in ("budget", "triples") for n in (128, 256)]


class Tap:
    """The oracle, noting after every phase whether it cut a delta (stats()["truncated"] rose) and whether the phase
    was a sub-phase (at the previous phase's tick)."""

    def __init__(self, orc):
        self.orc, self.cut, self.sub, self.prev = orc, [], [], None
        self.seen = orc.stats()["truncated"]

    def write(self, *a):
        self.orc.write(*a)

    def begin_round(self, t, up):
        self.prev = None
        self.orc.begin_round(t, up)

    def run_phase(self, t, pairs):
        self.orc.run_phase(t, pairs)
        now = self.orc.stats()["truncated"]
        self.cut.append(now > self.seen)
        self.sub.append(t == self.prev)
        self.seen, self.prev = now, t

    def liveness(self, t, up, r=-1):
        self.orc.liveness(t, up, r)

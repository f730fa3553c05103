"""Golden fixtures of cut exchanges from the REAL reference -- build container only.

TEST INFRASTRUCTURE (see ``oracle/refharness.py``).  ``CutRefSim`` drives the reference's own handlers and stops an
exchange after ``legs`` messages (aiocluster/server.py:378-439, 523-568): the responder's ``inc_heartbeat`` always
runs (524), ``_handle_syn_msg`` if the Syn arrived, ``_handle_synac_msg`` if the SynAck did, ``_handle_ack`` if the
Ack did.  Writes, under ``tests/golden/`` (scenarios of ``tests/lossycases.py``, legs drawn by
``aiocluster_amd.cuts.draw_cuts`` at loss 0.25, the reference's full state after every round):

* ``scen_cut8.json.gz``    -- cold, deletes, TTL writes, mtu 300, window 5: ring eviction together with Ack-lost
  cuts; ``expect_w1000`` holds the states of the same scenario rerun with window 1000 (which the oracle composer
  of tests/lossycases.py can replay);
* ``scen_cutw12.json.gz``  -- warm, 21 keys, no deletes (the canonical and prefix-view layouts replay it), and
  ``scen_cutw12s.json.gz``, the same with 13 keys (the 8-bit layouts, which stop at 16 keys, replay it too);
* ``scen_cutgc12.json.gz`` -- failure-detector garbage collection and re-insertion;
* ``events_cut8.json.gz``  -- the reference's hook events per round of ``scen_cut8`` (the callbacks and the
  canonical order of ``oracle/gen_events_fixture.py``).

Run:  python tools/gen_lossy_fixture.py
"""

from __future__ import annotations

import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from gen_events_fixture import canonical_liveness  # noqa: E402
from gen_golden import write_gz  # noqa: E402
from lossycases import cut8, cutgc12, cutw12, cutw12s, legs_counts  # noqa: E402
from refharness import RefSim, dt_tick  # noqa: E402

from aiocluster_amd.scenario import initial_by_owner, replay_round, scenario_node_ids, state_hash  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
GENERATOR = "tools/gen_lossy_fixture.py via oracle/refharness.py (reference @ /root/reference)"


class CutRefSim(RefSim):
    """The reference with exchanges that stop after ``legs`` messages."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.trunc_by_legs = [0, 0, 0, 0]  # delivered NodeDeltas that the mtu cut, by the exchange's legs

    def run_phase(self, t: int, pairs, legs=None):
        self.set_time(t)
        for e, (a, b) in enumerate(pairs):
            self.exchange(a, b, 3 if legs is None else legs[e])

    def _count_trunc(self, sender, packet_delta, legs):
        """NodeDeltas of a delivered delta that carry fewer kvs than the sender holds past the receiver's version."""
        byname = {nid.name: nid for nid in self.ids}
        for nd in packet_delta.node_deltas:
            ns = sender._cluster_state._node_states[byname[nd.node_id.name]]
            stale = sum(1 for vv in ns.key_values.values() if vv.version > nd.from_version_excluded)
            if len(nd.key_values) < stale:
                self.trunc_by_legs[legs] += 1

    def exchange(self, a: int, b: int, legs: int = 3):
        PacketPb = self.R.pb.PacketPb
        A, B = self.clusters[a], self.clusters[b]
        syn = PacketPb.FromString(A._make_syn_msg().SerializeToString())
        B.self_node_state().inc_heartbeat()
        if legs < 1:
            return
        synack = PacketPb.FromString(B._handle_syn_msg(syn).SerializeToString())
        if legs < 2:
            return
        self._count_trunc(B, synack.synack.delta, legs)
        ack = PacketPb.FromString(A._handle_synac_msg(synack).SerializeToString())
        if legs < 3:
            return
        self._count_trunc(A, ack.ack.delta, legs)
        B._handle_ack(ack)


def hook_events(ref: CutRefSim, keys, events: list):
    kidx = {k: i for i, k in enumerate(keys)}

    def hook(o):
        c = ref.clusters[o]

        def key_change(node_id, key, old_vv, new_vv):
            events.append([o, ref.idx[node_id], kidx[key], 0 if old_vv is None else old_vv.version, new_vv.version,
                           dt_tick(ref.now)])

        def join(node_id):
            events.append([o, ref.idx[node_id], 1 << 8, 0, 0, dt_tick(ref.now)])

        def leave(node_id):
            events.append([o, ref.idx[node_id], 2 << 8, 0, 0, dt_tick(ref.now)])

        c._emit_key_change = key_change
        c._emit_node_join = join
        c._emit_node_leave = leave

    for o in range(len(ref.clusters)):
        hook(o)


def run(scen: dict, events: bool = False):
    ref = CutRefSim(scenario_node_ids(scen), scen["keys"], scen["config"], scen["init"], initial_by_owner(scen))
    ev, per_round, states, hashes = [], [], [], []
    if events:
        hook_events(ref, scen["keys"], ev)
    for r in range(len(scen["rounds"])):
        replay_round(ref, scen, r)
        st = ref.state()
        states.append(st)
        hashes.append(state_hash(st))
        per_round.append(canonical_liveness(ev))
        ev.clear()
    expect = {"hashes": hashes, "states": states, "final": states[-1], "q9": ref.q9_events, "generator": GENERATOR}
    return expect, per_round, ref


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    for make in (cut8, cutw12, cutw12s, cutgc12):
        scen = make()
        name = scen["name"]
        counts = legs_counts(scen)
        assert min(counts) >= 20, (name, counts)
        scen["expect"], per_round, ref = run(scen, events=name == "cut8")
        if name == "cut8":
            assert ref.trunc_by_legs[2] > 0 and ref.trunc_by_legs[3] > 0, ref.trunc_by_legs
            wide = copy.deepcopy(scen)
            del wide["expect"]
            wide["config"]["window"] = 1000
            scen["expect_w1000"] = run(wide)[0]
            path = os.path.join(GOLDEN, "events_cut8.json.gz")
            write_gz(path, per_round)
            print("events_cut8", sum(len(x) for x in per_round), "events", os.path.getsize(path), "bytes")
        path = os.path.join(GOLDEN, f"scen_{name}.json.gz")
        write_gz(path, scen)
        print(name, "legs", counts, "truncated by legs", ref.trunc_by_legs, "q9", len(ref.q9_events),
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

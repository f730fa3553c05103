"""Wire bytes of the REAL reference (fixture generation only; build container, imports /root/reference
via refharness).  TEST INFRASTRUCTURE: nothing on the GPU box or in the product path runs it.

For rounds of golden scenarios, after the round's liveness sweep (the harness clock at the liveness
tick), and for ordered pairs (s, r) of up nodes:

* ``syn``   = ``clusters[s]._make_syn_msg().SerializeToString()`` (server.py:327-332): PacketPb
              {cluster_id, syn {digest = s.compute_digest(s's scheduled_for_deletion)}};
* ``delta`` = ``clusters[s]._cluster_state.compute_partial_delta_respecting_mtu(digest of r's Syn,
              mtu, s's scheduled_for_deletion).to_pb().SerializeToString()`` (server.py:339-345,
              state.py:340-415): the DeltaPb s would put in its SynAck to r.

Nothing is mutated (no _handle_* call).  Output: tests/golden/wire_<name>.json.gz =
{"tick": {round: liveness tick}, "cases": [[round, s, r, syn hex, delta hex], ...], "truncated": [indices of
the cases in which the mtu cut a NodeDelta: it carries fewer kvs than in the delta without an mtu]}.

Run:  python oracle/gen_wire_fixture.py [names...]
"""

from __future__ import annotations

import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from gen_golden import write_gz  # noqa: E402
from refharness import RefSim  # noqa: E402

from aiocluster_amd.scenario import initial_by_owner, replay_round, scenario_node_ids  # noqa: E402
from aiocluster_amd.workload import liveness_tick  # noqa: E402

# scenario -> (rounds to capture, max pairs per round[, half of them with a receiver that is down])
PLAN = {"trunc8": (None, 64), "sched16": (None, 48), "fdgc12": (None, 40), "simple3": (None, 9),
        "cold64": ([0, 1, 2, 5, 10, 20, 39], 48),
        # large values (tests/bigvalues.py): few cases, each delta up to the mtu.  bigsleep12's senders answer the
        # nodes that are away (a Syn built from the sleeper's state as it stands: nothing is mutated), so whole
        # NodeDeltas past 65,535 bytes and the mtu's cut are in the bytes
        "bigval6": ([0, 1, 4, 10], 30), "bigsleep12": ([2, 4, 5], 6, True),
        # 5, 37 and 21 keys (odd K, and the 16-word key arrays partly used)
        "keys5": (None, 24), "keys37": (None, 24), "keys21w": (None, 24)}


def capture(name):
    from helpers import load_scenario

    scen = load_scenario(name)
    rounds, per, *down_too = PLAN[name]
    nr = len(scen["rounds"])
    rounds = list(range(nr)) if rounds is None else [r for r in rounds if r < nr]
    ref = RefSim(scenario_node_ids(scen), scen["keys"], scen["config"], scen["init"], initial_by_owner(scen))
    R = ref.R
    mtu = scen["config"]["mtu"]
    rng = random.Random(name)
    cases, ticks, truncated = [], {}, []
    for r in range(nr):
        replay_round(ref, scen, r)
        if r not in rounds:
            continue
        up = [o for o, u in enumerate(scen["rounds"][r]["up"]) if u]
        pairs = [(s, q) for s in up for q in up if s != q]
        down = [o for o, u in enumerate(scen["rounds"][r]["up"]) if not u]
        if down_too and down:
            pairs = rng.sample([(s, q) for s in up for q in down], per // 2) + rng.sample(pairs, per - per // 2)
        elif len(pairs) > per:
            pairs = rng.sample(pairs, per)
        t = liveness_tick(r, len(scen["rounds"][r]["phases"]))
        ref.set_time(t)
        ticks[r] = t
        for s, q in pairs:
            cs, cq = ref.clusters[s], ref.clusters[q]
            syn_q = cq._make_syn_msg()
            syn_s = cs._make_syn_msg()
            sched = set(cs._failure_detector.scheduled_for_deletion_nodes())
            delta = cs._cluster_state.compute_partial_delta_respecting_mtu(
                digest=R.state.Digest.from_pb(syn_q.syn.digest), mtu=mtu, scheduled_for_deletion=sched)
            whole = cs._cluster_state.compute_partial_delta_respecting_mtu(
                digest=R.state.Digest.from_pb(syn_q.syn.digest), mtu=1 << 40, scheduled_for_deletion=sched)
            nkv = {nd.node_id: len(nd.key_values) for nd in whole.node_deltas}
            if any(len(nd.key_values) < nkv[nd.node_id] for nd in delta.node_deltas):
                truncated.append(len(cases))
            cases.append([r, s, q, syn_s.SerializeToString().hex(), delta.to_pb().SerializeToString().hex()])
    return {"tick": ticks, "cases": cases, "truncated": truncated}


def main(argv):
    for name in argv or PLAN:
        out = capture(name)
        path = os.path.join(REPO, "tests", "golden", f"wire_{name}.json.gz")
        write_gz(path, out)
        nb = sum(len(c[4]) // 2 for c in out["cases"])
        print(name, len(out["cases"]), "cases", len(out["truncated"]), "truncated", nb, "delta bytes",
              os.path.getsize(path), "bytes on disk")


if __name__ == "__main__":
    main(sys.argv[1:])

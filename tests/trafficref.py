"""gs_traffic_census restated in plain Python over an exported state.

TEST INFRASTRUCTURE.  The input is an ``export()`` dict (``GossipSim.export`` or the oracle's: ``pos`` = dict position
or -1, ``hb`` / ``mv`` / ``gc`` per view, ``kv_version`` / ``kv_status`` / ``kv_value_id`` per key, ``tod`` = time of
death in ticks or -1) taken right before the phase.  The rules are the reference's:

* the Syn digest is ``compute_digest`` (``state.py:324-331``): the initiator's known owners in dict order, without
  its targets scheduled for deletion (``failure_detector.py:121-128``);
* the SynAck digest is the responder's, taken after its own ``inc_heartbeat`` (``server.py:524``) and after
  ``_report_heartbeat`` over the Syn digest (``server.py:334-340``, ``state.py:280-287``): its own heartbeat + 1, the
  larger heartbeat for an owner of the Syn digest, and an owner it did not know appended with the initiator's
  heartbeat, last_gc 0 and max_version 0;
* a delta is ``compute_partial_delta_respecting_mtu`` (``state.py:340-415``) with sizes from ``pbsize``;
* the Ack delta is computed on the initiator's pre-exchange views (the two deltas commute);
* packets and frames are ``wire.packet_size`` / ``frame_size``; a frame is refused when its packet exceeds the mtu
  (``_read_message``, ``server.py:502-514``).
"""

import numpy as np

from aiocluster_amd.pbsize import kv_size_from_lens, msg_field, u_field, vlen
from aiocluster_amd.sim import sched_delay_ticks
from aiocluster_amd.wire import frame_size, packet_size

KINDS = ("syn", "synack", "ack")
BUCKETS = 32


def row(ex, name: str, o: int):
    """Observer ``o``'s row of an export field.  An export of some rows only (``export_rows``) carries ``"rows"``, the
    observers its rows belong to."""
    rows = ex.get("rows")
    if rows is None:
        return ex[name][o]
    i = ex.setdefault("_index", {int(r): i for i, r in enumerate(rows)})
    return ex[name][i[int(o)]]


def bucket(x: int) -> int:
    """GS_TC_BUCKETS: bucket 0 holds 0, bucket b >= 1 holds 2^(b-1) <= x < 2^b."""
    return min(BUCKETS - 1, int(x).bit_length())


class TrafficRef:
    def __init__(self, nid_sizes, key_lens, values, cfg: dict, cluster_id: str = "default-cluster"):
        """``values``: the backend's interned value table (index = value id)."""
        self.nid = [int(x) for x in nid_sizes]
        self.key_lens = [int(x) for x in key_lens]
        self.values = values
        self.mtu = int(cfg["mtu"])
        self.delay = sched_delay_ticks(float(cfg["dead_grace_s"]))
        self.cluster_id = cluster_id

    # ------------------------------------------------------------------ digests
    def scheduled(self, ex, o: int, t: int) -> np.ndarray:
        tod = np.asarray(row(ex, "tod", o)).astype(np.int64)
        return (tod >= 0) & (t - tod >= self.delay)

    def order(self, ex, o: int) -> list[int]:
        pos = np.asarray(row(ex, "pos", o))
        known = np.flatnonzero(pos >= 0)
        return [int(j) for j in known[np.argsort(pos[known], kind="stable")]]

    def digest(self, ex, o: int, t: int) -> dict:
        """{owner: (heartbeat, last_gc, max_version)} in dict order."""
        sch = self.scheduled(ex, o, t)
        hb, gc, mv = row(ex, "hb", o), row(ex, "gc", o), row(ex, "mv", o)
        return {j: (int(hb[j]), int(gc[j]), int(mv[j])) for j in self.order(ex, o) if not sch[j]}

    def synack_digest(self, ex, a: int, b: int, t: int, syn: dict) -> dict:
        sch = self.scheduled(ex, b, t)
        hbb, gcb, mvb = row(ex, "hb", b), row(ex, "gc", b), row(ex, "mv", b)
        views = {j: [int(hbb[j]), int(gcb[j]), int(mvb[j])] for j in self.order(ex, b)}
        views[b][0] += 1  # inc_heartbeat
        for j, (hb, _, _) in syn.items():  # _report_heartbeat
            if j == b:
                continue
            v = views.get(j)
            if v is None:
                views[j] = [hb, 0, 0]  # node_state_or_default, then apply_heartbeat over a 0
            elif hb > v[0]:
                v[0] = hb
        return {j: tuple(v) for j, v in views.items() if not sch[j]}

    def digest_size(self, dg: dict) -> int:
        return sum(msg_field(msg_field(self.nid[j]) + u_field(h) + u_field(g) + u_field(m)) for j, (h, g, m) in dg.items())

    # ------------------------------------------------------------------ deltas
    def delta_size(self, ex, s: int, dg: dict, t: int) -> int:
        sch = self.scheduled(ex, s, t)
        mvs, gcs = row(ex, "mv", s), row(ex, "gc", s)
        kver, kst, kvid = row(ex, "kv_version", s), row(ex, "kv_status", s), row(ex, "kv_value_id", s)
        S = 0
        for j in self.order(ex, s):
            if sch[j]:
                continue
            _, dgc, dmv = dg.get(j, (0, 0, 0))
            ms, gs = int(mvs[j]), int(gcs[j])
            if ms <= dmv:
                continue
            frm = 0 if (dgc < gs and dmv < gs) else dmv
            if ms <= frm:
                continue
            kvs = []
            for k in range(len(self.key_lens)):
                ver = int(kver[j, k])
                if ver > frm:
                    vl = len(self.values[int(kvid[j, k])].encode())
                    kvs.append((ver, kv_size_from_lens(self.key_lens[k], vl, ver, int(kst[j, k]))))
            if not kvs:
                continue
            kvs.sort()
            base = msg_field(self.nid[j]) + u_field(frm) + u_field(gs) + 1 + vlen(ms)
            body, sel = 0, 0
            for _, sz in kvs:
                if S + msg_field(base + body + msg_field(sz)) > self.mtu:
                    break
                body += msg_field(sz)
                sel += 1
            if sel:
                S += msg_field(base + body)
            if S >= self.mtu:
                break
        return S

    # ------------------------------------------------------------------ exchanges and phases
    def exchange(self, ex, a: int, b: int, t: int) -> list[int]:
        """[Syn digest, SynAck digest, SynAck delta, Ack delta] body bytes of a -> b."""
        syn = self.digest(ex, a, t)
        synack = self.synack_digest(ex, a, b, t, syn)
        return [self.digest_size(syn), self.digest_size(synack), self.delta_size(ex, b, syn, t),
                self.delta_size(ex, a, synack, t)]

    def packets(self, m) -> list[int]:
        c = self.cluster_id
        return [packet_size("syn", digest_len=m[0], cluster_id=c),
                packet_size("synack", digest_len=m[1], delta_len=m[2], cluster_id=c),
                packet_size("ack", delta_len=m[3], cluster_id=c)]

    def outcome(self, m, legs: int = 3, frame_limit: bool = False):
        """(sent[3], delivered[3], legs_out) of an exchange with body sizes ``m``."""
        pk = self.packets(m)
        sent, dlv, go = [], [], True
        for k in range(3):
            sent.append(go)
            go = go and legs > k and not (frame_limit and pk[k] > self.mtu)
            dlv.append(go)
        return sent, dlv, sum(dlv)

    def phase(self, ex, pairs, t: int, legs=None, frame_limit: bool = False) -> dict:
        n_nodes = np.asarray(ex["pos"]).shape[1]
        tot = {"exchanges": 0, "bad_index": 0, "digest_bytes_sent": 0, "delta_bytes_sent": 0, "delta_bytes_delivered": 0,
               "max_frame": [0, 0, 0], "frame_hist": [[0] * BUCKETS for _ in range(3)]}
        for k in ("sent", "delivered", "lost", "rejected", "bytes_sent", "bytes_delivered"):
            tot[k] = [0, 0, 0]
        msg, legs_out, pkts = [], [], []
        nodes = np.zeros((2, n_nodes), dtype=np.int64)
        for e, (a, b) in enumerate(pairs):
            a, b = int(a), int(b)
            lg = 3 if legs is None else int(legs[e])
            if not (0 <= a < n_nodes and 0 <= b < n_nodes) or a == b or lg > 3:
                tot["bad_index"] += 1
                msg.append([0, 0, 0, 0])
                legs_out.append(0)
                pkts.append([None, None, None])
                continue
            m = self.exchange(ex, a, b, t)
            sent, dlv, lo = self.outcome(m, lg, frame_limit)
            pk = self.packets(m)
            fr = [frame_size("syn", digest_len=m[0], cluster_id=self.cluster_id),
                  frame_size("synack", digest_len=m[1], delta_len=m[2], cluster_id=self.cluster_id),
                  frame_size("ack", delta_len=m[3], cluster_id=self.cluster_id)]
            msg.append(m)
            legs_out.append(lo)
            pkts.append([pk[k] if sent[k] else None for k in range(3)])
            tot["exchanges"] += 1
            snd, rcv = (a, b, a), (b, a, b)
            for k in range(3):
                if not sent[k]:
                    continue
                tot["sent"][k] += 1
                tot["bytes_sent"][k] += fr[k]
                tot["max_frame"][k] = max(tot["max_frame"][k], fr[k])
                tot["frame_hist"][k][bucket(fr[k])] += 1
                nodes[0, snd[k]] += fr[k]
                if dlv[k]:
                    tot["delivered"][k] += 1
                    tot["bytes_delivered"][k] += fr[k]
                    nodes[1, rcv[k]] += fr[k]
                elif lg <= k:
                    tot["lost"][k] += 1
                else:
                    tot["rejected"][k] += 1
            tot["digest_bytes_sent"] += m[0] + (m[1] if sent[1] else 0)
            tot["delta_bytes_sent"] += (m[2] if sent[1] else 0) + (m[3] if sent[2] else 0)
            tot["delta_bytes_delivered"] += (m[2] if dlv[1] else 0) + (m[3] if dlv[2] else 0)
        body = tot["digest_bytes_sent"] + tot["delta_bytes_sent"]
        tot["digest_share"] = tot["digest_bytes_sent"] / body if body else 0.0
        return {"msg": msg, "legs_out": legs_out, "packets": pkts, "nodes": nodes, "totals": tot}


def for_backend(backend, scen: dict, cluster_id: str = "default-cluster") -> TrafficRef:
    """The reference for a scenario backend (``GossipSim`` or the oracle: both intern values in write order)."""
    from aiocluster_amd.pbsize import nodeid_size

    nid = [nodeid_size(n[0], n[1], n[2], n[3], n[4]) for n in scen["nodes"]]
    return TrafficRef(nid, [len(k.encode()) for k in scen["keys"]], backend.values, scen["config"], cluster_id)

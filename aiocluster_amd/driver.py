"""Round driver shared by the bench, the full-size parity tests and the config-5 tool.

``prepare`` turns a seeded ``Workload`` (``workload.py``) into per-round device inputs (write
batches, up masks, phase arrays) uploaded before any timing; ``run_round`` drives one round
on the slices a process holds, in the order ``Cluster._gossip_multiple`` runs it
(``aiocluster/server.py:441-495``): owner writes, ``inc_heartbeat`` + tombstone GC
(``gs_begin_round``), the conflict-free phases (``gs_run_phase``, or the sliced
count/gather/pack of ``shard.py``), then ``_update_node_liveness`` (``gs_liveness``).

With ``WorkloadSpec.loss > 0`` every phase carries a device ``legs`` tensor (``rd["legs"]``, parallel to
``rd["phases"]``: the messages delivered of each exchange, ``aiocluster_amd.cuts``) and runs through
``gs_run_phase_cut``; with peer-selected rounds the legs are drawn on the device (``gs_draw_cuts``).  With
``loss == 0`` nothing changes.

With ``WorkloadSpec.frame_limit`` every phase is first sized by ``gs_traffic_census`` with the reference's frame limit
(after the loss draw, whose legs it takes as what the network delivers), asynchronously, and runs with the census's
``legs_out``: an exchange stops where the peer would refuse an oversize packet.  A round record may carry
``rd["traffic_nodes"]`` (device int64 [2, N]: frame bytes sent / accepted per node, added to) and
``rd["traffic_totals"] = True``, which reads each phase's totals back (one host wait per phase) and accumulates
them in ``rd["traffic"]``; either of the two also sizes the phases of a round without ``frame_limit`` (nothing is
refused then: the phase runs with the network's legs).  Without any of the three nothing changes.

With ``WorkloadSpec.topology`` (``aiocluster_amd.topology``: zones and the links between them) and
``WorkloadSpec.link_events`` the network is partitioned: ``prepare`` applies each round's events at its start, removes
from every explicit phase the pairs whose connect would fail (``rd["exchanges"]`` counts the attempted exchanges,
``rd["no_connect"]`` the rest), draws the legs of the others with the zoned mirror (``cuts.draw_cuts_zoned``; only in
rounds in which some link loses messages) and keeps that round's link snapshot (``rd["topo"]``, ``rd["zone"]`` on the
device, ``rd["link"]``).  With a ``PeerSelector`` ``run_round`` filters the selected targets on the device
(``gs_filter_targets_zoned``) before the schedule, and draws every scheduled phase's legs with ``gs_draw_cuts_zoned``;
``rd["no_connect"]`` is then the device's count, read once per round.  The zoned legs feed the traffic census exactly
as the uniform ones do.  With no topology nothing changes.

On a sim created with ``write_log=True`` ``begin`` notes the round's writes in the sim's write log at the round's tick
(``gs_note_writes`` after its ``gs_owner_writes``), which is what ``GossipSim.age_census`` ages views against.  Without
the log nothing changes.
"""

from __future__ import annotations

import ctypes as C

import numpy as np


def digits(x: np.ndarray) -> np.ndarray:
    return np.floor(np.log10(np.maximum(x, 1))).astype(np.int64) + 1


def boot_ops(n: int, k: int) -> list[np.ndarray]:
    """``Cluster(initial_key_values)``: key k of owner j = "v{j}.{k}.i", as K batches of distinct owners
    (owner, key, op, value_id, value_len); value ids 1 + k * n + j."""
    out = []
    for kk in range(k):
        ops = np.zeros((n, 5), dtype=np.uint32)
        ops[:, 0] = np.arange(n)
        ops[:, 1] = kk
        ops[:, 3] = 1 + kk * n + np.arange(n)
        ops[:, 4] = 3 + digits(np.arange(n)) + digits(np.full(n, kk)) + 1
        out.append(ops)
    return out


def prepare(spec, rounds: int, torch, dev) -> list[dict]:
    """Every round's device inputs (host schedule generation is not timed).  Write values are
    interned as ids 2^24 + i with the byte length of ``workload.write_value``."""
    from .cuts import LINK_DOWN, draw_cuts_q32, draw_cuts_zoned, loss_q32
    from .workload import OP_DELETE, OP_DELETE_AFTER_TTL, Workload, liveness_tick, phase_tick, round_tick

    q32 = loss_q32(spec.loss)
    topo = getattr(spec, "topology", None)
    if topo is not None:
        if q32:
            raise ValueError("WorkloadSpec.loss together with a topology: express a uniform loss as a uniform link "
                             "matrix")
        if topo.n != spec.n:
            raise ValueError(f"topology of {topo.n} nodes for a workload of {spec.n}")
        topo = topo.copy()  # the events change the links: the spec keeps the initial ones
        zone_dev = torch.from_numpy(topo.zone.copy()).to(dev)
    elif getattr(spec, "link_events", None):
        raise ValueError("WorkloadSpec.link_events without a topology")
    events = sorted(getattr(spec, "link_events", None) or [], key=lambda e: e[0])
    wl = Workload(spec)
    out = []
    vid = 1 << 24
    for _ in range(rounds):
        p = wl.next_round(materialize_values=False)
        w = p.writes
        ops = np.zeros((len(w), 5), dtype=np.int64)
        if len(w):
            # value "v{j}.{k}.{r}" / "t{j}.{k}.{r}" (deletes: ""): byte length without materialising strings
            ops[:, 0], ops[:, 1], ops[:, 2] = w[:, 0], w[:, 1], w[:, 2]
            ops[:, 3] = vid + np.arange(len(w))
            vid += len(w)
            ops[:, 4] = 3 + digits(w[:, 0]) + digits(w[:, 1]) + digits(np.full(len(w), p.r))
            dele = (w[:, 2] == OP_DELETE) | (w[:, 2] == OP_DELETE_AFTER_TTL)
            ops[dele, 3] = 0
            ops[dele, 4] = 0
        r = p.r
        no_connect = 0
        if topo is not None:
            for _, action, args in (e for e in events if e[0] == r):
                topo.apply(action, args)
            kept = []
            for a, b in p.phases:
                ok = topo.connect_ok(a, b)
                no_connect += int((~ok).sum())
                kept.append((a[ok], b[ok]))
            p.phases = kept
        out.append({
            "r": r,
            "t": round_tick(r),
            "ops": torch.from_numpy(ops.astype(np.int32)).to(dev),
            "nops": len(w),
            "up": torch.from_numpy(p.up.astype(np.uint8)).to(dev),
            "up_host": p.up.astype(np.uint8),
            "phases": [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), len(a), phase_tick(r, i))
                       for i, (a, b) in enumerate(p.phases)],
            "t_live": liveness_tick(r, len(p.phases)),
            "exchanges": p.n_exchanges,
        })
        if q32:  # message loss: the legs of every phase, from the host mirror of gs_draw_cuts
            out[-1]["legs"] = [torch.from_numpy(draw_cuts_q32(a, b, spec.cut_seed, r, i, q32)).to(dev)
                               for i, (a, b) in enumerate(p.phases)]
            out[-1]["loss_q32"], out[-1]["cut_seed"] = q32, spec.cut_seed
        if topo is not None:
            snap = topo.copy()
            out[-1].update(no_connect=no_connect, topo=snap, zone=zone_dev, link=snap.link, cut_seed=spec.cut_seed)
            # legs only in rounds in which some link loses messages (a round of whole and down links runs plain phases)
            out[-1]["zoned_loss"] = bool(((snap.link != 0) & (snap.link != LINK_DOWN)).any())
            if out[-1]["zoned_loss"]:
                out[-1]["legs"] = [
                    torch.from_numpy(draw_cuts_zoned(a, b, spec.cut_seed, r, i, snap.zone, snap.link)).to(dev)
                    for i, (a, b) in enumerate(p.phases)]
        if getattr(spec, "frame_limit", False):
            out[-1]["frame_limit"] = True
    return out


def begin(sims, rd):
    """Owner writes + gs_begin_round of round ``rd`` on every slice."""
    for sim in sims:
        if rd["nops"]:
            sim._chk(sim.L.gs_owner_writes(sim.h, C.c_void_p(rd["ops"].data_ptr()), rd["nops"], rd["t"]),
                     "gs_owner_writes")
            if getattr(sim, "wlog", None) is not None:  # write_log=True: the round's writes are logged at its tick
                sim.note_writes(rd["t"])
        sim._chk(sim.L.gs_begin_round(sim.h, C.c_void_p(rd["up"].data_ptr()), rd["t"]), "gs_begin_round")


def run_phases(sims, rd, events=None, group=None, phases=None, legs=None):
    """The round's phases (``phases`` overrides the plan's: (a, b, n, tick) tuples; ``legs``: one device u8 tensor
    per phase, default the plan's ``rd["legs"]`` for the plan's phases)."""
    s0 = sims[0]
    if phases is None and legs is None:
        legs = rd.get("legs")
    limit = bool(rd.get("frame_limit"))
    framed = limit or bool(rd.get("traffic_totals")) or rd.get("traffic_nodes") is not None
    if (legs is not None or framed) and group is not None:
        raise ValueError("cut exchanges (loss > 0, frame_limit) run on one-slice handles only")
    if framed:
        from .sim import add_traffic_totals

        rd["traffic"] = None
    for i, (a, b, n, t) in enumerate(rd["phases"] if phases is None else phases):
        if not n:
            continue
        for s_ in sims:
            if s_._ev is not None:  # hook events: order_events needs each phase's exchange order
                if group is not None:
                    raise ValueError("hook events on a sliced cluster are not supported (drain per slice)")
                s_._ev_note_phase(a, b)
        if events is not None:
            e0 = s0.torch.cuda.Event(enable_timing=True)
            e1 = s0.torch.cuda.Event(enable_timing=True)
            e0.record(s0.stream)
        if framed:  # size the phase first; it then runs with what the peers would accept
            tc = s0.traffic_census(t, (a, b), legs=None if legs is None else legs[i], frame_limit=limit,
                                   nodes=rd.get("traffic_nodes"), totals=bool(rd.get("traffic_totals")))
            if rd.get("traffic_totals"):
                rd["traffic"] = add_traffic_totals(rd["traffic"], tc)
            s0._chk(s0.L.gs_run_phase_cut(s0.h, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                          C.c_void_p(tc["legs_out"].data_ptr()), n, t), "gs_run_phase_cut")
        elif legs is not None:
            s0._chk(s0.L.gs_run_phase_cut(s0.h, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                          C.c_void_p(legs[i].data_ptr()), n, t), "gs_run_phase_cut")
        elif group is None:
            s0._chk(s0.L.gs_run_phase(s0.h, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n, t),
                    "gs_run_phase")
        else:  # the group's own driver: shard.py's (its scratch kept across phases), or the library's (native)
            group.run_phase_arrays(t, a, b)
        if events is not None:
            e1.record(s0.stream)
            events.append((e0, e1))


def end(sims, rd, tick=None):
    """gs_liveness closing the round."""
    for sim in sims:
        sim._chk(sim.L.gs_liveness(sim.h, C.c_void_p(rd["up"].data_ptr()), rd["t_live"] if tick is None else tick),
                 "gs_liveness")


def run_round(sims, rd, events=None, group=None, sel=None):
    """One gossip round on the slices this process drives (one GossipSim when unsliced).  With ``sel``
    (a PeerSelector) the round's exchanges come from the device's select_nodes_for_gossip + phase
    schedule instead of the workload's explicit schedule (``rd`` gains "exchanges", "unscheduled")."""
    from .workload import TICKS_PER_ROUND, liveness_tick, phase_tick

    begin(sims, rd)
    phases = legs = None
    if sel is not None:
        sel.select(rd["up"], rd["r"])
        dropped = None
        if rd.get("topo") is not None:  # a failed connect occupies neither node: removed before the schedule
            dropped = sims[0].torch.zeros(1, dtype=sims[0].torch.int32, device=sims[0].device)
            sims[0].filter_targets(sel.targets, rd["zone"], rd["link"], dropped=dropped)
        ph, offs, left = sel.schedule(rd["up"], rd["r"])
        if dropped is not None:
            rd["no_connect"] = int(dropped.item())
        phases = [(a, b, n, phase_tick(rd["r"], p)) for p, (a, b, n) in enumerate(ph)]
        rd["exchanges"] = offs[-1]
        rd["unscheduled"] = left
        rd["t_live"] = liveness_tick(rd["r"], len(phases))  # sub-phases share the budget's last tick
        rd["phases_run"] = len(phases)
        if rd.get("loss_q32"):  # message loss over the scheduled phases, drawn on the device
            legs = [sims[0].draw_cuts(a, b, rd["cut_seed"], rd["r"], p, rd["loss_q32"])
                    for p, (a, b, n) in enumerate(ph)]
        elif rd.get("zoned_loss"):  # ... per link, on the device
            legs = [sims[0].draw_cuts_zoned(a, b, rd["cut_seed"], rd["r"], p, rd["zone"], rd["link"])
                    for p, (a, b, n) in enumerate(ph)]
    if rd["t_live"] >= rd["t"] + TICKS_PER_ROUND:
        raise ValueError(f"round {rd['r']}: liveness tick {rd['t_live']} reaches the next round's tick")
    run_phases(sims, rd, events, group, phases, legs)
    end(sims, rd)

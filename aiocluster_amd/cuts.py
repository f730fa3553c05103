"""Cut exchanges: independent message loss, drawn reproducibly.

An exchange is three messages -- Syn, SynAck, Ack (aiocluster/server.py:378-439, 523-568) -- and each is
followed by the next handler only if it arrived.  ``legs`` of an exchange is the number of messages
delivered before the first lost one (``gs_run_phase_cut`` in include/gossip_sim.h):

    3  intact
    2  the Ack is lost: the responder has reported heartbeats but learns no data
    1  the SynAck is lost: the responder alone has merged the initiator's digest
    0  the connection was accepted, the Syn never read: only the responder's own heartbeat + 1

``draw_cuts`` is the definition of the draw; the device's ``gs_draw_cuts`` must equal it.  Message m
(0 = Syn, 1 = SynAck, 2 = Ack) of an exchange is lost iff word m of
Philox4x32-10(key = seed, counter = (round, initiator, responder, phase)) is below ``loss_q32``.
"""

from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def loss_q32(loss: float) -> int:
    """The loss probability as a 32-bit threshold: min(round(loss * 2^32), 2^32 - 1)."""
    if not 0.0 <= loss <= 1.0:
        raise ValueError(f"loss must be a probability (got {loss})")
    return min(int(round(loss * 4294967296.0)), 4294967295)


def philox4x32(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 over arrays of counter words (uint64 arrays holding 32-bit values); returns the 4 words."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in (c0, c1, c2, c3)]
    k0 &= 0xFFFFFFFF
    k1 &= 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & _M32, p1 & _M32,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & _M32, p0 & _M32]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def draw_cuts_q32(ini, res, seed: int, rnd: int, phase: int, q32: int) -> np.ndarray:
    """``draw_cuts`` for a threshold given as ``loss_q32``."""
    ini = np.asarray(ini, dtype=np.int64).reshape(-1)
    res = np.asarray(res, dtype=np.int64).reshape(-1)
    if ini.shape != res.shape:
        raise ValueError("initiators and responders differ in length")
    n = ini.size
    full = lambda v: np.full(n, v & 0xFFFFFFFF, dtype=np.uint64)  # noqa: E731
    w = philox4x32(full(rnd), ini.astype(np.uint64) & _M32, res.astype(np.uint64) & _M32, full(phase),
                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    q = np.uint64(q32)
    lost = [w[m] < q for m in range(3)]
    legs = np.where(lost[0], 0, np.where(lost[1], 1, np.where(lost[2], 2, 3)))
    return legs.astype(np.uint8)


LINK_DOWN = 0xFFFFFFFF  # GS_LINK_DOWN: the link carries nothing
LEGS_NO_CONNECT = 255  # GS_LEGS_NO_CONNECT: the connect of that pair would fail
MAX_ZONES = 16  # GS_MAX_ZONES


def _link_matrix(link) -> np.ndarray:
    link = np.asarray(link)
    if link.ndim != 2 or link.shape[0] != link.shape[1] or not 1 <= link.shape[0] <= MAX_ZONES:
        raise ValueError(f"link: a [Z, Z] matrix of 32-bit thresholds, 1 <= Z <= {MAX_ZONES} (got shape {link.shape})")
    return link.astype(np.uint64)


def connect_ok(ini, res, zone, link) -> np.ndarray:
    """The connect rule of zoned links (include/gossip_sim.h): the exchange ``ini[e] -> res[e]`` is attempted iff
    both nodes exist, both zone bytes are below Z and neither ``link[zone a][zone b]`` nor ``link[zone b][zone a]``
    is ``LINK_DOWN``.  A link down in one direction alone fails the connects of both directions."""
    link = _link_matrix(link)
    Z = link.shape[0]
    zone = np.asarray(zone, dtype=np.int64).reshape(-1)
    n = zone.size
    a = np.asarray(ini, dtype=np.int64).reshape(-1)
    b = np.asarray(res, dtype=np.int64).reshape(-1)
    ok = (a >= 0) & (a < n) & (b >= 0) & (b < n)
    za, zb = zone[np.where(ok, a, 0)], zone[np.where(ok, b, 0)]
    ok &= (za < Z) & (zb < Z)
    za, zb = np.where(ok, za, 0), np.where(ok, zb, 0)
    return ok & (link[za, zb] != LINK_DOWN) & (link[zb, za] != LINK_DOWN)


def draw_cuts_zoned(ini, res, seed: int, rnd: int, phase: int, zone, link) -> np.ndarray:
    """The definition of the zoned draw; the device's ``gs_draw_cuts_zoned`` must equal it.  Message m of an
    attempted exchange (0 Syn a->b, 1 SynAck b->a, 2 Ack a->b) is lost iff word m of ``draw_cuts``' Philox block is
    below the link threshold of that message's direction; a pair whose connect would fail gets 255."""
    linkm = _link_matrix(link)
    zone = np.asarray(zone, dtype=np.int64).reshape(-1)
    a = np.asarray(ini, dtype=np.int64).reshape(-1)
    b = np.asarray(res, dtype=np.int64).reshape(-1)
    if a.shape != b.shape:
        raise ValueError("initiators and responders differ in length")
    n = a.size
    ok = connect_ok(a, b, zone, linkm)
    za, zb = zone[np.where(ok, a, 0)], zone[np.where(ok, b, 0)]
    fwd, bwd = linkm[za, zb], linkm[zb, za]
    full = lambda v: np.full(n, v & 0xFFFFFFFF, dtype=np.uint64)  # noqa: E731
    w = philox4x32(full(rnd), a.astype(np.uint64) & _M32, b.astype(np.uint64) & _M32, full(phase),
                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    legs = np.where(w[0] < fwd, 0, np.where(w[1] < bwd, 1, np.where(w[2] < fwd, 2, 3)))
    return np.where(ok, legs, LEGS_NO_CONNECT).astype(np.uint8)


def filter_targets_zoned(targets, zone, link) -> tuple[np.ndarray, int]:
    """The mirror of ``gs_filter_targets_zoned``: ``targets`` ([N, slots], -1 = none: ``gs_select_peers``' output)
    with every target whose connect would fail made -1, and the number of targets dropped."""
    t = np.asarray(targets, dtype=np.int32)
    n = np.asarray(zone).reshape(-1).size
    if t.ndim != 2 or t.shape[0] != n:
        raise ValueError(f"targets: [N, slots] for {n} nodes (got shape {t.shape})")
    ini = np.repeat(np.arange(n, dtype=np.int64), t.shape[1])
    drop = (t.reshape(-1) >= 0) & ~connect_ok(ini, t.reshape(-1), zone, link)
    out = np.where(drop.reshape(t.shape), -1, t).astype(np.int32)
    return out, int(drop.sum())


def draw_cuts(ini, res, seed: int, rnd: int, phase: int, loss: float) -> np.ndarray:
    """uint8 legs of the exchanges ``ini[e] -> res[e]`` of phase ``phase`` of round ``rnd`` under independent
    message loss with probability ``loss``."""
    return draw_cuts_q32(ini, res, seed, rnd, phase, loss_q32(loss))

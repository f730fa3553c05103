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


def draw_cuts(ini, res, seed: int, rnd: int, phase: int, loss: float) -> np.ndarray:
    """uint8 legs of the exchanges ``ini[e] -> res[e]`` of phase ``phase`` of round ``rnd`` under independent
    message loss with probability ``loss``."""
    return draw_cuts_q32(ini, res, seed, rnd, phase, loss_q32(loss))

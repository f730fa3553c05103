"""Network partitions: zones, the links between them, and the ground truth of a partitioned cluster.

Every node has a zone; ``link[x][y]`` is the loss threshold (``cuts.loss_q32``) of a message sent from a node of zone
``x`` to a node of zone ``y`` (the diagonal is the loss inside a zone; the matrix need not be symmetric) and
``LINK_DOWN`` means the link carries nothing.  The model is stated in ``include/gossip_sim.h`` (zoned links):

* an exchange ``a -> b`` is attempted only if neither direction between the two zones is down -- otherwise the TCP
  connect times out (``asyncio.wait_for(open_coro, connect_timeout)``, ``aiocluster/server.py:403-405, 424-431``)
  and nothing happens at either node;
* zones ``x`` and ``y`` are *connected* if a chain of zones joins them in which each consecutive pair has both
  directions not down (the transitive closure of the connect rule: gossip relays, so a heartbeat crosses any such
  chain); the classes are the *components*;
* a target ``j`` is *reachable* for an observer ``o`` iff ``up[j]`` and the zones of ``o`` and ``j`` are in one
  component; ``unreachable_since(o, j)`` is the earliest tick of the causes still in force (the node went down, the
  two components were separated).

``Topology`` holds the zones and the links, ``LinkClock`` is the partner of ``detect.DownClock`` for the links.
"""

from __future__ import annotations

import numpy as np

from .cuts import LINK_DOWN, MAX_ZONES, connect_ok, loss_q32

# a link that loses every message but still connects: loss_q32(1.0) is LINK_DOWN's value
LOSS_MAX_Q32 = LINK_DOWN - 1


class Topology:
    """Zones of ``len(zone)`` nodes and the ``[Z, Z]`` link matrix between them.

    ``set_link`` sets a link's loss and remembers it as the link's healthy state; ``cut`` takes a link down;
    ``heal`` / ``heal_all`` put links back to their healthy state."""

    def __init__(self, zone, n_zones: int, link=None):
        z = np.asarray(zone)
        self.n_zones = int(n_zones)
        if not 1 <= self.n_zones <= MAX_ZONES:
            raise ValueError(f"n_zones must be in 1..{MAX_ZONES} (got {n_zones})")
        if z.ndim != 1 or z.size == 0 or int(z.min()) < 0 or int(z.max()) >= self.n_zones:
            raise ValueError(f"zone: one zone in 0..{self.n_zones - 1} per node")
        self.zone = z.astype(np.uint8)
        self.n = int(z.size)
        if link is None:
            link = np.zeros((self.n_zones, self.n_zones), dtype=np.uint32)
        link = np.asarray(link)
        if link.shape != (self.n_zones, self.n_zones):
            raise ValueError(f"link: a [{self.n_zones}, {self.n_zones}] matrix (got shape {link.shape})")
        self.link = link.astype(np.uint32)
        self._healthy = np.where(self.link == LINK_DOWN, 0, self.link).astype(np.uint32)

    @classmethod
    def blocks(cls, bounds, n_zones: int | None = None) -> "Topology":
        """Zones as consecutive index ranges: zone z = nodes ``bounds[z] .. bounds[z + 1] - 1``."""
        bounds = [int(b) for b in bounds]
        zone = np.zeros(bounds[-1], dtype=np.uint8)
        for z in range(len(bounds) - 1):
            zone[bounds[z]:bounds[z + 1]] = z
        return cls(zone, len(bounds) - 1 if n_zones is None else n_zones)

    def copy(self) -> "Topology":
        t = Topology(self.zone, self.n_zones, self.link)
        t._healthy = self._healthy.copy()
        return t

    def _z(self, x) -> int:
        x = int(x)
        if not 0 <= x < self.n_zones:
            raise ValueError(f"zone {x} of {self.n_zones}")
        return x

    def set_link(self, x: int, y: int, loss: float = 0.0, both: bool = True):
        """``link[x][y]`` (and ``link[y][x]`` with ``both``) loses each message with probability ``loss``; 1.0 is
        a link that loses everything but still connects (a connect needs ``cut`` to fail)."""
        x, y = self._z(x), self._z(y)
        q = min(loss_q32(loss), LOSS_MAX_Q32)
        for a, b in ((x, y), (y, x)) if both else ((x, y),):
            self.link[a, b] = self._healthy[a, b] = q

    def cut(self, x: int, y: int, both: bool = True):
        """``link[x][y]`` (and ``link[y][x]`` with ``both``) carries nothing.  One direction is enough to fail the
        connects of both."""
        x, y = self._z(x), self._z(y)
        self.link[x, y] = LINK_DOWN
        if both:
            self.link[y, x] = LINK_DOWN

    def heal(self, x: int, y: int):
        """Both directions between ``x`` and ``y`` back to their healthy loss."""
        x, y = self._z(x), self._z(y)
        self.link[x, y], self.link[y, x] = self._healthy[x, y], self._healthy[y, x]

    def split(self, groups):
        """Cut every link between zones of different groups (``groups``: lists of zones; the zones not listed form
        one more group)."""
        g = np.full(self.n_zones, len(groups), dtype=np.int64)
        for i, zs in enumerate(groups):
            for z in zs:
                g[self._z(z)] = i
        apart = g[:, None] != g[None, :]
        self.link[apart] = LINK_DOWN

    def heal_all(self):
        self.link = self._healthy.copy()

    def apply(self, action: str, args=()):
        """One link event by name (``WorkloadSpec.link_events``): split, heal_all, cut, heal, set_link."""
        if action not in ("split", "heal_all", "cut", "heal", "set_link"):
            raise ValueError(f"unknown link event {action!r}")
        if action == "split":
            self.split(args)
        else:
            getattr(self, action)(*args)

    def link_u32(self) -> np.ndarray:
        """The matrix as the contiguous ``u32 [Z * Z]`` array the library takes."""
        return np.ascontiguousarray(self.link, dtype=np.uint32).reshape(-1)

    def connect_ok(self, ini, res) -> np.ndarray:
        """bool mask: the exchanges ``ini[e] -> res[e]`` that will be attempted (the host mirror of the connect
        rule)."""
        return connect_ok(ini, res, self.zone, self.link)

    def zone_components(self) -> np.ndarray:
        """int64 [Z]: the component of each zone, numbered by their smallest zone."""
        Z = self.n_zones
        both = (self.link != LINK_DOWN) & (self.link.T != LINK_DOWN)
        comp = np.full(Z, -1, dtype=np.int64)
        c = 0
        for s in range(Z):
            if comp[s] >= 0:
                continue
            comp[s] = c
            todo = [s]
            while todo:
                x = todo.pop()
                for y in np.flatnonzero(both[x] & (comp < 0)).tolist():
                    comp[y] = c
                    todo.append(y)
            c += 1
        return comp

    def components(self) -> list[list[int]]:
        """The components as lists of zones, ordered by their smallest zone."""
        comp = self.zone_components()
        return [np.flatnonzero(comp == c).tolist() for c in range(int(comp.max()) + 1)]

    def node_components(self) -> np.ndarray:
        """int64 [N]: the component of each node's zone."""
        return self.zone_components()[self.zone]

    def reachable(self, up) -> np.ndarray:
        """bool [C, N]: ``[c, j]`` = target ``j`` is reachable for the observers of component ``c``."""
        up = np.asarray(up).astype(bool)
        nc = self.node_components()
        return (nc[None, :] == np.arange(int(nc.max()) + 1)[:, None]) & up[None, :]


def views_behind(sim, up, topo: Topology) -> np.ndarray:
    """int64 [Z, Z]: ``[x, y]`` = the views of zone ``y``'s owners, held by the up observers of zone ``x``, that are
    behind the owner's own max_version: how far each zone's data has spread into the others.  One
    ``view_census(per_owner=True)`` per observer zone (rows that are not counted are not read, so the Z calls stream
    the matrix once), ``owner_behind`` summed on the host by owner zone.  A component's rows are the sum of its
    zones'.  ``sim``: a ``GossipSim`` or a ``ShardGroup``."""
    up = np.asarray(up.cpu() if hasattr(up, "cpu") else up).astype(bool)
    out = np.zeros((topo.n_zones, topo.n_zones), dtype=np.int64)
    for x in range(topo.n_zones):
        mask = up & (topo.zone == x)
        if not mask.any():
            continue
        behind = sim.view_census(mask.astype(np.uint8), per_owner=True)["owner_behind"].cpu().numpy()
        out[x] = np.bincount(topo.zone, weights=behind, minlength=topo.n_zones).astype(np.int64)
    return out


class LinkClock:
    """The tick at which two zones were separated (stopped being in one component), as ``detect.DownClock`` keeps
    the tick at which a node went down.  ``update(topo, tick)`` after every change of the links."""

    def __init__(self, n_zones: int):
        self.n_zones = int(n_zones)
        self.apart_since = np.full((self.n_zones, self.n_zones), -1, dtype=np.int64)  # -1: connected

    def update(self, topo: Topology, tick: int) -> np.ndarray:
        comp = topo.zone_components()
        apart = comp[:, None] != comp[None, :]
        self.apart_since[apart & (self.apart_since < 0)] = int(tick)
        self.apart_since[~apart] = -1
        return self.apart_since

    def unreachable_since(self, topo: Topology, up, down_since) -> np.ndarray:
        """uint32 [C, N]: per component of observers, the earliest tick of the causes for which target ``j`` is
        unreachable that are still in force -- ``down_since[j]`` (``DownClock.down_since`` or the clock itself) if
        the node is down, the separation tick if its zone is in another component.  A component has lost a zone
        when its last member did: the latest of its zones' separation ticks.  Entries of reachable targets are 0
        (the census ignores them)."""
        ds = np.asarray(getattr(down_since, "down_since", down_since)).astype(np.int64)
        up = np.asarray(up).astype(bool)
        comp = topo.zone_components()
        C = int(comp.max()) + 1
        big = np.iinfo(np.int64).max
        out = np.zeros((C, topo.n), dtype=np.uint32)
        for c in range(C):
            mine = comp == c
            sep_zone = np.where(mine, -1, self.apart_since[mine].max(axis=0))  # [Z]: -1 = one of this component's
            if ((sep_zone < 0) != mine).any():
                raise ValueError("LinkClock.update has not seen the topology's current links")
            sep = sep_zone[topo.zone]
            cause = np.minimum(np.where(up, big, ds), np.where(sep >= 0, sep, big))
            out[c] = np.where(cause == big, 0, cause).astype(np.uint32)
        return out

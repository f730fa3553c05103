"""Large-value scenarios: values up to the 16,383-byte limit and NodeDeltas past 64 KiB.

Every other scenario of the suite writes values of about ten bytes (``workload.write_value``), so no size
field on the device ever holds a value length of 128 or more, or a NodeDelta of 16,384 bytes or more.  The
two deterministic builders here produce plain scenario dicts (``aiocluster_amd.scenario``) that do:

* ``big_values(scen)`` rewrites the value strings of a ``make_scenario`` dict to lengths at the varint and
  limit edges (``EDGES``);
* ``sleeper_scenario(...)`` builds a cluster in which a few nodes are away while every other owner writes
  five values of 13-16 KB, so that on their return most whole NodeDeltas are 65,536 bytes or more, one of
  them exactly 65,536.

Used by ``oracle/gen_golden.py`` (fixtures ``scen_bigval6``, ``scen_bigsleep12``), ``tests/test_bigvalues_host.py``
and ``tests/test_gpu_bigvalues.py``.
"""

from aiocluster_amd.pbsize import kv_size_from_lens, msg_field, nodedelta_size, nodeid_size
from aiocluster_amd.scenario import make_scenario
from aiocluster_amd.workload import OP_DELETE, OP_DELETE_AFTER_TTL, WorkloadSpec

MAX_VALUE_LEN = (1 << 14) - 1  # gs_owner_writes refuses value lengths >= 2^14
# 1- / 2- / 3-byte length varints of the value (127 | 128) and of the kv message around it (16,382 + the key and
# version fields is past 16,383), mid-range values and the limit itself
EDGES = (1, 2, 127, 128, 129, 5_000, 9_000, 13_000, 16_256, 16_382, MAX_VALUE_LEN)
PAD = "x"


def edge_len(j: int, k: int, r: int) -> int:
    """The value length of owner j's write of key k in round r (r = -1: the boot write)."""
    return EDGES[(7 * j + 3 * k + 5 * (r + 1)) % len(EDGES)]


def _grow(orig: str, length: int, seq: int) -> str:
    """``orig`` padded to ``length`` bytes.  The original text stays as the prefix, so values that differed still
    differ; a length below the original's cannot keep it, and takes base-26 digits of ``seq`` (the write's round
    + 1) instead: distinct among the writes of one (owner, key), which is what the no-op rule of
    NodeState.set compares (state.py:140-151)."""
    if length >= len(orig):
        return orig + PAD * (length - len(orig))
    assert seq < 26 ** length, "too many rounds for distinct short values"
    s = ""
    for _ in range(length):
        s = chr(ord("a") + seq % 26) + s
        seq //= 26
    return s


def big_values(scen: dict) -> dict:
    """Rewrite, in place, the value of every boot write and every SET / SET_WITH_TTL write of ``scen`` to
    ``edge_len`` bytes; deletes keep ``""``.  Returns ``scen``."""
    for w in scen["initial"]:
        j, k, v = w
        w[2] = _grow(v, edge_len(j, k, -1), 0)
    for r, rd in enumerate(scen["rounds"]):
        for w in rd["writes"]:
            j, k, op, v = w
            if op in (OP_DELETE, OP_DELETE_AFTER_TTL):
                assert v == ""
                continue
            w[3] = _grow(v, edge_len(j, k, r), r + 1)
    return scen


def _nid_size(scen: dict, j: int) -> int:
    name, gen, host, port, tls = scen["nodes"][j]
    return nodeid_size(name, gen, host, port, tls)


def whole_nodedelta_size(scen: dict, j: int, from_version: int, value_lens: list[int], key_len: int) -> int:
    """DeltaPb bytes of owner j's NodeDelta carrying the writes ``from_version + 1 ..`` with these value lengths
    (status SET, no tombstone GC), from ``aiocluster_amd.pbsize``."""
    kvs = [kv_size_from_lens(key_len, vl, from_version + 1 + i, 0) for i, vl in enumerate(value_lens)]
    return msg_field(nodedelta_size(_nid_size(scen, j), from_version, 0, kvs, from_version + len(kvs)))


def sleeper_lens(j: int, away: int) -> list[int]:
    """Value lengths of owner j's writes in the away rounds: every fifth owner writes 1..200 bytes (small NodeDeltas
    for first-fit continuation to pick up after the first miss), the others 13,200..16,383."""
    if j % 5 == 0:
        return [1 + (31 * j + 17 * r) % 200 for r in range(away)]
    return [13_200 + (7919 * j + 104_729 * r) % (MAX_VALUE_LEN - 13_200 + 1) for r in range(away)]


def sleeper_scenario(n: int, mtu: int, sleepers: int, away: int, after: int, designated: int = 5,
                     exact: int = 1 << 16):
    """(scenario, sizes).  Warm start, K = 16, SET only.  Rounds 0..away-1: nodes 0..sleepers-1 are down (their
    pairs leave the phases), every other owner j writes key r once per round, ``sleeper_lens(j, away)`` bytes --
    except owner ``designated``, whose last value is tuned so that its whole NodeDelta to a sleeper is exactly
    ``exact`` DeltaPb bytes.  Then ``after`` rounds with everybody up and no writes.  ``sizes[j]`` = DeltaPb bytes
    of owner j's whole NodeDelta to a node that slept through all of it (0 for the sleepers, who wrote nothing)."""
    K = 16
    assert sleepers <= designated < n and away <= K
    spec = WorkloadSpec(n=n, k=K, fanout=3, seed=n, init="warm", write_frac=0.0)
    scen = make_scenario(f"bigsleep{n}", spec, away + after, {"mtu": mtu})
    key_len = len(scen["keys"][0])
    assert all(len(k) == key_len for k in scen["keys"])
    lens = {j: sleeper_lens(j, away) for j in range(sleepers, n)}
    # the designated owner: 13,000 bytes per write, the last one whatever makes the NodeDelta exactly `exact`
    head = [13_000] * (away - 1)
    fit = [v for v in range(1, MAX_VALUE_LEN + 1)
           if whole_nodedelta_size(scen, designated, K, head + [v], key_len) == exact]
    assert len(fit) == 1, f"no last value length gives a NodeDelta of {exact} bytes"
    lens[designated] = head + fit
    for r in range(away):
        rd = scen["rounds"][r]
        for s in range(sleepers):
            rd["up"][s] = 0
        rd["phases"] = [[p for p in ph if p[0] >= sleepers and p[1] >= sleepers] for ph in rd["phases"]]
        rd["writes"] = [[j, r, 0, (f"v{j}.{r}." + PAD * lens[j][r])[:lens[j][r]]] for j in range(sleepers, n)]
    sizes = [0] * sleepers + [whole_nodedelta_size(scen, j, K, lens[j], key_len) for j in range(sleepers, n)]
    return scen, sizes

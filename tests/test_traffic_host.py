"""gs_traffic_census on the host (CPU): the closed-form packet sizes, the plain-Python model (tests/trafficref.py)
pinned to the real reference's bytes, and the ABI.

The model is pinned twice before any GPU is involved: to the Syn and delta lengths of the wire fixtures
(``wire_*.json.gz``: the reference's own ``SerializeToString``), over the reference's round states; and to every size
and outcome the reference recorded in the framed fixtures (tools/gen_traffic_fixture.py), with the oracle composer of
tests/lossycases.py stepping the same phases.
"""

import ctypes as C
import random
import re

import numpy as np
import pytest
from helpers import first_diff, load_scenario, make_backend
from lossycases import CutOracleSim
from pbread import fields
from test_wire_host import NAMES as WIRE_NAMES
from test_wire_host import load_wire
from trafficcases import CASES, FIXTURES
from trafficref import BUCKETS, TrafficRef, bucket, for_backend

from aiocluster_amd import _lib
from aiocluster_amd.pbsize import nodeid_size
from aiocluster_amd.scenario import round_tick, round_ticks
from aiocluster_amd.wire import frame, frame_size, packet, packet_size


# ---------------------------------------------------------------- 1. closed forms
EDGES = [0, 1, 2, 126, 127, 128, 129, 16382, 16383, 16384, 16385, (1 << 21) - 1, 1 << 21]


def check_sizes(cid, dg, dl):
    d, e = b"\x01" * dg, b"\x02" * dl
    for kind, kw, args in (("syn", {"digest": d}, {"digest_len": dg}),
                           ("synack", {"digest": d, "delta": e}, {"digest_len": dg, "delta_len": dl}),
                           ("ack", {"delta": e}, {"delta_len": dl})):
        pkt = packet(cid, kind, **kw)
        assert packet_size(kind, cluster_id=cid, **args) == len(pkt), (cid, kind, dg, dl)
        assert frame_size(kind, cluster_id=cid, **args) == len(frame(pkt)) == len(pkt) + 4


def test_packet_and_frame_size_at_every_length_prefix_boundary():
    """127/128 and 16,383/16,384 of each of the prefixes: the digest's, the delta's, the SynPb / SynAckPb / AckPb
    body's (the bodies add 2-8 bytes to the sizes below) and the cluster id's."""
    for cid in ("", "c", "default-cluster", "x" * 127, "y" * 128):
        for dg in EDGES[:11]:
            for dl in (0, 1, 127, 128, 16383, 16384):
                check_sizes(cid, dg, dl)
    for total in (127, 128, 16383, 16384):  # the SynAckPb body itself at a boundary
        for cut in range(0, 9):
            for dg in (0, 5, 60):
                dl = total - cut - dg
                if dl >= 0:
                    check_sizes("default-cluster", dg, dl)
    with pytest.raises(ValueError):
        packet_size("nak")


def test_packet_and_frame_size_random():
    rng = random.Random(7)
    for _ in range(300):
        check_sizes("c" * rng.randrange(0, 40), rng.randrange(0, 70000), rng.randrange(0, 70000))


def test_buckets():
    assert [bucket(x) for x in (0, 1, 2, 3, 4, 127, 128, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1)] == \
        [0, 1, 2, 2, 3, 7, 8, 16, 17, 31, 31, 31]
    assert BUCKETS == _lib.GS_TC_BUCKETS


# ---------------------------------------------------------------- 2. the model against the wire fixtures
def export_of_states(states, n, keys):
    """The reference's canonical round states (``expect.states[r]``) as an ``export()`` dict, with a value table."""
    K = len(keys)
    kidx = {k: i for i, k in enumerate(keys)}
    values, vid = [""], {"": 0}
    ex = {"pos": np.full((n, n), -1, np.int32), "hb": np.zeros((n, n), np.uint32), "mv": np.zeros((n, n), np.uint32),
          "gc": np.zeros((n, n), np.uint32), "kv_version": np.zeros((n, n, K), np.uint32),
          "kv_status": np.zeros((n, n, K), np.int32), "kv_value_id": np.zeros((n, n, K), np.uint32),
          "tod": np.full((n, n), -1, np.int64)}
    for o, st in enumerate(states):
        for p, (j, hb, mv, gc, kvs) in enumerate(st["nodes"]):
            ex["pos"][o, j], ex["hb"][o, j], ex["mv"][o, j], ex["gc"][o, j] = p, hb, mv, gc
            for key, value, ver, status, _ in kvs:
                k = kidx[key]
                ex["kv_version"][o, j, k], ex["kv_status"][o, j, k] = ver, status
                ex["kv_value_id"][o, j, k] = vid.setdefault(value, len(values))
                if vid[value] == len(values):
                    values.append(value)
        for j, tod in st["dead"]:
            ex["tod"][o, j] = tod
    return ex, values


# the wire fixtures whose scenario fixture holds the reference's round states (the others hold hashes only)
WIRE_WITH_STATES = [name for name in WIRE_NAMES if load_scenario(name)["expect"].get("states")]


@pytest.mark.parametrize("name", WIRE_WITH_STATES)
def test_model_reproduces_the_wire_fixtures(name):
    scen = load_scenario(name)
    states = scen["expect"]["states"]
    w = load_wire(name)
    n = scen["n"]
    nid = [nodeid_size(x[0], x[1], x[2], x[3], x[4]) for x in scen["nodes"]]
    klen = [len(k.encode()) for k in scen["keys"]]
    cache, checked = {}, 0
    for r, s, q, syn_hex, delta_hex in w["cases"]:
        if r >= len(states):
            continue
        if r not in cache:
            ex, values = export_of_states(states[r], n, scen["keys"])
            cache[r] = (ex, TrafficRef(nid, klen, values, scen["config"]))
        ex, ref = cache[r]
        t = w["tick"][str(r)]
        syn = bytes.fromhex(syn_hex)
        digest = fields(fields(syn)[1][2])[0][2]
        mine = ref.digest(ex, s, t)
        assert ref.digest_size(mine) == len(digest), (r, s)
        assert packet_size("syn", digest_len=len(digest)) == len(syn)
        assert ref.delta_size(ex, s, ref.digest(ex, q, t), t) == len(delta_hex) // 2, (r, s, q)
        checked += 1
    assert checked > 0


# ---------------------------------------------------------------- 3. the model against the framed fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_the_scenario_of_trafficcases(name):
    scen, want = load_scenario(name), CASES[name]()
    for k in want:
        if k != "rounds":
            assert scen[k] == want[k], k
    assert set(scen) - set(want) <= {"expect", "w1000"}
    for r, rd in enumerate(want["rounds"]):
        for k in rd:
            assert scen["rounds"][r][k] == rd[k], (r, k)


def test_fixtures_hold_what_they_are_for():
    total, hb_lo, hb_hi = [0, 0, 0, 0], False, False
    for name in FIXTURES:
        scen = load_scenario(name)
        c = [0, 0, 0, 0]
        for rd in scen["rounds"]:
            for lg in rd["legs"]:
                for x in lg:
                    c[x] += 1
        assert sum(1 for x in c if x) >= 2, (name, c)
        total = [x + y for x, y in zip(total, c)]
        for st in scen["expect"]["states"]:
            for o in st:
                for _, hb, _, _, _ in o["nodes"]:
                    hb_lo |= 0 < hb < 128
                    hb_hi |= hb >= 128
    assert min(total) >= 10 and hb_lo and hb_hi, total
    own = [[nd[2] for nd in st[2]["nodes"] if nd[0] == 2][0] for st in load_scenario("frame10")["expect"]["states"]]
    assert min(own) < 128 <= max(own)  # owner 2's own max_version crosses 128


def framed_for_composer(scen):
    """The composer keeps no ring contents across an Ack-lost exchange (tests/lossycases.py), so a fixture whose
    windows roll over carries ``"w1000"``: the reference's legs, traffic and states of the same scenario with
    window 1000.  That run is the one the composer steps."""
    wide = scen.get("w1000")
    if wide is None:
        return scen
    scen = dict(scen, config=dict(scen["config"], window=1000), expect=wide["expect"])
    scen["rounds"] = [dict(rd, legs=wide["legs"][r], traffic=wide["traffic"][r]) for r, rd in enumerate(scen["rounds"])]
    return scen


@pytest.mark.parametrize("name", FIXTURES)
def test_model_reproduces_the_framed_fixture(name):
    """Before each phase: the model over the composer's export gives every recorded size, packet and outcome; the
    composer then runs the phase with those outcomes, and ends every round in the reference's state."""
    scen = framed_for_composer(load_scenario(name))
    exp = scen["expect"]
    orc = make_backend(CutOracleSim, scen)
    ref = for_backend(orc, scen)
    sizes = 0
    for r, rd in enumerate(scen["rounds"]):
        t = round_tick(r)
        ticks = round_ticks(scen, r)
        for j, k, op, v in rd["writes"]:
            orc.write(t, j, k, op, v)
        orc.begin_round(t, rd["up"])
        for p, ph in enumerate(rd["phases"]):
            net = rd["net_legs"][p] if "net_legs" in rd else None
            got = ref.phase(orc.export(), ph, ticks[p], legs=net, frame_limit=True)
            assert got["legs_out"] == rd["legs"][p], (r, p)
            for e, rec in enumerate(rd["traffic"][p]):
                m, pk = got["msg"][e], got["packets"][e]
                for i in range(4):
                    if rec[i] is not None:
                        assert m[i] == rec[i], (r, p, e, i, m, rec)
                        sizes += 1
                assert pk == rec[4:], (r, p, e, pk, rec)
            orc.run_phase(ticks[p], ph, rd["legs"][p])
        orc.liveness(ticks[-1], rd["up"], r)
        st = orc.state()
        assert st == exp["states"][r], f"round {r}: {first_diff(st, exp['states'][r])}"
    assert sizes > 1000
    orc.close()


# ---------------------------------------------------------------- 4. ABI
@pytest.fixture()
def handle():
    from aiocluster_amd.scenario import DEFAULT_CFG
    from aiocluster_amd.sim import make_config

    lib = _lib.load()
    h = C.c_void_p()
    cfg = make_config(1000, 16, DEFAULT_CFG, _lib.GS_CANONICAL, 32)
    assert lib.gs_create(C.byref(cfg), C.byref(h)) == 0
    yield lib, h
    lib.gs_destroy(h)


def test_totals_struct_is_128_words():
    T = _lib.GsTrafficTotals
    assert C.sizeof(T) == 128 * 8
    assert T.exchanges.offset == 0 and T.bad_index.offset == 8 and T.sent.offset == 16
    assert T.bytes_delivered.offset == 17 * 8 and T.digest_bytes_sent.offset == 20 * 8
    assert T.max_frame.offset == 23 * 8 and T.frame_hist.offset == 26 * 8 and T.reserved.offset == 122 * 8


def test_header_and_binding_agree():
    src = open(_lib.HEADER).read()
    for name, want in (("GS_TC_FRAME_LIMIT", _lib.GS_TC_FRAME_LIMIT), ("GS_TC_BUCKETS", _lib.GS_TC_BUCKETS)):
        m = re.search(rf"^#define {name} (\d+)u?\b", src, re.M)
        assert m and int(m.group(1)) == want, name
    assert "gs_traffic_census" in _lib.EXPORTS
    body = re.search(r"typedef struct gs_traffic_totals \{(.*?)\} gs_traffic_totals;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\w+\])*\s*[,;]", body)
    assert names == [f[0] for f in _lib.GsTrafficTotals._fields_]
    assert re.search(r"int gs_traffic_census\(gs_handle \*h, const int32_t \*initiators, const int32_t \*responders,", src)


def test_refusals_come_before_any_device_work(handle):
    lib, h = handle
    call, inv = lib.gs_traffic_census, _lib.GS_E_INVALID
    p = C.c_void_p(0x1000)  # never dereferenced: every call below fails before any device work
    tot = _lib.GsTrafficTotals()

    def err():
        return lib.gs_last_error(h)

    assert hasattr(lib, "gs_traffic_census")
    assert call(None, p, p, None, 1, 0, 15, 0, None, p, None, None) == inv
    assert call(h, None, p, None, 1, 0, 15, 0, None, p, None, None) == inv and b"NULL" in err()
    assert call(h, p, None, None, 1, 0, 15, 0, None, p, None, None) == inv and b"NULL" in err()
    assert call(h, p, p, None, 1, 0, 15, 2, None, p, None, None) == inv and b"flag" in err()
    assert call(h, p, p, None, 1, 0, 15, 0, None, None, None, None) == inv and b"every output" in err()
    for tick in (1 << 15, 1 << 20, 0xFFFFFFFF, 0x80000000):
        assert call(h, p, p, None, 1, tick, 15, 1, None, p, None, C.byref(tot)) == inv, tick
        assert b"latest tick" in err()
    assert call(h, p, p, None, 1, (1 << 15) - 1, 15, 1, p, p, p, C.byref(tot)) == inv and b"not booted" in err()
    assert b"gs_traffic_census" in err()

"""Host half of the wire-format emitter against the REAL reference's bytes (no GPU).

``tests/golden/wire_*.json.gz`` (``oracle/gen_wire_fixture.py``) hold the reference's
``_make_syn_msg().SerializeToString()`` for pairs of nodes of golden scenarios.  The host encodes
the NodeIdPb table the device copies into every NodeDigest / NodeDelta, and the PacketPb framing
around the device's DigestPb / DeltaPb; both must reproduce the reference's bytes exactly.
"""

import gzip
import json
import os

import pytest
from helpers import GOLDEN, load_scenario
from pbread import fields

from aiocluster_amd.pbsize import nodeid_size
from aiocluster_amd.scenario import scenario_node_ids
from aiocluster_amd.wire import frame, node_id_pb, packet, varint

NAMES = ["trunc8", "sched16", "fdgc12", "simple3", "cold64", "bigval6", "bigsleep12",
         "keys5", "keys37", "keys21w"]


def load_wire(name):
    with gzip.open(os.path.join(GOLDEN, f"wire_{name}.json.gz"), "rt") as f:
        return json.load(f)


@pytest.mark.parametrize("name", NAMES)
def test_syn_framing_and_node_ids_match_reference(name):
    scen = load_scenario(name)
    ids = scenario_node_ids(scen)
    nid = [node_id_pb(x) for x in ids]
    for x, b in zip(ids, nid):  # the device packer prices NodeIds with pbsize (GS_R_NID_SIZE)
        assert len(b) == nodeid_size(x.name, x.generation_id, *x.gossip_advertise_addr, x.tls_name)
    w = load_wire(name)
    assert w["cases"]
    for r, s, q, syn_hex, _ in w["cases"]:
        syn = bytes.fromhex(syn_hex)
        top = fields(syn)
        assert top[0] == (1, 2, b"default-cluster")
        assert [f[0] for f in top] == [1, 2]
        synpb = fields(top[1][2])
        assert [f[0] for f in synpb] == [2]
        digest = synpb[0][2]
        assert packet("default-cluster", "syn", digest=digest) == syn
        for num, wt, nd in fields(digest):
            assert (num, wt) == (1, 2)
            sub = fields(nd)
            assert sub[0][0] == 1 and sub[0][2] in nid  # NodeIdPb bytes of a known node
            assert [f[0] for f in sub] == sorted(f[0] for f in sub)  # field-number order
            assert all(f[2] != 0 for f in sub[1:])  # proto3: zero scalars are omitted


def test_delta_fixture_structure():
    """DeltaPb bodies of the fixture: NodeDeltaPb fields in number order, max_version always present
    (proto3 ``optional``), kvs in increasing version order (state.py:373-374)."""
    seen_trunc = False
    for name in NAMES:
        for _, _, _, _, dhex in load_wire(name)["cases"]:
            for num, _, nd in fields(bytes.fromhex(dhex)):
                assert num == 1
                sub = fields(nd)
                nums = [f[0] for f in sub]
                assert nums == sorted(nums) and nums[-1] == 5
                vers = [dict((g[0], g[2]) for g in fields(f[2])).get(3, 0) for f in sub if f[0] == 4]
                assert vers == sorted(vers)
                seen_trunc |= len(vers) == 0
    assert not seen_trunc  # a NodeDelta is only sent with at least one kv (state.py:403)


@pytest.mark.parametrize("name", ["bigval6", "bigsleep12"])
def test_large_value_fixtures_hold_long_bodies_and_mtu_cuts(name):
    """What the large-value wire fixtures are for: a NodeDelta body of 16,384 bytes or more (a 3-byte length
    prefix) and a NodeDelta the mtu cut; bigsleep12 also a NodeDelta field of 65,536 bytes or more and one of
    exactly 65,536 (tests/bigvalues.py: the designated owner's)."""
    w = load_wire(name)
    assert w["truncated"] and all(0 <= i < len(w["cases"]) for i in w["truncated"])
    bodies, values = [], []
    for _, _, _, _, dhex in w["cases"]:
        for num, _, nd in fields(bytes.fromhex(dhex)):
            bodies.append(len(nd))
            values += [len(g[2]) for f in fields(nd) if f[0] == 4 for g in fields(f[2]) if g[0] == 2]
    assert max(bodies) >= 1 << 14
    assert max(values) == (1 << 14) - 1 or name != "bigval6"  # the value limit itself is on the wire
    if name == "bigsleep12":
        fld = [1 + len(varint(b)) + b for b in bodies]  # the node_deltas field: tag, length, body
        assert max(fld) > 1 << 16 and (1 << 16) in fld
        # SET only: a NodeDelta whose last kv is below its max_version was cut by the mtu
        cut = 0
        for i in w["truncated"]:
            for _, _, nd in fields(bytes.fromhex(w["cases"][i][4])):
                sub = fields(nd)
                vers = [dict((g[0], g[2]) for g in fields(f[2])).get(3, 0) for f in sub if f[0] == 4]
                cut += vers[-1] < sub[-1][2]
        assert cut >= len(w["truncated"])


def test_packet_kinds_and_frame():
    d, e = b"\x0a\x01x", b"\x0a\x01y"
    assert packet("c", "synack", digest=d, delta=e) == b"\x0a\x01c" + b"\x1a" + varint(10) + b"\x12\x03" + d + b"\x1a\x03" + e
    assert packet("", "ack", delta=b"") == b"\x22\x02\x1a\x00"
    assert frame(b"abc") == b"\x00\x00\x00\x03abc"

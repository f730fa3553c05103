"""k_pass1v's record scatter (emit_v) on constructed stale-owner patterns (GPU only).

One phase on 8-bit views (GS_HB8 + GS_MV8), K = 4, at N = 2,048 (each wave owns one 1,024-column step) and
N = 4,096 + 48 (row halves of 3,072 and 1,072 columns: the unrolled second step, a third step, and a last step
with three lanes of columns and 61 past the end).  Every case is one exchange of that phase; its stale owners are
chosen per lane of a step: after two quiet rounds every view of every owner is equal, the chosen owners write
once, every third of them twice (gs_owner_writes), and the sender row of each case gets those owners' new max_version views, as an earlier
phase that delivered them would have left them.  The exchange must then record exactly those owners:

* the lists' counts (GS_R_CAND_N) and records (GS_R_CAND: column order, sender | receiver max_version words),
  and from the step whose owners overflow GS_CAND_CAP on, the bitmap words (GS_R_SLICE_BITS);
* the rows of every exchange and the counters against the C oracle (``oracle/rowcheck.py``), bit for bit.

The expected counts are part of the check: a case that degenerates (no records, no overflow, no delta cut short
by the MTU) fails.
"""

import numpy as np
import pytest
from rowcheck import check_phase_rows

from aiocluster_amd import driver
from aiocluster_amd.scenario import DEFAULT_CFG
from aiocluster_amd.sim import GossipSim
from aiocluster_amd.workload import WorkloadSpec, key_names, synthetic_node_ids

pytestmark = pytest.mark.gpu

K = 4
CAP = 1024  # GS_CAND_CAP
STEP = 1024  # columns per wave step: 64 lanes x 16

# columns of a lane holding 0, 1, 2, 3, 15 and 16 stale owners
LANE_COLS = {0: [], 1: [7], 2: [0, 15], 3: [3, 4, 12], 15: [i for i in range(16) if i != 8], 16: list(range(16))}


def _lane(base, lane, cols):
    return {base + 16 * lane + i for i in cols}


def _counts(base, lane0, ncol):
    """lanes lane0 .. lane0 + 5 of the step at ``base`` holding 0, 1, 2, 3, 15, 16 stale owners (lanes with columns
    below ``ncol`` only)"""
    out = set()
    for d, cnt in enumerate((0, 1, 2, 3, 15, 16)):
        out |= _lane(base, lane0 + d, LANE_COLS[cnt])
    return {c for c in out if c < ncol}


def _cases(n):
    """(name, a, b, ba, ab, overflows): stale owners b -> a (b holds the newer view) and a -> b, as column sets.
    The exchanges' own nodes sit in the last full step (N = 2,048: its lanes 40 .. 59, among the patterns of other
    exchanges; else its lanes 0 .. 39), unless a case is about them."""
    if n == 2048:
        bases, node0 = [0, 1024], 1024 + 16 * 40
    else:
        bases, node0 = [1024, 2048, 4096], 3072  # wave 0's steps 1 and 2, wave 1's ragged step 1
    nodes = iter(range(node0, node0 + 16 * (20 if n == 2048 else 40), 16))

    def pair():
        return next(nodes) + 3, next(nodes) + 9

    cases = []
    for base in bases:
        ragged = base + STEP > n  # three lanes of columns
        lanes = (n - base) // 16 if ragged else 64
        a, b = pair()
        cases.append((f"counts-ba@{base}", a, b, _counts(base, 0 if ragged else 2, n), set(), False))
        a, b = pair()
        cases.append((f"counts-ab@{base}", a, b, set(), _counts(base, 0 if ragged else 10, n), False))
        a, b = pair()
        # both directions in one step, the lanes overlapping: a lane's columns split between the directions
        ba = _counts(base, 0 if ragged else 20, n)
        ab = {c for c in _counts(base, 0 if ragged else 22, n) | _lane(base, 0 if ragged else 24, range(16)) if c < n}
        cases.append((f"counts-both@{base}", a, b, ba, ab - ba, False))
        a, b = pair()
        last = lanes - 1
        cases.append((f"lanes-0-{last}@{base}", a, b, _lane(base, 0, [0, 5]) | _lane(base, last, [15]),
                      _lane(base, 0, [9]) | _lane(base, last, [1, 2]), False))
        a, b = pair()
        cases.append((f"one-per-lane@{base}", a, b, {base + 16 * l + (5 * l) % 16 for l in range(lanes)},
                      {base + 16 * l + (5 * l + 7) % 16 for l in range(lanes)}, False))
    # the exchange's own columns (the per-column path's groups) inside a step that also has byte-parallel
    # records: a and b both wrote (a's own view of a is newer than b's: a -> b at column a; b -> a at column b)
    base = bases[0]
    a, b = base + 16 * 6 + 4, base + 16 * 12 + 8
    ba = {b, b + 1, b - 1} | _lane(base, 7, [0, 9]) | _lane(base, 30, [15])
    ab = {a, a + 1, a - 4} | _lane(base, 0, [2]) | _lane(base, 7, [3]) | _lane(base, 12, [0])
    cases.append((f"slow-groups@{base}", a, b, ba, ab, False))
    if n > 2048:
        # b -> a passes GS_CAND_CAP in the middle of wave 0's second step (700 owners in each of steps 0 and 1:
        # record 1,024 is lane 20's fifth), with more owners in step 2; a -> b has a few records in those steps
        a, b = pair()
        ba = set()
        for base in (0, 1024):
            ba |= {base + c for c in range(16 * 44) if c % 176 != 3}
        ba |= _counts(2048, 5, n) | _lane(2048, 63, [15])
        ab = _lane(0, 50, [1]) | _lane(1024, 20, [0, 1]) | _lane(1024, 63, [15]) | _lane(2048, 7, [4])
        cases.append(("cap-mid-step", a, b, ba, ab - ba, True))
    return cases


@pytest.mark.parametrize("n", [2048, 4096 + 48])
def test_constructed_stale_owners_are_recorded_and_match_the_oracle(n):
    import torch

    cfg = dict(DEFAULT_CFG)
    cfg["mtu"] = 16000  # cuts the overflowing case's delta short, the others fit
    spec = WorkloadSpec(n=n, k=K, fanout=3, seed=3, init="warm", write_frac=0.0)
    sim = GossipSim(synthetic_node_ids(n), key_names(K), cfg, init="warm", tombstones=False, fd_ring=False,
                    hist_cap=16, initial_ops=driver.boot_ops(n, K), hb8=True, mv8=True)
    plans = driver.prepare(spec, 3, torch, sim.device)
    for r in range(2):
        driver.run_round([sim], plans[r])
    sim.check()
    np_, H = sim.np_, ((n + 1) // 2 + 1023) & ~1023  # half_cols: wave w streams columns [w H, min((w + 1) H, n))
    mv = sim.region("MV", torch.uint8, (n, np_))
    assert int((mv[:, :n] != K).sum().item()) == 0  # every view: the K boot writes, no holes

    cases = _cases(n)
    nodes = [x for _, a, b, *_ in cases for x in (a, b)]
    assert len(set(nodes)) == len(nodes) and max(nodes) < n
    rd = dict(plans[2])
    wrote = sorted(set().union(*[ba | ab for _, _, _, ba, ab, _ in cases]))
    assert max(wrote) < n
    # a node that is among the writers (a stale owner of another case): its own view of itself is the newer one
    cases = [(name, a, b, ba | ({b} & set(wrote)), ab | ({a} & set(wrote)), over) for name, a, b, ba, ab, over in cases]
    ops = np.zeros((len(wrote), 5), dtype=np.uint32)
    ops[:, 0] = wrote
    ops[:, 3] = (1 << 25) + np.arange(len(wrote))
    ops[:, 4] = 9
    sim.owner_writes(ops, rd["t"])
    # every third owner writes a second key: a record's sender word then tells its column from its neighbours'
    twice = [j for j in wrote if j % 3 == 0]
    ops = np.zeros((len(twice), 5), dtype=np.uint32)
    ops[:, 0] = twice
    ops[:, 1] = 1
    ops[:, 3] = (1 << 26) + np.arange(len(twice))
    ops[:, 4] = 5
    sim.owner_writes(ops, rd["t"])
    for _, a, b, ba, ab, _ in cases:
        for row, cols in ((b, ba - {b}), (a, ab - {a})):  # (a node's own column holds its write already)
            assert a not in cols and b not in cols
            if cols:
                cj = torch.as_tensor(sorted(cols), device=sim.device, dtype=torch.long)
                mv[row, cj] = mv[cj, cj]
    a_t = torch.as_tensor([c[1] for c in cases], dtype=torch.int32, device=sim.device)
    b_t = torch.as_tensor([c[2] for c in cases], dtype=torch.int32, device=sim.device)
    rd["phases"] = [(a_t, b_t, len(cases), rd["phases"][0][3])]
    before = sim.check()
    driver.begin([sim], rd)
    diff, info = check_phase_rows(sim, cfg, rd, sample=len(cases), phase=0)
    assert diff is None, diff
    c = sim.check()
    got = {k: c[k] - before[k] for k in ("exchanges", "node_deltas", "hb_reports", "truncated", "lite_slots")}
    print(n, got, info)
    # the counters against the oracle's (the sample is the whole phase)
    for k in ("node_deltas", "hb_reports", "truncated"):
        assert got[k] == info[k], (k, got, info)
    assert got["exchanges"] == len(cases)
    # every stale owner is one NodeDelta (`truncated`, the NodeDeltas sent in part, is the oracle's above), and every
    # slot fits the MTU whole on the lite path -- but the overflowing direction, which the MTU cuts short and the
    # exact packer takes
    stale = sum(len(ba) + len(ab) for _, _, _, ba, ab, _ in cases)
    cut = sum(over for *_, over in cases)
    assert cut == (n > 2048)
    assert got["lite_slots"] == 2 * len(cases) - cut, got
    assert got["node_deltas"] == stale if not cut else 0 < stale - got["node_deltas"] < 1438, (got, stale)

    ne = len(cases)

    def head(name, dt, shape):  # the first ne exchanges' part of a per-exchange region
        return sim.region(name, dt, (-1,))[: ne * int(np.prod(shape))].view(ne, *shape).cpu().numpy()

    cand_n = head("CAND_N", torch.int32, (2, 2))
    cand = head("CAND", torch.int32, (2, 2, CAP, 2)).view(np.uint32)
    bits = head("SLICE_BITS", torch.int16, (2, np_ // 16)).view(np.uint16)

    def words(cols):  # sender view | receiver view << 16, both without holes
        return [(K + 1 + (x % 3 == 0)) | (K << 16) for x in cols]

    for e, (name, a, b, ba, ab, over) in enumerate(cases):
        hit = False
        for d, cols in enumerate((ba, ab)):
            for hf in range(2):
                want = sorted(x for x in cols if hf * H <= x < (hf + 1) * H)
                assert cand_n[e, d, hf] == len(want), (name, d, hf, cand_n[e].tolist(), len(want))
                m = min(len(want), CAP)
                assert cand[e, d, hf, :m, 0].tolist() == want[:m], (name, d, hf)
                assert cand[e, d, hf, :m, 1].tolist() == words(want[:m]), (name, d, hf)
                if len(want) > CAP:
                    # from the step of record CAP + 1 on: one u16 per lane, bit i = column 16 g + i
                    hit = True
                    s0 = hf * H + (want[CAP] - hf * H) // STEP * STEP
                    end = min((hf + 1) * H, n)
                    assert s0 + STEP < end and want[CAP] % 16 and any(x >= s0 + STEP for x in want)
                    wmask = np.zeros(np_ // 16, np.uint16)
                    for x in want:
                        wmask[x >> 4] |= np.uint16(1 << (x & 15))
                    g0, g1 = s0 // 16, (end + 15) // 16
                    assert bits[e, d, g0:g1].tolist() == wmask[g0:g1].tolist(), (name, d, hf)
        assert hit == over, name
        assert len(ba) + len(ab) > 0, name
    # what the cases are named for
    by = {c[0].split("@")[0]: e for e, c in enumerate(cases)}
    full = [e for e, c in enumerate(cases) if c[0].startswith("one-per-lane") and len(c[3]) == 64]
    assert full and all(64 in cand_n[e, 0] and 64 in cand_n[e, 1] for e in full)  # 64 records from level 0 alone
    e = by["slow-groups"]
    assert cases[e][1] in cand[e, 1, 0, :, 0] and cases[e][2] in cand[e, 0, 0, :, 0]  # columns a and b recorded
    sim.close()

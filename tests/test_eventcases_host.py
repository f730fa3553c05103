"""The scenarios of tests/eventcases.py on the C oracle alone (CPU): each has the properties its GPU case in
tests/test_gpu_events_layouts.py relies on, so that case never passes because its input was tame."""

import numpy as np
from eventcases import cold_k64, warm_k16_esc, warm_k37
from helpers import make_backend
from oracle import OracleSim

from aiocluster_amd.scenario import replay_round


def run(scen):
    orc = make_backend(OracleSim, scen)
    orc.enable_events()
    ev = []
    for r in range(len(scen["rounds"])):
        replay_round(orc, scen, r)
        ev.append(orc.drain_events().astype(np.int64))
    s = orc.stats()
    orc.close()
    return np.concatenate(ev), s


def test_cold_k64_truncates_and_reports_keys_past_31():
    scen = cold_k64()
    assert scen["k"] == 64 and scen["n"] == 32 and scen["init"] == "cold"
    assert {op for rd in scen["rounds"] for _, _, op, _ in rd["writes"]} == {0, 1, 2, 3}  # set, delete, both TTL ops
    ev, s = run(scen)
    assert s["truncated"] > 0
    kind, key = ev[:, 2] >> 8, ev[:, 2] & 0xFF
    assert set(kind.tolist()) == {0, 1, 2}
    applied = (kind == 0) & (ev[:, 0] != ev[:, 1])  # apply_delta's records: the observer is not the owner
    assert (key[applied] >= 32).sum() > 100 and key[applied].max() == 63
    assert ((kind == 0) & (ev[:, 0] == ev[:, 1]) & (key >= 32)).any()  # owner writes too


def test_warm_k37_truncates_and_reports_keys_up_to_36():
    scen = warm_k37()
    assert scen["k"] == 37 and scen["n"] == 96 and scen["init"] == "warm"
    assert {op for rd in scen["rounds"] for _, _, op, _ in rd["writes"]} == {0}  # SET only: prefix views
    ev, s = run(scen)
    assert s["truncated"] > 0
    kind, key = ev[:, 2] >> 8, ev[:, 2] & 0xFF
    assert set(kind.tolist()) == {0, 1, 2}
    applied = (kind == 0) & (ev[:, 0] != ev[:, 1])  # apply_delta's records: the observer is not the owner
    assert (key[applied] >= 32).any() and key[applied].max() == 36


def test_warm_k16_esc_truncates_with_churn():
    scen = warm_k16_esc()
    assert scen["k"] == 16 and scen["n"] == 128 and scen["init"] == "warm"
    ev, s = run(scen)
    assert s["truncated"] > 0
    kind = ev[:, 2] >> 8
    assert set(kind.tolist()) == {0, 1, 2}
    assert ((ev[:, 2] & 0xFF)[kind == 0] >= 8).any()

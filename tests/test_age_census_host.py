"""gs_age_census / gs_note_writes on the host (CPU): struct layout, constants, argument checks, the numpy mirror of
gs_note_writes, the numpy reference the GPU tests compare the device with (tests/ageref.py) on a hand-made case, and
the histogram-to-bound helpers.

The argument checks come before any HIP call, so a handle from gs_create alone is enough, as in
tests/test_detect_census_host.py.
"""

import ctypes as C
import math
import re

import numpy as np
import pytest
from ageref import BUCKETS, GS_NONE, age_census_ref, bucket, hist_of

from aiocluster_amd import _lib, staleness


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


def test_totals_struct_is_80_words():
    T = _lib.GsAgeTotals
    assert C.sizeof(T) == 80 * 8
    assert len(_lib.AGE_TOTAL_FIELDS) == 11
    assert T.observers.offset == 0 and T.max_pending_age.offset == 10 * 8
    assert T.age_hist.offset == 11 * 8
    assert T.spread_hist.offset == (11 + _lib.GS_AC_BUCKETS) * 8
    assert T.pending_age_hist.offset == (11 + 2 * _lib.GS_AC_BUCKETS) * 8
    assert T.reserved.offset == (11 + 3 * _lib.GS_AC_BUCKETS) * 8


def test_header_and_binding_agree():
    src = open(_lib.HEADER).read()
    for name, want in (("GS_AC_BUCKETS", _lib.GS_AC_BUCKETS), ("GS_VC_BUCKETS", _lib.GS_VC_BUCKETS),
                       ("GS_API_VERSION", _lib.API_VERSION)):
        m = re.search(rf"^#define {name} (\d+)u?\b", src, re.M)
        assert m and int(m.group(1)) == want, name
    assert (_lib.GS_AC_BUCKETS, _lib.API_VERSION, BUCKETS) == (20, 23, 20)
    for fn in ("gs_write_log_words", "gs_write_log_init", "gs_note_writes", "gs_age_census"):
        assert fn in _lib.EXPORTS
    body = re.search(r"typedef struct gs_age_totals \{(.*?)\} gs_age_totals;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\w+\])?\s*[,;]", body)
    assert names == [f[0] for f in _lib.GsAgeTotals._fields_]
    # no new region: the log is the caller's
    assert len(_lib.REGIONS) == 37 and not any("LOG" in r and r != "VLOG" for r in _lib.REGIONS)


def test_write_log_words(handle):
    lib, h = handle
    wl = C.c_uint32()
    assert lib.gs_write_log_words(h, C.byref(wl)) == 0
    assert wl.value == _lib.write_log_words(16, 32) == 500  # 16 * 31 + 1 = 497, rounded up to 4
    assert _lib.write_log_words(4, 16) == 64 and _lib.write_log_words(2, 8) == 16 and _lib.write_log_words(1, 2) == 4
    assert lib.gs_write_log_words(None, C.byref(wl)) == _lib.GS_E_INVALID


def test_argument_errors_return_invalid(handle):
    lib, h = handle
    tot = _lib.GsAgeTotals()
    inv = _lib.GS_E_INVALID
    log = C.c_void_p(0x1000)  # never dereferenced: every check below comes before any device work
    assert lib.gs_age_census(None, None, log, 0, 0, None, None, None, C.byref(tot)) == inv
    assert lib.gs_age_census(h, None, None, 0, 0, None, None, None, C.byref(tot)) == inv
    assert b"gs_age_census" in lib.gs_last_error(h) and b"wlog" in lib.gs_last_error(h)
    assert lib.gs_age_census(h, None, log, 0, 0, None, None, None, None) == inv
    assert b"gs_age_census" in lib.gs_last_error(h) and b"out" in lib.gs_last_error(h)
    for flags in (1, 2, 0x80000000):
        assert lib.gs_age_census(h, None, log, 0, flags, None, None, None, C.byref(tot)) == inv
        assert b"gs_age_census" in lib.gs_last_error(h) and b"flags" in lib.gs_last_error(h)
    t = C.c_uint32()
    assert lib.gs_latest_tick(h, C.byref(t)) == 0 and t.value == 0
    for tick in (1 << 15, (1 << 15) + 7, 0xFFFFFFFF):  # 2^15 or more past the latest tick; before it (mod 2^32)
        assert lib.gs_age_census(h, None, log, tick, 0, None, None, None, C.byref(tot)) == inv
        assert b"gs_age_census" in lib.gs_last_error(h) and b"tick" in lib.gs_last_error(h)
    assert lib.gs_note_writes(h, 0, None) == inv and b"gs_note_writes" in lib.gs_last_error(h)
    assert lib.gs_write_log_init(h, None) == inv and b"gs_write_log_init" in lib.gs_last_error(h)
    assert lib.gs_note_writes(None, 0, log) == inv and lib.gs_write_log_init(None, log) == inv


def test_note_writes_host_logs_each_version_once_and_no_ops_nothing():
    log = staleness.new_log_host(3, 8)
    assert log.dtype == np.uint32 and (log == GS_NONE).all()
    mv = np.array([0, 0, 0])
    staleness.note_writes_host(log, mv, 5)  # nothing written yet: version 0 is never logged
    assert (log == GS_NONE).all()
    mv = np.array([1, 0, 1])  # owners 0 and 2 set a key
    staleness.note_writes_host(log, mv, 10)
    assert log[0, 1] == 10 and log[2, 1] == 10 and (log[1] == GS_NONE).all()
    # a same-value set / a delete of an absent key: max_version unchanged, the later tick is not logged
    staleness.note_writes_host(log, mv, 20)
    assert log[0, 1] == 10 and log[2, 1] == 10 and (log == GS_NONE).sum() == log.size - 2
    mv = np.array([2, 1, 1])  # owner 0 deletes its key (version 2), owner 1 sets one
    staleness.note_writes_host(log, mv, 30)
    assert log[0].tolist()[:3] == [GS_NONE, 10, 30] and log[1, 1] == 30 and log[2, 1] == 10
    # a batch nobody noted (owner 0: version 3), then a noted one (version 4): 3 stays GS_NONE
    mv = np.array([4, 1, 1])
    staleness.note_writes_host(log, mv, 40)
    assert log[0].tolist()[:5] == [GS_NONE, 10, 30, GS_NONE, 40]
    assert (log[:, 0] == GS_NONE).all()  # entry 0 is unused
    with pytest.raises(ValueError):
        staleness.note_writes_host(log, np.array([1, 2]), 1)


def test_reference_on_a_hand_made_case():
    """4 observers x 4 owners at tick 100.  Owners' versions M = [3, 2, 1, 4]; log ticks below.
    Observer 1 does not know owner 2 (a view at version 0); owner 3's version 3 was never noted."""
    N = GS_NONE
    M = [3, 2, 1, 4]
    log = np.array([[N, 10, 50, 90, N, N, N, N],
                    [N, 10, 60, N, N, N, N, N],
                    [N, 40, N, N, N, N, N, N],
                    [N, 10, 20, N, 96, N, N, N]], dtype=np.uint32)
    ver = np.array([[3, 2, 1, 4],
                    [2, 2, 7, 2],    # (1, 2) is unknown: its stored version is ignored
                    [1, 1, 1, 3],
                    [3, 0, 1, 4]])
    known = np.ones((4, 4), bool)
    known[1, 2] = False
    got = age_census_ref(ver, known, M, log, 100, done=np.zeros(4, np.int64))
    # behind: (1,0) lacks v3 -> age 10; (1,2) unknown lacks v1 -> 60; (1,3) lacks v3 -> unlogged; (2,0) lacks v2 -> 50;
    # (2,1) lacks v2 -> 40; (2,3) lacks v4 -> 4; (3,1) lacks v1 -> 90
    assert (got["observers"], got["pairs"], got["unknown"], got["behind"], got["unlogged"]) == (4, 16, 1, 7, 1)
    assert got["max_age"] == 90
    assert got["age_hist"] == hist_of([10, 60, 50, 40, 4, 90]) and sum(got["age_hist"]) == 6
    assert got["age_hist"][bucket(4)] == 1 and bucket(4) == 3 and bucket(90) == 7
    assert got["row_max_age"].tolist() == [0, 60, 50, 90]
    assert got["owner_floor"].tolist() == [1, 0, 0, 2]
    # spread from done = 0: owner 0 v1 (latency 90); owner 3 v1, v2 (90, 80).  Pending: owner 0 v2, v3 (50, 10);
    # owner 1 v1, v2 (90, 40); owner 2 v1 (60); owner 3 v3 unlogged, v4 (4)
    assert (got["spread_writes"], got["pending_writes"], got["unlogged_writes"]) == (3, 6, 1)
    assert got["max_spread_latency"] == 90 and got["max_pending_age"] == 90
    assert got["spread_hist"] == hist_of([90, 90, 80]) and got["pending_age_hist"] == hist_of([50, 10, 90, 40, 60, 4])
    assert got["done"].tolist() == [1, 0, 0, 2]
    # the second call, at tick 130: everyone caught up except observer 2 on owner 3 (still at v3), and observer 3 is
    # masked out; `done` carries over, so nothing is credited twice
    ver2 = np.array([[3, 2, 1, 4], [3, 2, 1, 4], [3, 2, 1, 3], [0, 0, 0, 0]])
    got2 = age_census_ref(ver2, np.ones((4, 4), bool), M, log, 130, up=[1, 1, 1, 0], done=got["done"])
    assert (got2["observers"], got2["pairs"], got2["unknown"], got2["behind"], got2["unlogged"]) == (3, 12, 0, 1, 0)
    assert got2["max_age"] == 34 and got2["row_max_age"].tolist() == [0, 0, 34, 0]
    assert got2["owner_floor"].tolist() == [3, 2, 1, 3]
    # credited now: owner 0 v2, v3 (80, 40); owner 1 v1, v2 (120, 70); owner 2 v1 (90); owner 3 v3 is unlogged
    assert (got2["spread_writes"], got2["pending_writes"], got2["unlogged_writes"]) == (5, 1, 1)
    assert got2["spread_hist"] == hist_of([80, 40, 120, 70, 90]) and got2["max_spread_latency"] == 120
    assert got2["pending_age_hist"] == hist_of([34]) and got2["max_pending_age"] == 34
    assert got2["done"].tolist() == [3, 2, 1, 3]
    # a third call on the same state credits nothing; a node that comes back behind does not un-credit
    ver3 = ver2.copy()
    ver3[0, 0] = 1
    got3 = age_census_ref(ver3, np.ones((4, 4), bool), M, log, 140, up=[1, 1, 1, 0], done=got2["done"])
    assert got3["spread_writes"] == 0 and got3["done"].tolist() == [3, 2, 1, 3]
    assert got3["owner_floor"].tolist() == [1, 2, 1, 3] and got3["pending_writes"] == 1  # owner 3's v4 only
    # without done: no spread, pending = the writes above the floor; no observers: the owner pass is skipped
    got4 = age_census_ref(ver3, np.ones((4, 4), bool), M, log, 140, up=[1, 1, 1, 0])
    assert got4["spread_writes"] == 0 and got4["pending_writes"] == 3 and got4["done"] is None
    got5 = age_census_ref(ver3, np.ones((4, 4), bool), M, log, 140, up=[0, 0, 0, 0], done=got2["done"])
    assert got5["observers"] == got5["behind"] == got5["pending_writes"] == got5["unlogged_writes"] == 0
    assert got5["owner_floor"].tolist() == M and got5["done"].tolist() == [3, 2, 1, 3]


def test_histogram_bounds():
    assert [staleness.bucket(x) for x in (0, 1, 2, 3, 4, 63, 64, (1 << 18) - 1, 1 << 18, 1 << 25)] == \
        [0, 1, 2, 2, 3, 6, 7, 18, 19, 19]
    assert all(staleness.bucket(x) == bucket(x) for x in range(300))
    assert staleness.bucket_bound_ticks(0) == 0 and staleness.bucket_bound_ticks(1) == 2
    assert staleness.bucket_bound_ticks(7) == 128 and staleness.bucket_bound_ticks(19) == math.inf
    h = [0] * 20
    assert staleness.quantile_bound_ticks(h, 0.5) is None and staleness.quantile_bound_s(h, 0.99) is None
    h[0], h[3], h[7] = 50, 49, 1  # 50 zeros, 49 values in [4, 8), one in [64, 128)
    assert staleness.quantile_bound_ticks(h, 0.5) == 0
    assert staleness.quantile_bound_ticks(h, 0.51) == 8
    assert staleness.quantile_bound_ticks(h, 0.99) == 8
    assert staleness.quantile_bound_ticks(h, 1.0) == 128
    assert staleness.quantile_bound_s(h, 1.0) == 2.0 and staleness.ticks_to_s(64) == 1.0
    h[19] = 1
    assert staleness.quantile_bound_ticks(h, 1.0) == math.inf
    s = staleness.hist_summary(h, max_ticks=640)
    assert s == {"n": 101, "p50_s": 8 / 64, "p99_s": 2.0, "max_s": 10.0}  # the 51st and the 100th of 101 values
    with pytest.raises(ValueError):
        staleness.quantile_bound_ticks(h, 0.0)

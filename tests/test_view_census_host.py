"""gs_view_census argument checks and struct layout (CPU: no device call is reached).

The checks come before any HIP call, so a handle from gs_create alone (nothing bound, nothing booted) is
enough: every bad argument returns GS_E_INVALID.
"""

import ctypes as C

import pytest

from aiocluster_amd import _lib


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


def test_totals_struct_is_56_words():
    assert C.sizeof(_lib.GsViewTotals) == 56 * 8
    assert C.sizeof(_lib.GsProbe) == 8
    assert _lib.GsViewTotals.version_lag_hist.offset == 7 * 8
    assert _lib.GsViewTotals.heartbeat_lag_hist.offset == (7 + _lib.GS_VC_BUCKETS) * 8
    assert (_lib.GS_VC_HEARTBEATS, _lib.GS_VC_MAX_PROBES, _lib.GS_VC_BUCKETS) == (1, 64, 20)


def test_header_and_binding_agree_on_the_census_constants():
    import re

    src = open(_lib.HEADER).read()
    for name, want in (("GS_VC_HEARTBEATS", _lib.GS_VC_HEARTBEATS), ("GS_VC_MAX_PROBES", _lib.GS_VC_MAX_PROBES),
                       ("GS_VC_BUCKETS", _lib.GS_VC_BUCKETS), ("GS_API_VERSION", _lib.API_VERSION)):
        m = re.search(rf"^#define {name} (\d+)u?\b", src, re.M)
        assert m and int(m.group(1)) == want, name


def test_argument_errors_return_invalid(handle):
    lib, h = handle
    tot = _lib.GsViewTotals()
    reach = (C.c_uint64 * 65)()

    def probes(*pv):
        return (_lib.GsProbe * max(1, len(pv)))(*[_lib.GsProbe(j, v) for j, v in pv])

    one = probes((3, 1))
    call = lib.gs_view_census
    inv = _lib.GS_E_INVALID
    # n_probes > GS_VC_MAX_PROBES
    assert call(h, None, 0, probes(*[(i, 0) for i in range(65)]), 65, reach, None, None, C.byref(tot)) == inv
    # a probe owner >= N
    assert call(h, None, 0, probes((1000, 0)), 1, reach, None, None, C.byref(tot)) == inv
    assert call(h, None, 0, probes((0, 0), (0xFFFFFFFF, 0)), 2, reach, None, None, C.byref(tot)) == inv
    # out == NULL
    assert call(h, None, 0, one, 1, reach, None, None, None) == inv
    assert call(h, None, 0, None, 0, None, None, None, None) == inv
    # unknown flag bits
    for flags in (2, 4, 0x80000000, 3):
        assert call(h, None, flags, None, 0, None, None, None, C.byref(tot)) == inv, flags
    # n_probes > 0 with probes or reach NULL
    assert call(h, None, 0, None, 1, reach, None, None, C.byref(tot)) == inv
    assert call(h, None, 0, one, 1, None, None, None, C.byref(tot)) == inv
    assert b"gs_view_census" in lib.gs_last_error(h)
    assert call(None, None, 0, None, 0, None, None, None, C.byref(tot)) == inv

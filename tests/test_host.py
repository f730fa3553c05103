"""Host-side logic that needs no GPU (CPU): write batching, window packing, config, multi-rank aggregation."""

import os
import socket

import numpy as np
import pytest

from aiocluster_amd import _lib
from aiocluster_amd.scenario import DEFAULT_CFG
from aiocluster_amd.sim import make_config, split_owner_batches


def test_split_owner_batches_keeps_per_owner_order():
    ops = [(0, 1, "a"), (0, 2, "b"), (0, 1, "c"), (0, 1, "d"), (0, 3, "e"), (0, 2, "f")]
    batches = split_owner_batches(ops)
    for b in batches:
        owners = [op[1] for op in b]
        assert len(owners) == len(set(owners))
    flat = {}
    for b in batches:
        for op in b:
            flat.setdefault(op[1], []).append(op[2])
    assert flat == {1: ["a", "c", "d"], 2: ["b", "f"], 3: ["e"]}


def test_fd_window_decode():
    """GS_R_FD (sum | cnt << sum_bits) + GS_R_FD_LAST (tick mod 2^16) + GS_R_FD_STATE bits (window, old):
    the host decode restates the device's fd_get; exact while the last report is < 2^16 ticks old."""
    from aiocluster_amd.sim import FD_OLD, FD_OLD_AGE, FD_WIN, unpack_fd

    W = 1000
    sb = _lib.fd_sum_bits(W)
    assert sb == 21 and W * 640 < (1 << sb)
    rng = np.random.default_rng(0)
    t = 5_000_000
    last = t - rng.integers(0, 1 << 16, 100, dtype=np.int64)
    sm = rng.integers(0, 1 << sb, 100, dtype=np.uint64)
    cnt = rng.integers(0, 2 * W, 100, dtype=np.uint64)
    sc = (sm | (cnt << np.uint64(sb))).astype(np.uint32)
    st = np.full(100, FD_WIN | 1, np.uint8)
    st[:3] = 0  # no window
    st[3:6] |= FD_OLD
    l2, s2, c2 = unpack_fd(st, (last & 0xFFFF).astype(np.uint16), sc, t, sb)
    assert np.all(l2[:3] == _lib.GS_NONE)
    assert np.all(l2[3:6] == t - FD_OLD_AGE)
    assert np.array_equal(l2[6:], last[6:].astype(np.uint32))
    assert np.array_equal(s2, sm.astype(np.uint32)) and np.array_equal(c2, cnt.astype(np.uint32))


def test_make_config_ticks_and_rejects_fractional_ticks():
    c = make_config(100, 16, DEFAULT_CFG, 0, 32)
    assert c.max_interval_ticks == 640 and c.tombstone_grace_ticks == 7200 * 64
    assert c.dead_grace_ticks == 86400 * 64 and c.prior_weighted == 25.0
    bad = dict(DEFAULT_CFG, max_interval_s=0.01)
    with pytest.raises(ValueError):
        make_config(100, 16, bad, 0, 32)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, q):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench

    ex, tm = bench.aggregate(1000 * (rank + 1), 2.0 + rank, dist, "cpu")
    q.put((rank, ex, tm))
    dist.destroy_process_group()


def test_multi_rank_aggregation_gloo():
    """bench.py's N>1 reduction (exchanges summed, time = max over ranks), world_size 2 on gloo."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
    assert [o[1:] for o in out] == [(3000.0, 3.0), (3000.0, 3.0)]


class _ExportOnly:
    """The part of GossipSim that bench.dump_outputs reads: n, ncol, export_rows (the oracle's export format)."""

    def __init__(self, n, k):
        self.n = self.ncol = n
        self.k = k
        self.asked = []

    def export_rows(self, rows):
        import numpy as np

        self.asked.append(np.asarray(rows).copy())
        r, n, k = len(rows), self.n, self.k
        view = np.asarray(rows)[:, None] * 7 + np.arange(n)[None, :]
        kv = view[:, :, None] + np.arange(k)[None, None, :]
        return {"hb": view.astype(np.uint32), "fd_sum": view / 64.0, "fd_last": (view + (1 << 30)).astype(np.int64),
                "kv_version": kv.astype(np.uint32), "kv_value_id": (kv + (1 << 24) + 1).astype(np.uint32)}


def test_bench_dump_outputs_writes_a_fixed_sample_as_float_arrays(tmp_path):
    """bench.py --dump-outputs: the same seeded rows and columns every time, per-view arrays over every column,
    per-key arrays over the drawn columns, the counters in COUNTER_FIELDS order; float32 / float64 .npy files
    that hold the exported integers exactly, within 64 MB."""
    import numpy as np

    import bench
    from aiocluster_amd import _lib

    n, k = 5000, 3
    counters = {f: (1 << 40) + i for i, f in enumerate(_lib.COUNTER_FIELDS)}
    sims = [_ExportOnly(n, k), _ExportOnly(n, k)]
    shapes = [bench.dump_outputs(s, counters, str(tmp_path / f"o{i}")) for i, s in enumerate(sims)]
    assert shapes[0] == shapes[1]
    rows = sims[0].asked[0]
    assert len(rows) == bench.DUMP_ROWS and np.array_equal(rows, sims[1].asked[0]) and len(set(rows.tolist())) == len(rows)
    got = {f[:-4]: np.load(tmp_path / "o0" / f) for f in sorted(os.listdir(tmp_path / "o0"))}
    assert set(got) == {"sample_rows", "sample_cols", "counters", "hb", "fd_sum", "fd_last", "kv_version", "kv_value_id"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    cols = got["sample_cols"].astype(np.int64)
    assert len(cols) == bench.DUMP_COLS and np.all(np.diff(cols) > 0) and cols[-1] < n
    want = sims[0].export_rows(rows)
    assert got["hb"].shape == (len(rows), n) and got["kv_version"].shape == (len(rows), len(cols), k)
    assert np.array_equal(got["hb"], want["hb"]) and np.array_equal(got["fd_sum"], want["fd_sum"])
    assert np.array_equal(got["fd_last"], want["fd_last"])  # above 2^24: binary64
    assert np.array_equal(got["kv_value_id"], want["kv_value_id"][:, cols])
    assert np.array_equal(got["kv_version"], want["kv_version"][:, cols])
    assert got["counters"].tolist() == [float(counters[f]) for f in _lib.COUNTER_FIELDS]
    for f in os.listdir(tmp_path / "o0"):
        assert np.array_equal(np.load(tmp_path / "o0" / f), np.load(tmp_path / "o1" / f)), f

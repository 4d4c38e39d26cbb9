#!/usr/bin/env python3
"""Measure cndpfwd's fwd, l3fwd and ACL modes over the mbuf queue
(cndp_gpu_mq_create_fwd, include/cndp_mqfwd.h) against the host twins on one core.

    python tools/cndpfwd_mq_bench.py [--pool 65536] [--reps 7] [--out profiles/cndpfwd_mq_bench.json]

One lcore, as cndpfwd's thread_func loop: a pool of --pool mbufs (2 KiB each,
frames at data_off 256, as CNDP's pktmbuf pool lays them out) is handed to the
queue in 256-mbuf bursts -- submit, then poll, draining whatever has finished --
and the pass ends when every mbuf is back (pending == 0: poll's load of the
batch's completion flag is the synchronisation, so the clock stops after the
last result is on the host).  Both forms: zero-copy (the pool registered, the
kernels read and edit the frames over PCIe) and staged (the host copies 16 / 48
bytes a frame into pinned staging and the changed bytes back).

The CPU figure is the twin of each mode -- cndp_cfwd_host, cndp_acl_classify_host
-- on the same thread over the same pool in one call: slab = the pool, stride
2048, data_off 256, len from the mbufs.

Frames: 64-byte IPv4/UDP; ACL runs cndpfwd's 4226 default rules (strict, with
MAC_SWAP), and the addresses hit its four families and miss in equal parts;
l3fwd's FIB has a /8, a /16, 256 /24s and 1024 /32s behind them (tbl8 groups),
so a fifth of the lookups takes the second gather (tbl8), a fifth ends at the
/8 and three fifths miss.

Method: per case --warmup untimed windows, then --reps timed ones, each window
--passes passes over the pool back to back (one pass of 64Ki mbufs is under a
millisecond, too short to time alone); the median and the min-max of the
windows' rates are reported, and every window's seconds are kept in the JSON.
The loop is driven from Python through ctypes; what two foreign calls a burst
cost with nothing to do is measured the same way (calls_us_per_burst) so that
it can be told apart from the library's own time.  --dry builds a small pool
and runs the set-up on the CPU (each twin's mix of edges, the bytes it changes)
without timing anything; without a GPU nothing else runs.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cndp_amd import native as N                                   # noqa: E402
from cndp_amd.acl import AclTable, acl_io, default_n_bins          # noqa: E402
from cndp_amd.cfwd import cfwd_io, l3fwd_fib, route_add            # noqa: E402
from cndp_amd.mbuf import FRAME, MbufPool, MbufQueue               # noqa: E402

BURST = 256
IN_LPORT, LPORTS = 0, (0, 1, 2, 3)
MODES = (("fwd", N.CNDP_MQ_CFWD_FWD), ("l3fwd", N.CNDP_MQ_CFWD_L3FWD), ("acl", N.CNDP_MQ_ACL_FWD))


def build_fib():
    fib = l3fwd_fib("mq-bench")
    route_add(fib, 0x64000000, 8, "02:00:00:00:01:00", 1)
    route_add(fib, 0x6E000000, 16, "02:00:00:00:02:00", 2)
    for k in range(256):
        route_add(fib, 0x6E000000 | (k << 8), 24, bytes([2, 0, 0, 1, k, 0]), 1 + k % 3)
    for k in range(1024):
        route_add(fib, 0x6E000000 | ((k & 255) << 8) | (7 + 13 * (k >> 8)), 32, bytes([2, 0, 0, 2, k & 255, k >> 8]), k % 4)
    return fib


def build_pool(n, seed=1):
    """Frame i by i % 5: allowed (210.0.h.l -> 110.0.h.l, the /24s and /32s of the
    FIB), denied by dst (100.k.0.x, the /8), by src /8 and src /24, and unmatched
    (a FIB miss)."""
    rng = np.random.default_rng(seed)
    fam, j = np.arange(n) % 5, np.arange(n) // 5
    rnd = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.int64)
    hl = (j * 2654435761) % 4096
    hl = np.where(j % 2 == 0, (hl & 0xFF00) | 7, hl)              # every other allowed frame behind a /32
    src = np.select([fam == 0, fam == 2, fam == 3], [0xD2000000 | hl, ((10 + j % 15) << 24) | (rnd & 0xFFFFFF),
                                                      0x65000000 | ((j % 15) << 8) | (rnd & 0xFF)], 0x01010101)
    dst = np.select([fam == 0, fam == 1], [0x6E000000 | hl, 0x64000000 | ((j % 100) << 16) | (rnd & 0xFF)], 0x02020202)
    rows = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    rows[:, :14] = np.frombuffer(bytes.fromhex("0200000000010200000000aa0800"), np.uint8)
    rows[:, 5] = j % 5                                             # p[5]: ports 0-3 exist, 4 does not
    rows[:, 14:26] = np.frombuffer(bytes([0x45, 0, 0, 46, 0, 0, 0, 0, 64, 17, 0x12, 0x34]), np.uint8)
    for k in range(4):
        rows[:, 26 + k] = (src >> (24 - 8 * k)) & 0xFF
        rows[:, 30 + k] = (dst >> (24 - 8 * k)) & 0xFF
    pool = MbufPool(n)
    pool.mem.reshape(n, FRAME)[:, 256:256 + 64] = rows
    pool.hdr["data_len"] = 64
    return pool


class Twin:
    """One mode's host twin over the whole pool in one call, its arrays made once."""

    def __init__(self, name, pool, fib, acl):
        n = pool.n
        self.L, self.name, self.fib, self.acl = N.lib(), name, fib, acl
        self.b = N.Batch()
        self.b.n, self.b.slab, self.b.slab_len = n, pool.mem.ctypes.data, pool.mem.size
        self.b.stride, self.b.data_off = FRAME, 256
        self.len = np.ascontiguousarray(pool.hdr["data_len"])
        ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        nb = default_n_bins(IN_LPORT, LPORTS)
        if name == "acl":
            self.out = {"result": np.zeros(n, np.uint32), "verdict": np.zeros(n, np.uint8), "tx_lport": np.zeros(n, np.uint8),
                        "stats": np.zeros(N.CNDP_ACL_NSTATS, np.uint64)}
            self.io = acl_io(self.out, ptr, IN_LPORT, LPORTS, nb, length=self.len)
        else:
            self.out = {"tx_lport": np.zeros(n, np.uint16), "echoed": np.zeros(n, np.uint8),
                        "stats": np.zeros(N.CNDP_CFWD_NSTATS, np.uint64)}
            self.io = cfwd_io(self.out, ptr, IN_LPORT, LPORTS, nb)

    def run(self):
        if self.name == "acl":
            rc = self.L.cndp_acl_classify_host(self.acl.h, ctypes.byref(self.b), N.CNDP_ACL_STRICT, N.CNDP_ACL_F_MAC_SWAP,
                                               ctypes.byref(self.io))
        else:
            rc = self.L.cndp_cfwd_host(self.fib.h, ctypes.byref(self.b),
                                       N.CNDP_CFWD_L3FWD if self.name == "l3fwd" else N.CNDP_CFWD_FWD, ctypes.byref(self.io))
        N.check(rc, "host twin")

    def edges(self):
        if self.name == "acl":
            v = self.out["verdict"]
            return np.where(v == N.CNDP_ACL_FORWARD, self.out["tx_lport"].astype(np.uint16),
                            np.where(v == N.CNDP_ACL_DENY, N.CNDP_MQ_EDGE_ACL_DENY, N.CNDP_MQ_EDGE_ACL_PREFILTER)).astype(np.uint16)
        return self.out["tx_lport"] | (self.out["echoed"].astype(np.uint16) << 8)


class Loop:
    """cndpfwd's loop over the pool through one queue, its buffers made once."""

    def __init__(self, q, pool):
        self.L, self.q, self.n = N.lib(), q.h, pool.n
        self.ptrs = pool.ptrs(np.arange(pool.n))
        self.base = ctypes.addressof(self.ptrs)
        self.out = (ctypes.c_void_p * pool.n)()
        self.edges = np.zeros(pool.n, np.uint16)

    def run(self):
        """One pass; returns the edges in submission order."""
        L, q, n = self.L, self.q, self.n
        out, ed = ctypes.addressof(self.out), self.edges.ctypes.data
        got = 0
        for b in range(0, n, BURST):
            want = min(BURST, n - b)
            done = 0
            while done < want:
                k = L.cndp_gpu_mq_submit(q, self.base + 8 * (b + done), want - done)
                if k < 0:
                    raise OSError(-k, "cndp_gpu_mq_submit")
                done += k
                g = L.cndp_gpu_mq_poll(q, out + 8 * got, ed + 2 * got, n - got)
                got += g
                if k == 0 and g == 0:
                    L.cndp_gpu_mq_wait(q)
        while got < n:
            L.cndp_gpu_mq_flush(q)
            L.cndp_gpu_mq_wait(q)
            got += L.cndp_gpu_mq_poll(q, out + 8 * got, ed + 2 * got, n - got)
        return self.edges

    def idle_calls(self):
        """Two foreign calls a burst with nothing to do (the loop's own cost)."""
        L, q = self.L, self.q
        for _ in range(0, self.n, BURST):
            L.cndp_gpu_mq_pending(q)
            L.cndp_gpu_mq_pending(q)


def timed(fn, warmup, reps, passes=1):
    """Seconds of each of `reps` windows of `passes` calls, after `warmup` untimed windows."""
    t = []
    for w in range(warmup + reps):
        t0 = time.perf_counter()
        for _ in range(passes):
            fn()
        if w >= warmup:
            t.append(time.perf_counter() - t0)
    return t


def summary(t, n):
    r = sorted(n / x / 1e6 for x in t)
    return {"mpps_median": float(np.median(r)), "mpps_min": r[0], "mpps_max": r[-1], "seconds": t}


def dry(n):
    """The set-up on the CPU: the twins' verdict mix, and -- where tests/ is
    there -- the twins against the numpy restatements."""
    pool, fib, acl = build_pool(n), build_fib(), AclTable()
    acl.add_init_rules()
    acl.build()
    for name, _ in MODES:
        before = pool.mem.copy()
        tw = Twin(name, pool, fib, acl)
        tw.run()
        e = tw.edges()
        print(name, {hex(int(k)): int(v) for k, v in zip(*np.unique(e, return_counts=True))},
              "bytes changed:", int((pool.mem != before).sum()))
        pool.mem[:] = before
    print("dry OK")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--passes", type=int, default=64, help="passes over the pool per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cndpfwd_mq_bench.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    if a.dry:
        return dry(min(a.pool, 4096))
    if a.reps < 5:
        ap.error("--reps: at least five")
    import torch
    if not torch.cuda.is_available():
        sys.exit("cndpfwd_mq_bench: no GPU (a measurement does not fall back; --dry checks the set-up)")
    from cndp_amd.classify import Classifier
    cl = Classifier(0)
    pool, fib, acl = build_pool(a.pool), build_fib(), AclTable()
    acl.add_init_rules()
    acl.build()
    res = {"box": torch.cuda.get_device_name(0), "hip": torch.version.hip, "cpu": _cpu_name(), "pool": a.pool, "burst": BURST,
           "batch": a.batch, "depth": a.depth, "warmup": a.warmup, "reps": a.reps, "passes": a.passes, "acl_rules": acl.count(), "cases": {}}
    pristine = pool.mem.copy()
    for name, mode in MODES:
        # the twin first, on the pristine pool; its edges check every queue form below
        tw = Twin(name, pool, fib, acl)
        tw.run()
        want_edges, want_mem = tw.edges().copy(), pool.mem.copy()
        res["cases"][f"{name}/cpu_twin"] = summary(timed(tw.run, a.warmup, a.reps, a.passes), a.pool * a.passes)
        for form in ("zero_copy", "staged"):
            pool.mem[:] = pristine
            zc = form == "zero_copy"
            if zc:
                cl.host_register(pool.mem)
            try:
                q = MbufQueue(cl, mode, batch=a.batch, depth=a.depth, umem=pool.base if zc else None, lport=IN_LPORT,
                              lports=LPORTS, fib=fib, acl=acl, acl_mode=N.CNDP_ACL_STRICT, acl_flags=N.CNDP_ACL_F_MAC_SWAP)
                lp = Loop(q, pool)
                e = lp.run()
                if not np.array_equal(e, want_edges) or not np.array_equal(pool.mem, want_mem):
                    sys.exit(f"cndpfwd_mq_bench: {name}/{form} differs from the host twin")
                c = summary(timed(lp.run, a.warmup, a.reps, a.passes), a.pool * a.passes)
                c["calls_us_per_burst"] = (float(np.median(timed(lp.idle_calls, 1, a.reps, a.passes)))
                                           / (a.passes * a.pool / BURST) * 1e6)
                c["batches"] = q.stat(N.CNDP_MQ_STAT_BATCHES)
                res["cases"][f"{name}/{form}"] = c
                q.close()
            finally:
                if zc:
                    cl.host_unregister(pool.mem)
        pool.mem[:] = pristine
    for k, v in res["cases"].items():
        print(f"{k:18s} {v['mpps_median']:8.2f} Mpps  ({v['mpps_min']:.2f} .. {v['mpps_max']:.2f})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out, "box": res["box"]}))


def _cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


if __name__ == "__main__":
    main()

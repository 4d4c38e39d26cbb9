#!/usr/bin/env python3
"""Measure cnet's ip4_forward node over the mbuf queue
(cndp_gpu_mq_create_ip4_forward, include/cndp_mqcnet.h) against the host twin
(cndp_fwd_node_host) on one core.

    python tools/ip4_forward_mq_bench.py [--pool 65536] [--reps 7] [--out profiles/ip4_forward_mq_bench.json]

The frames are those ip4_forward_bench.py's stage takes: of bench.py's C4 batch
(pktgen.imix) the untagged IPv4 frames on the /24 routes, which leave ip4_input
on its forward edge.  The first --pool of them go into a pool of 2 KiB mbufs as
ip4_input hands them on: the frame at data_off 192, mtod at its IPv4 header
(data_off 206), l2_len 14.  The three forwarding tables are that tool's too:
direct (one lookup), gateway (three dependent lookups) and miss (two).

One lcore, as a cnet-graph node: the pool is handed to the queue in 256-mbuf
bursts -- submit, then poll, draining whatever has finished -- and a pass ends
when every mbuf is back.  Both forms: zero-copy (the pool registered, the kernel
reads and edits the frames over PCIe) and staged (the host copies header bytes
8-19 into pinned staging and the changed bytes back).  The CPU figure is
cndp_fwd_node_host on the same thread over the same pool, one call per burst.

The node moves data_off back by l2_len, so before every pass data_off and
data_len are put back (outside the clock); the TTL and checksum bytes just keep
stepping, the arithmetic does not depend on their values.  Method: per case
--warmup untimed windows, then --reps timed ones of --passes passes each; the
median and the min-max of the windows' rates are reported and every window's
seconds are kept in the JSON.  The loop is driven from Python through ctypes;
what two foreign calls a burst cost with nothing to do is measured the same way
(calls_us_per_burst).  --dry builds a small pool and runs the twin over the
three tables on the CPU without timing anything; without a GPU nothing else
runs.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cndp_amd import native as N                                   # noqa: E402
from cndp_amd import pktgen                                        # noqa: E402
from cndp_amd.mbuf import FRAME, MbufPool, MbufQueue               # noqa: E402
from ip4_forward_bench import cnet_fibs, table                     # noqa: E402

BURST = 256
L2 = 14


def build_pool(n, routes, v6):
    """The first n forwarded frames of a C4 batch large enough to hold them."""
    want24 = np.array(sorted({ip >> 8 for ip, d, _ in routes if d == 24}), np.int64)
    seed_n = max(4 * n, 4096)
    fr = pktgen.imix(seed_n, v4routes=routes, v6routes=v6, device="cpu")
    slab, offs = fr.slab.numpy(), fr.offsets.numpy().astype(np.int64)
    plain4 = (slab[offs + 12] == 8) & (slab[offs + 13] == 0)
    dst24 = (slab[offs + 30].astype(np.int64) << 16) | (slab[offs + 31].astype(np.int64) << 8) | slab[offs + 32]
    take = np.nonzero(plain4 & np.isin(dst24, want24))[0]
    if len(take) < n:
        sys.exit(f"ip4_forward_mq_bench: the C4 batch of {seed_n} has {len(take)} forwarded frames, {n} wanted")
    pool = MbufPool(n)
    pool.mem.reshape(n, FRAME)[:, 256:256 + 64] = np.stack([slab[offs[i]:offs[i] + 64] for i in take[:n]])
    pool.hdr["tx_offload"] = L2 | 20 << 7
    reset(pool)
    return pool


def reset(pool):
    """The header fields the node moves, as ip4_input leaves them."""
    pool.hdr["data_off"] = 192 + L2
    pool.hdr["data_len"] = 64 - L2


class Twin:
    """cndp_fwd_node_host over the pool, one call per 256-mbuf burst."""

    def __init__(self, tbl, pool):
        self.L, self.t, self.n = N.lib(), tbl.h, pool.n
        self.ptrs = pool.ptrs(np.arange(pool.n))
        self.base = ctypes.addressof(self.ptrs)
        self.edges = np.zeros(pool.n, np.uint16)

    def run(self):
        L, t, ed = self.L, self.t, self.edges.ctypes.data
        for b in range(0, self.n, BURST):
            rc = L.cndp_fwd_node_host(t, self.base + 8 * b, min(BURST, self.n - b), ed + 2 * b, None)
            if rc:
                raise OSError(-rc, "cndp_fwd_node_host")
        return self.edges


class Loop:
    """A node's loop over the pool through one queue, its buffers made once."""

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


def timed(fn, warmup, reps, passes, before=None):
    """Seconds of each of `reps` windows of `passes` calls (`before` runs in
    front of every call, outside the clock), after `warmup` untimed windows."""
    t = []
    for w in range(warmup + reps):
        s = 0.0
        for _ in range(passes):
            if before:
                before()
            t0 = time.perf_counter()
            fn()
            s += time.perf_counter() - t0
        if w >= warmup:
            t.append(s)
    return t


def summary(t, n):
    r = sorted(n / x / 1e6 for x in t)
    return {"mpps_median": float(np.median(r)), "mpps_min": r[0], "mpps_max": r[-1], "seconds": t}


def mix(e):
    e = np.asarray(e)
    return {"direct": int(((e & N.CNDP_MQ_EDGE_FWD_GATEWAY) == 0).sum() - (e == 1).sum()),
            "gateway": int(((e & N.CNDP_MQ_EDGE_FWD_GATEWAY) != 0).sum()), "arp_request": int((e == 1).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--passes", type=int, default=64, help="passes over the pool per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip4_forward_mq_bench.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    fib, fib6, routes, v6 = cnet_fibs()
    if a.dry:
        pool = build_pool(min(a.pool, 4096), routes, v6)
        for kind in ("direct", "gateway", "miss"):
            arp, rt4, tbl = table(kind, routes)
            before = pool.mem.copy()
            e = Twin(tbl, pool).run()
            print(kind, mix(e), "bytes changed:", int((pool.mem != before).sum()))
            pool.mem[:] = before
            tbl.close()
        print("dry OK")
        return
    if a.reps < 5:
        ap.error("--reps: at least five")
    import torch
    if not torch.cuda.is_available():
        sys.exit("ip4_forward_mq_bench: no GPU (a measurement does not fall back; --dry checks the set-up)")
    from cndp_amd.classify import Classifier
    cl = Classifier(0)
    pool = build_pool(a.pool, routes, v6)
    res = {"box": torch.cuda.get_device_name(0), "hip": torch.version.hip, "cpu": _cpu_name(), "pool": a.pool, "burst": BURST,
           "batch": a.batch, "depth": a.depth, "warmup": a.warmup, "reps": a.reps, "passes": a.passes, "cases": {}}
    pristine = pool.mem.copy()
    rs = lambda: reset(pool)                                        # noqa: E731
    for kind in ("direct", "gateway", "miss"):
        arp, rt4, tbl = table(kind, routes)
        tw = Twin(tbl, pool)
        want_edges = tw.run().copy()
        want_mem = pool.mem.copy()
        res["cases"][f"{kind}/cpu_twin"] = dict(summary(timed(tw.run, a.warmup, a.reps, a.passes, rs), a.pool * a.passes),
                                                mix=mix(want_edges))
        for form in ("zero_copy", "staged"):
            pool.mem[:] = pristine
            zc = form == "zero_copy"
            if zc:
                cl.host_register(pool.mem)
            try:
                q = MbufQueue(cl, N.CNDP_MQ_IP4_FORWARD, batch=a.batch, depth=a.depth, umem=pool.base if zc else None,
                              fwd_tbl=tbl)
                lp = Loop(q, pool)
                e = lp.run()
                if not np.array_equal(e, want_edges) or not np.array_equal(pool.mem, want_mem):
                    sys.exit(f"ip4_forward_mq_bench: {kind}/{form} differs from the host twin")
                c = summary(timed(lp.run, a.warmup, a.reps, a.passes, rs), a.pool * a.passes)
                c["calls_us_per_burst"] = (float(np.median(timed(lp.idle_calls, 1, a.reps, a.passes)))
                                           / (a.passes * a.pool / BURST) * 1e6)
                c["batches"] = q.stat(N.CNDP_MQ_STAT_BATCHES)
                res["cases"][f"{kind}/{form}"] = c
                q.close()
            finally:
                if zc:
                    cl.host_unregister(pool.mem)
        pool.mem[:] = pristine
        tbl.close()
        arp.close()
        rt4.close()
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

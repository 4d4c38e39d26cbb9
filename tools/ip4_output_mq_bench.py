#!/usr/bin/env python3
"""Measure cnet's udp_output + ip4_output nodes over the mbuf queue
(cndp_gpu_mq_create_ip4_output, include/cndp_mqtx.h) against the host twin
(cndp_ip4_output_node_host) on one core.

    python tools/ip4_output_mq_bench.py [--pool 16384] [--reps 7] [--out profiles/ip4_output_mq_bench.json]

Four cases: a pool of 2 KiB mbufs as the application hands them to udp_output
(mtod at the payload, data_off 234, the PCB index in userptr, the metadata as
udp_input left it), 64 sockets on four netifs, every peer with an ARP entry, so
every mbuf leaves on its netif's edge:

    udp18 / udp18_cksum        18-byte payloads (a 60-byte frame), without / with CNDP_UDP_CHKSUM_FLAG
    udp1472 / udp1472_cksum    1472-byte payloads (a 1514-byte frame)

One lcore, as a cnet-graph node: the pool is handed over in 256-mbuf bursts --
submit, then poll, draining whatever has finished -- and a pass ends when every
mbuf is back.  Three runners per case: the queue zero-copy (the pool registered,
the kernels write the headers in place and read the payloads over PCIe), the
queue staged (the host copies each payload into pinned staging and the written
header bytes back) and the twin on the same thread, one call per burst.
Zero-copy and staged each have a pool of their own with the same contents; the
twin runs over the staged one.

The nodes move data_off back, so before every pass data_off, data_len and
tx_offload are put back (outside the clock).  Method: per case --warmup untimed
windows, then --reps timed ones of --passes passes each (a quarter as many for
the 1472-byte cases), the runners taking turns window by window (interleaved);
the median and the min-max of the windows' rates are reported and every window's
seconds are kept in the JSON.  The loop is driven from Python through ctypes.
--dry builds small pools and runs the twin over the four cases on the CPU
without timing anything; without a GPU nothing else runs.
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cndp_amd import native as N                                   # noqa: E402
from cndp_amd.fib import Fib                                       # noqa: E402
from cndp_amd.fwd import FwdTable                                  # noqa: E402
from cndp_amd.l4 import PcbTable                                   # noqa: E402
from cndp_amd.mbuf import FRAME, MbufPool, MbufQueue               # noqa: E402
from cndp_amd.tx import ident_set                                  # noqa: E402

BURST = 256
DOFF = 192 + 42
SOCKS, NETIFS = 64, 4
CASES = {"udp18": (18, False), "udp18_cksum": (18, True), "udp1472": (1472, False), "udp1472_cksum": (1472, True)}
TXO0 = 14 | 20 << 7 | 8 << 16


def make_tables(cksum):
    """64 sockets 10.(4 + k % 4).0.7:5000 + k, a route per /16 onto netif k % 4, 256 peers with ARP entries."""
    mk = lambda nm: Fib(nm, N.CNE_FIB_DIR24_8, default_nh=300, max_routes=512, nh_sz=N.CNE_FIB_DIR24_8_4B,  # noqa: E731
                        num_tbl8=16)
    arp, rt4 = mk("arp-fib"), mk("rt4-fib")
    fwd = FwdTable(arp, rt4, 272, 16)
    for k in range(NETIFS):
        assert fwd.netif_set(k, f"02:00:00:00:00:1{k}") == 0
        assert fwd.rt_set(1 + k, 0, k) == 0 and rt4.add(0x0A040000 + (k << 16), 16, 1 + k) == 0
    for k in range(256):
        assert fwd.arp_set(1 + k, k % NETIFS, f"02:aa:00:00:00:{k:02x}") == 0 and arp.add(0xC6120000 + k, 32, 1 + k) == 0
    pcb = PcbTable(SOCKS)
    for k in range(SOCKS):
        pcb.add(laddr=f"10.{4 + k % NETIFS}.0.7", lport=5000 + k, cksum=cksum)
    return arp, rt4, fwd, pcb


def build_pool(n, ln, seed=3):
    pool = MbufPool(n)
    rng = np.random.default_rng(seed)
    rows = pool.mem.reshape(n, FRAME)
    kinds = rng.integers(0, 256, (64, ln), dtype=np.uint8)
    rows[:, 64 + DOFF:64 + DOFF + ln] = kinds[rng.integers(0, 64, n)]
    i = np.arange(n)
    k = i % SOCKS
    md = np.zeros((n, 40), np.uint8)
    md[:, 0], md[:, 1], md[:, 20], md[:, 21] = 2, 4, 2, 4
    fport = 40000 + i % 20000
    md[:, 2], md[:, 3] = fport >> 8, fport & 0xFF
    md[:, 4:8] = np.stack([np.full(n, 198), np.full(n, 18), np.zeros(n), i % 256], 1)
    md[:, 22], md[:, 23] = (5000 + k) >> 8, (5000 + k) & 0xFF
    md[:, 24:28] = np.stack([np.full(n, 10), 4 + k % NETIFS, np.zeros(n), np.full(n, 7)], 1)
    rows[:, 64:104] = md
    pool.hdr["udata64"] = k
    pool.ln = ln
    reset(pool)
    return pool


def reset(pool):
    """The header fields the nodes move, as the application hands the mbuf over."""
    pool.hdr["data_off"] = DOFF
    pool.hdr["data_len"] = pool.ln
    pool.hdr["tx_offload"] = TXO0


class Twin:
    """cndp_ip4_output_node_host over the pool, one call per 256-mbuf burst."""

    def __init__(self, fwd, pcb, pool):
        self.L, self.f, self.p, self.n = N.lib(), fwd.h, pcb.h, pool.n
        self.ptrs = pool.ptrs(np.arange(pool.n))
        self.base = ctypes.addressof(self.ptrs)
        self.edges = np.zeros(pool.n, np.uint16)

    def run(self):
        L, ed = self.L, self.edges.ctypes.data
        for b in range(0, self.n, BURST):
            rc = L.cndp_ip4_output_node_host(self.f, self.p, N.CNDP_TX_UDP, self.base + 8 * b, min(BURST, self.n - b),
                                             ed + 2 * b, None, 2048, None)
            if rc:
                raise OSError(-rc, "cndp_ip4_output_node_host")
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


def timed_interleaved(runners, warmup, reps, passes):
    """runners: name -> (fn, before).  Windows of `passes` calls each, the runners
    taking turns window by window; `before` runs in front of every call, outside
    the clock.  Returns name -> seconds of each timed window."""
    t = {k: [] for k in runners}
    for w in range(warmup + reps):
        for name, (fn, before) in runners.items():
            s = 0.0
            for _ in range(passes):
                before()
                t0 = time.perf_counter()
                fn()
                s += time.perf_counter() - t0
            if w >= warmup:
                t[name].append(s)
    return t


def summary(t, n):
    r = sorted(n / x / 1e6 for x in t)
    return {"mpps_median": float(np.median(r)), "mpps_min": r[0], "mpps_max": r[-1], "seconds": t}


def close_tables(arp, rt4, fwd, pcb):
    pcb.close()
    fwd.close()
    arp.close()
    rt4.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--passes", type=int, default=64,
                    help="passes over the pool per timed window (a quarter of it for the 1472-byte cases)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip4_output_mq_bench.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    if a.dry:
        for case, (ln, ck) in CASES.items():
            tabs, pool = make_tables(ck), build_pool(min(a.pool, 1024), ln)
            e = Twin(tabs[2], tabs[3], pool).run()
            assert ((e & N.CNDP_MQ_EDGE_TX_MASK) >= 2).all() and (((e & N.CNDP_MQ_EDGE_TX_CKSUM) != 0) == ck).all(), case
            assert (pool.hdr["data_off"] == 192).all() and (pool.hdr["data_len"] == ln + 42).all()
            print(case, "sent:", len(e), "frame bytes:", int(pool.hdr["data_len"][0]))
            close_tables(*tabs)
        print("dry OK")
        return
    if a.reps < 5:
        ap.error("--reps: at least five")
    import torch
    if not torch.cuda.is_available():
        sys.exit("ip4_output_mq_bench: no GPU (a measurement does not fall back; --dry checks the set-up)")
    from cndp_amd.classify import Classifier
    cl = Classifier(0)
    res = {"box": torch.cuda.get_device_name(0), "hip": torch.version.hip, "cpu": _cpu_name(), "pool": a.pool, "burst": BURST,
           "batch": a.batch, "depth": a.depth, "warmup": a.warmup, "reps": a.reps, "passes": a.passes,
           "interleaved": True, "cases": {}}
    for case, (ln, ck) in CASES.items():
        arp, rt4, fwd, pcb = make_tables(ck)
        passes = a.passes if ln < 1000 else max(1, a.passes // 4)
        pz, ps = build_pool(a.pool, ln), build_pool(a.pool, ln)
        tw = Twin(fwd, pcb, ps)
        want_edges = tw.run().copy()
        if not ((want_edges & N.CNDP_MQ_EDGE_TX_MASK) >= 2).all():
            sys.exit(f"ip4_output_mq_bench: {case}: the twin does not send every mbuf")
        want_mem = ps.mem.copy()
        ps.mem.reshape(a.pool, FRAME)[:, 64 + 192:64 + DOFF] = pz.mem.reshape(a.pool, FRAME)[:, 64 + 192:64 + DOFF]
        reset(ps)
        cl.host_register(pz.mem)
        try:
            qz = MbufQueue(cl, N.CNDP_MQ_IP4_OUTPUT, batch=a.batch, depth=a.depth, umem=pz.base, fwd_tbl=fwd, pcb_tbl=pcb)
            qs = MbufQueue(cl, N.CNDP_MQ_IP4_OUTPUT, batch=a.batch, depth=a.depth, fwd_tbl=fwd, pcb_tbl=pcb)
            lz, ls = Loop(qz, pz), Loop(qs, ps)
            for lp, pool, form in ((lz, pz, "zero_copy"), (ls, ps, "staged")):
                for k in range(NETIFS):
                    ident_set(fwd, k, 0)
                e = lp.run()
                same = np.array_equal(pool.mem.reshape(a.pool, FRAME)[:, 24:], want_mem.reshape(a.pool, FRAME)[:, 24:])
                if not np.array_equal(e, want_edges) or not same:
                    sys.exit(f"ip4_output_mq_bench: {case}/{form} differs from the host twin")
                reset(pool)
            t = timed_interleaved({"cpu_twin": (tw.run, lambda: reset(ps)), "zero_copy": (lz.run, lambda: reset(pz)),
                                   "staged": (ls.run, lambda: reset(ps))}, a.warmup, a.reps, passes)
            for name, secs in t.items():
                c = summary(secs, a.pool * passes)
                c["passes"] = passes
                if name != "cpu_twin":
                    c["batches_all_windows"] = (qz if name == "zero_copy" else qs).stat(N.CNDP_MQ_STAT_BATCHES)
                res["cases"][f"{case}/{name}"] = c
            qz.close()
            qs.close()
        finally:
            cl.host_unregister(pz.mem)
        close_tables(arp, rt4, fwd, pcb)
    for k, v in res["cases"].items():
        print(f"{k:28s} {v['mpps_median']:8.2f} Mpps  ({v['mpps_min']:.2f} .. {v['mpps_max']:.2f})")
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

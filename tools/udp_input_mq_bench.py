#!/usr/bin/env python3
"""Measure cnet's ip4_proto + udp_input nodes over the mbuf queue
(cndp_gpu_mq_create_udp_input, include/cndp_mql4.h) against the host twin
(cndp_udp_input_node_host) on one core.

    python tools/udp_input_mq_bench.py [--pool 16384] [--reps 7] [--out profiles/udp_input_mq_bench.json]

Three cases, each over a table of 16 sockets (16 local ports, every fourth one
connected to a peer as well) and a pool of 2 KiB mbufs as ip4_input hands them
to its proto edge (mtod at the IPv4 header, data_off 206, l3_len 20, l4_len 8):

    nocksum_64    sockets without UDP_CHKSUM_FLAG, 64-byte frames (a 30-byte datagram)
    cksum_64      the same sockets with the flag: every datagram is verified
    cksum_1472    with the flag, 1472-byte datagrams

Every datagram carries a good checksum and finds its socket, so every mbuf goes
to chnl_recv.  One lcore, as a cnet-graph node: the pool is handed over in
256-mbuf bursts -- submit, then poll, draining whatever has finished -- and a
pass ends when every mbuf is back.  Three runners per case: the queue zero-copy
(the pool registered, the kernel reads the frames over PCIe), the queue staged
(the host copies each frame's readable bytes into pinned staging) and the twin
on the same thread, one call per burst.  Zero-copy and staged each have a pool
of their own with the same contents; the twin runs over the staged one.  Both
queue forms are run a second time with CNDP_TUNE_MQ_PCB_LDS on (the kernel
copies the table image into LDS per block instead of reading it in device
memory): the figures behind the choice of the default.

The node moves data_off forward, so before every pass data_off and data_len are
put back (outside the clock).  Method: per case --warmup untimed windows, then
--reps timed ones of --passes passes each (a quarter as many for the 1472-byte
case, whose passes are long), the runners taking turns
window by window (interleaved); the median and the min-max of the windows'
rates are reported and every window's seconds are kept in the JSON.  The loop is
driven from Python through ctypes.  --dry builds small pools and runs the twin
over the three cases on the CPU without timing anything; without a GPU nothing
else runs.
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
from cndp_amd.l4 import PcbTable                                   # noqa: E402
from cndp_amd.mbuf import FRAME, MbufPool, MbufQueue               # noqa: E402

BURST = 256
DOFF = 192 + 14
CASES = {"nocksum_64": (False, 30), "cksum_64": (True, 30), "cksum_1472": (True, 1472)}
RECV = 0x0401
LADDR, PEER = bytes([10, 4, 0, 7]), bytes([198, 18, 0, 1])


def make_table(cksum):
    t = PcbTable(64)
    for k in range(16):
        t.add(laddr="10.4.0.7", lport=5000 + k, cksum=cksum)
        if k % 4 == 0:
            t.add(laddr="10.4.0.7", lport=5000 + k, faddr="198.18.0.1", fport=40000, cksum=cksum)
    return t


def build_pool(n, dgram, seed=3):
    """n mbufs: datagrams of `dgram` bytes to the 16 ports from two source ports,
    good checksums.  A handful of distinct payloads, repeated."""
    pool = MbufPool(n)
    rng = np.random.default_rng(seed)
    rows = pool.mem.reshape(n, FRAME)
    kinds = []
    for k in range(64):
        ip = bytes([0x45, 0]) + struct.pack(">H", 20 + dgram) + bytes([0, 0, 0, 0, 64, 17, 0, 0]) + PEER + LADDR
        d = bytearray(struct.pack(">HHHH", 40000 + k // 16 % 2, 5000 + k % 16, dgram, 0) +
                      rng.integers(0, 256, dgram - 8, dtype=np.uint8).tobytes())
        w = np.frombuffer(PEER + LADDR + bytes([0, 17]) + struct.pack(">H", dgram) + bytes(d) + b"\0" * (dgram & 1), ">u2")
        c = int(w.sum(dtype=np.uint64))
        c = (c & 0xFFFF) + (c >> 16)
        c = ~((c & 0xFFFF) + (c >> 16)) & 0xFFFF
        d[6:8] = struct.pack(">H", c or 0xFFFF)
        kinds.append(np.frombuffer(ip + bytes(d), np.uint8))
    pick = rng.integers(0, 64, n)
    for k in range(64):
        rows[pick == k, 64 + DOFF:64 + DOFF + 20 + dgram] = kinds[k]
    pool.hdr["tx_offload"] = 14 | 20 << 7 | 8 << 16
    pool.tot = 20 + dgram
    reset(pool)
    return pool


def reset(pool):
    """The header fields the node moves, as ip4_input leaves them."""
    pool.hdr["data_off"] = DOFF
    pool.hdr["data_len"] = pool.tot


class Twin:
    """cndp_udp_input_node_host over the pool, one call per 256-mbuf burst."""

    def __init__(self, tbl, pool):
        self.L, self.t, self.n = N.lib(), tbl.h, pool.n
        self.ptrs = pool.ptrs(np.arange(pool.n))
        self.base = ctypes.addressof(self.ptrs)
        self.edges = np.zeros(pool.n, np.uint16)

    def run(self):
        L, t, ed = self.L, self.t, self.edges.ctypes.data
        for b in range(0, self.n, BURST):
            rc = L.cndp_udp_input_node_host(t, self.base + 8 * b, min(BURST, self.n - b), ed + 2 * b, None, 2048, None)
            if rc:
                raise OSError(-rc, "cndp_udp_input_node_host")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--passes", type=int, default=512,
                    help="passes over the pool per timed window (a quarter of it for the 1472-byte case)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "udp_input_mq_bench.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    if a.dry:
        for case, (ck, dgram) in CASES.items():
            tbl, pool = make_table(ck), build_pool(min(a.pool, 1024), dgram)
            e = Twin(tbl, pool).run()
            assert (e == RECV).all(), case
            print(case, "chnl_recv:", int((e == RECV).sum()), "data_off:", int(pool.hdr["data_off"][0]))
            tbl.close()
        print("dry OK")
        return
    if a.reps < 5:
        ap.error("--reps: at least five")
    import torch
    if not torch.cuda.is_available():
        sys.exit("udp_input_mq_bench: no GPU (a measurement does not fall back; --dry checks the set-up)")
    from cndp_amd.classify import Classifier
    cl = Classifier(0)
    res = {"box": torch.cuda.get_device_name(0), "hip": torch.version.hip, "cpu": _cpu_name(), "pool": a.pool, "burst": BURST,
           "batch": a.batch, "depth": a.depth, "warmup": a.warmup, "reps": a.reps, "passes": a.passes,
           "interleaved": True, "cases": {}}
    for case, (ck, dgram) in CASES.items():
        tbl = make_table(ck)
        passes = a.passes if dgram < 1000 else max(1, a.passes // 4)
        pz, ps = build_pool(a.pool, dgram), build_pool(a.pool, dgram)
        tw = Twin(tbl, ps)
        want_edges = tw.run().copy()
        if not (want_edges == RECV).all():
            sys.exit(f"udp_input_mq_bench: {case}: the twin does not send every mbuf to chnl_recv")
        want_mem = ps.mem.copy()
        reset(ps)
        cl.host_register(pz.mem)
        try:
            qz = MbufQueue(cl, N.CNDP_MQ_UDP_INPUT, batch=a.batch, depth=a.depth, umem=pz.base, pcb_tbl=tbl)
            qs = MbufQueue(cl, N.CNDP_MQ_UDP_INPUT, batch=a.batch, depth=a.depth, pcb_tbl=tbl)
            lz, ls = Loop(qz, pz), Loop(qs, ps)
            for lp, pool, form in ((lz, pz, "zero_copy"), (ls, ps, "staged")):
                e = lp.run()
                same = np.array_equal(pool.mem.reshape(a.pool, FRAME)[:, 24:], want_mem.reshape(a.pool, FRAME)[:, 24:])
                if not np.array_equal(e, want_edges) or not same:       # all but pooldata / buf_addr / hash
                    sys.exit(f"udp_input_mq_bench: {case}/{form} differs from the host twin")
            def with_lds(on, pool):
                def before():
                    cl.set_tuning(mq_pcb_lds=on)
                    reset(pool)
                return before

            t = timed_interleaved({"cpu_twin": (tw.run, lambda: reset(ps)), "zero_copy": (lz.run, with_lds(0, pz)),
                                   "staged": (ls.run, with_lds(0, ps)), "zero_copy_lds": (lz.run, with_lds(1, pz)),
                                   "staged_lds": (ls.run, with_lds(1, ps))}, a.warmup, a.reps, passes)
            cl.set_tuning(mq_pcb_lds=0)
            for name, secs in t.items():
                c = summary(secs, a.pool * passes)
                c["passes"] = passes
                if name != "cpu_twin":
                    c["batches_all_windows"] = (qz if name.startswith("zero_copy") else qs).stat(N.CNDP_MQ_STAT_BATCHES)
                res["cases"][f"{case}/{name}"] = c
            qz.close()
            qs.close()
        finally:
            cl.host_unregister(pz.mem)
        tbl.close()
    for k, v in res["cases"].items():
        print(f"{k:24s} {v['mpps_median']:8.2f} Mpps  ({v['mpps_min']:.2f} .. {v['mpps_max']:.2f})")
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

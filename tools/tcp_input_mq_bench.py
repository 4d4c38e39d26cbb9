#!/usr/bin/env python3
"""Measure cnet's tcp_input node over the mbuf queue
(cndp_gpu_mq_create_tcp_input, include/cndp_mqtcp.h) against the host twin
(cndp_tcp_input_node_host) on one core.

    python tools/tcp_input_mq_bench.py [--pool 16384] [--reps 7] [--out profiles/tcp_input_mq_bench.json]

Four cases: a TCP table of 16 or of 4096 established connections behind one
listener, and a pool of 2 KiB mbufs as ip4_proto hands them to its tcp_input
edge (mtod at the IPv4 header, data_off 206, l3_len 20, l4_len 20) holding

    conn16_64 / conn4096_64        64-byte frames (a 30-byte segment)
    conn16_1460 / conn4096_1460    1460-byte segments

Every segment carries a good checksum and finds its connection, so every mbuf
leaves on SEGMENT; in TCP every matched frame's checksum is verified.  One
lcore, as a cnet-graph node: the pool is handed over in 256-mbuf bursts --
submit, then poll_tcp, draining whatever has finished with its records -- and a
pass ends when every mbuf is back.  Three runners per case: the queue zero-copy
(the pool registered, the kernel reads the frames over PCIe), the queue staged
(the host copies each frame's readable bytes into pinned staging) and the twin
on the same thread, one call per burst.  Zero-copy and staged each have a pool
of their own with the same contents; the twin runs over the staged one.

The node moves data_off forward, so before every pass data_off and data_len are
put back (outside the clock).  Method: per case --warmup untimed windows, then
--reps timed ones of --passes passes each (a quarter as many for the 1460-byte
cases, whose passes are long), the runners taking turns window by window
(interleaved); the median and the min-max of the windows' rates are reported and
every window's seconds are kept in the JSON.  The loop is driven from Python
through ctypes.  --dry builds small pools and runs the twin over the four cases
on the CPU without timing anything; without a GPU nothing else runs.
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
from cndp_amd.l4 import SEG_DT, PcbTable                           # noqa: E402
from cndp_amd.mbuf import FRAME, MbufPool, MbufQueue               # noqa: E402

BURST = 256
DOFF = 192 + 14
CASES = {"conn16_64": (16, 30), "conn4096_64": (4095, 30), "conn16_1460": (16, 1460), "conn4096_1460": (4095, 1460)}
SEG = 0x0501
LADDR, PEER = bytes([10, 4, 0, 7]), bytes([198, 18, 0, 1])


def make_table(conns):
    """One listener on port 5000 and `conns` connections behind it (4095: a full table)."""
    t = PcbTable(conns + 1)
    t.add(lport=5000)
    for k in range(conns):
        t.add(laddr="10.4.0.7", lport=5000, faddr="198.18.0.1", fport=10000 + k)
    return t


def build_pool(n, conns, seg, seed=3):
    """n mbufs: segments of `seg` bytes on the table's connections in turn, good
    checksums.  64 distinct payloads, repeated; the ports and the checksum are
    set per mbuf (the sum moves with the port by incremental update)."""
    pool = MbufPool(n)
    rng = np.random.default_rng(seed)
    rows = pool.mem.reshape(n, FRAME)
    ip = bytes([0x45, 0]) + struct.pack(">H", 20 + seg) + bytes([0, 0, 0, 0, 64, 6, 0, 0]) + PEER + LADDR
    kinds, sums = [], []
    for k in range(64):
        d = bytearray(struct.pack(">HHIIBBHHH", 0, 5000, k * 1000, k * 7, 0x50, 0x18, 512, 0, 0) +
                      rng.integers(0, 256, seg - 20, dtype=np.uint8).tobytes())
        w = np.frombuffer(PEER + LADDR + bytes([0, 6]) + struct.pack(">H", seg) + bytes(d) + b"\0" * (seg & 1), ">u2")
        kinds.append(np.frombuffer(ip + bytes(d), np.uint8))
        sums.append(int(w.sum(dtype=np.uint64)))
    pick = rng.integers(0, 64, n)
    for k in range(64):
        rows[pick == k, 64 + DOFF:64 + DOFF + 20 + seg] = kinds[k]
    sport = 10000 + np.arange(n, dtype=np.int64) % conns
    c = np.array(sums, np.int64)[pick] + sport                      # the source port joins the sum
    c = (c & 0xFFFF) + (c >> 16)
    c = ~((c & 0xFFFF) + (c >> 16)) & 0xFFFF
    o = 64 + DOFF + 20
    rows[:, o], rows[:, o + 1] = sport >> 8, sport & 0xFF
    rows[:, o + 16], rows[:, o + 17] = c >> 8, c & 0xFF
    pool.hdr["tx_offload"] = 14 | 20 << 7 | 20 << 16
    pool.tot = 20 + seg
    reset(pool)
    return pool


def reset(pool):
    """The header fields the node moves, as ip4_proto hands them on."""
    pool.hdr["data_off"] = DOFF
    pool.hdr["data_len"] = pool.tot


class Twin:
    """cndp_tcp_input_node_host over the pool, one call per 256-mbuf burst."""

    def __init__(self, tbl, pool):
        self.L, self.t, self.n = N.lib(), tbl.h, pool.n
        self.ptrs = pool.ptrs(np.arange(pool.n))
        self.base = ctypes.addressof(self.ptrs)
        self.edges = np.zeros(pool.n, np.uint16)
        self.segs = np.zeros(pool.n, SEG_DT)

    def run(self):
        L, t, ed, sg = self.L, self.t, self.edges.ctypes.data, self.segs.ctypes.data
        for b in range(0, self.n, BURST):
            rc = L.cndp_tcp_input_node_host(t, self.base + 8 * b, min(BURST, self.n - b), ed + 2 * b, sg + 16 * b, None,
                                            2048, None)
            if rc:
                raise OSError(-rc, "cndp_tcp_input_node_host")
        return self.edges


class Loop:
    """A node's loop over the pool through one queue, its buffers made once."""

    def __init__(self, q, pool):
        self.L, self.q, self.n = N.lib(), q.h, pool.n
        self.ptrs = pool.ptrs(np.arange(pool.n))
        self.base = ctypes.addressof(self.ptrs)
        self.out = (ctypes.c_void_p * pool.n)()
        self.edges = np.zeros(pool.n, np.uint16)
        self.segs = np.zeros(pool.n, SEG_DT)

    def run(self):
        """One pass; returns the edges in submission order."""
        L, q, n = self.L, self.q, self.n
        out, ed, sg = ctypes.addressof(self.out), self.edges.ctypes.data, self.segs.ctypes.data
        got = 0
        for b in range(0, n, BURST):
            want = min(BURST, n - b)
            done = 0
            while done < want:
                k = L.cndp_gpu_mq_submit(q, self.base + 8 * (b + done), want - done)
                if k < 0:
                    raise OSError(-k, "cndp_gpu_mq_submit")
                done += k
                g = L.cndp_gpu_mq_poll_tcp(q, out + 8 * got, ed + 2 * got, sg + 16 * got, n - got)
                got += g
                if k == 0 and g == 0:
                    L.cndp_gpu_mq_wait(q)
        while got < n:
            L.cndp_gpu_mq_flush(q)
            L.cndp_gpu_mq_wait(q)
            got += L.cndp_gpu_mq_poll_tcp(q, out + 8 * got, ed + 2 * got, sg + 16 * got, n - got)
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
    ap.add_argument("--passes", type=int, default=128,
                    help="passes over the pool per timed window (a quarter of it for the 1460-byte cases)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcp_input_mq_bench.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    if a.dry:
        for case, (conns, seg) in CASES.items():
            tbl, pool = make_table(conns), build_pool(min(a.pool, 1024), conns, seg)
            tw = Twin(tbl, pool)
            e = tw.run()
            assert (e == SEG).all() and (tw.segs["len"] == seg - 20).all(), case
            print(case, "segments:", int((e == SEG).sum()), "data_off:", int(pool.hdr["data_off"][0]))
            tbl.close()
        print("dry OK")
        return
    if a.reps < 5:
        ap.error("--reps: at least five")
    import torch
    if not torch.cuda.is_available():
        sys.exit("tcp_input_mq_bench: no GPU (a measurement does not fall back; --dry checks the set-up)")
    from cndp_amd.classify import Classifier
    cl = Classifier(0)
    res = {"box": torch.cuda.get_device_name(0), "hip": torch.version.hip, "cpu": _cpu_name(), "pool": a.pool, "burst": BURST,
           "batch": a.batch, "depth": a.depth, "warmup": a.warmup, "reps": a.reps, "passes": a.passes,
           "interleaved": True, "cases": {}}
    for case, (conns, seg) in CASES.items():
        tbl = make_table(conns)
        passes = a.passes if seg < 1000 else max(1, a.passes // 4)
        pz, ps = build_pool(a.pool, conns, seg), build_pool(a.pool, conns, seg)
        tw = Twin(tbl, ps)
        want_edges = tw.run().copy()
        want_segs = tw.segs.copy()
        if not (want_edges == SEG).all():
            sys.exit(f"tcp_input_mq_bench: {case}: the twin does not send every mbuf on SEGMENT")
        want_mem = ps.mem.copy()
        reset(ps)
        cl.host_register(pz.mem)
        try:
            qz = MbufQueue(cl, N.CNDP_MQ_TCP_INPUT, batch=a.batch, depth=a.depth, umem=pz.base, pcb_tbl=tbl)
            qs = MbufQueue(cl, N.CNDP_MQ_TCP_INPUT, batch=a.batch, depth=a.depth, pcb_tbl=tbl)
            lz, ls = Loop(qz, pz), Loop(qs, ps)
            for lp, pool, form in ((lz, pz, "zero_copy"), (ls, ps, "staged")):
                e = lp.run()
                same = np.array_equal(pool.mem.reshape(a.pool, FRAME)[:, 24:], want_mem.reshape(a.pool, FRAME)[:, 24:])
                if not np.array_equal(e, want_edges) or not same or lp.segs.tobytes() != want_segs.tobytes():
                    sys.exit(f"tcp_input_mq_bench: {case}/{form} differs from the host twin")
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
        tbl.close()
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

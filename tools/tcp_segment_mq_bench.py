#!/usr/bin/env python3
"""Measure cnet's tcp_input + tcp_do_options + header-prediction triage over the
mbuf queue (cndp_gpu_mq_create_tcp_segment, include/cndp_mqtcb.h) on one core
against (a) the host twin (cndp_tcp_segment_node_host) and (b) what a binding
does without this mode: the queue's CNDP_MQ_TCP_INPUT mode, then
cndp_tcp_segment_host on the lcore over what poll_tcp returned.

    python tools/tcp_segment_mq_bench.py [--pool 16384] [--reps 7] [--out profiles/tcp_segment_mq_bench.json]

Cases: a TCP table of 64 or of 4096 established connections (4095 behind one
listener: a full table), each with a TCB, and a pool of 2 KiB mbufs as ip4_proto
hands them to its tcp_input edge (mtod at the IPv4 header, data_off 206, l3_len
20), every segment a pure or data-carrying ACK with the timestamp-only 32-byte
header (NOP NOP timestamp), a good checksum and a connection of its own turn:

    conn64_ts32 / conn4096_ts32      no payload: a 66-byte frame on the wire
    conn64_1460 / conn4096_1460      1460-byte segments

Each case runs twice: with no TCB touched ("still") and with every connection's
TCB rewritten by cndp_tcb_set in front of every batch ("churn"), which is what
a TCP host does.  The rewriting itself is outside the clock; what it costs the
launch (the snapshot and copy of the changed entries) is inside.  The seconds
spent inside cndp_gpu_mq_submit / _flush -- the fill and the launches -- are
reported per pass beside the rate: a launch that waited for the stream would
show there in the churn rows.

Runners: the queue zero-copy and staged in the new mode, the twin one call per
256-mbuf burst, and "mode9_host": the tcp_input mode zero-copy, then
cndp_tcp_segment_host per burst over the records it returned.  That last runner
is handed the PCB index of every mbuf ready-made (the pool's layout is fixed), so
the gather from m->userptr a binding would make is left out, in its favour.

Method: tools/tcp_input_mq_bench.py's -- untimed warm-up windows, then --reps
timed ones of --passes passes each (a quarter for the 1460-byte cases and for
churn), the runners taking turns window by window; median and min-max of the
windows' rates, every window's seconds kept.  The loop is driven from Python
through ctypes.  --dry builds small pools and runs the twin on the CPU without
timing anything; without a GPU nothing else runs."""
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
from cndp_amd.l4 import OPT_DT, SEG_DT, PcbTable, TcbTable         # noqa: E402
from cndp_amd.mbuf import FRAME, MbufPool, MbufQueue               # noqa: E402

BURST = 256
DOFF = 192 + 14
HDR = 32
CASES = {"conn64_ts32": (64, HDR), "conn4096_ts32": (4095, HDR), "conn64_1460": (64, 1460), "conn4096_1460": (4095, 1460)}
SEG = 0x0501
LADDR, PEER = bytes([10, 4, 0, 7]), bytes([198, 18, 0, 1])
NOW = 100000
PRED_ACK, PRED_DATA = N.CNDP_TCPSEG_PRED_ACK, N.CNDP_TCPSEG_PRED_DATA


def make_tables(conns):
    """One listener on port 5000 and `conns` connections behind it, each with an
    established TCB the pool's segments pass header prediction against."""
    t = PcbTable(conns + 1)
    t.add(lport=5000)
    for k in range(conns):
        t.add(laddr="10.4.0.7", lport=5000, faddr="198.18.0.1", fport=10000 + k)
    tc = TcbTable(t)
    tcb = (N.Tcb * (conns + 1))()
    for i in range(1, conns + 1):
        x = tcb[i]
        x.rcv_nxt, x.snd_una, x.snd_nxt, x.snd_max, x.snd_wnd, x.snd_cwnd = 1000, 500, 700, 700, 512, 4000
        x.ts_recent, x.last_ack_sent, x.rcv_space, x.max_mss = 90, 990, 4000, 1460
        x.state, x.flags = N.CNDP_TCPS_ESTABLISHED, N.CNDP_TCB_REASS_EMPTY
    churn(tc, tcb, conns)
    return t, tc, tcb


def churn(tc, tcb, conns):
    """cndp_tcb_set for every connection, as a host that has applied a batch."""
    L, h = N.lib(), tc.h
    for i in range(1, conns + 1):
        tcb[i].snd_cwnd += 1
        L.cndp_tcb_set(h, i, ctypes.byref(tcb[i]))


def build_pool(n, conns, seg, seed=3):
    """n mbufs: segments of `seg` bytes on the table's connections in turn, good
    checksums, 64 distinct payloads repeated."""
    pool = MbufPool(n)
    rng = np.random.default_rng(seed)
    rows = pool.mem.reshape(n, FRAME)
    ip = bytes([0x45, 0]) + struct.pack(">H", 20 + seg) + bytes([0, 0, 0, 0, 64, 6, 0, 0]) + PEER + LADDR
    data = seg > HDR
    kinds, sums = [], []
    for k in range(64):
        d = bytearray(struct.pack(">HHIIBBHHH", 0, 5000, 1000, 500 if data else 600, HDR // 4 << 4, 0x10, 512, 0, 0) +
                      bytes([1, 1, 8, 10]) + struct.pack(">II", 95, NOW - 5) +
                      rng.integers(0, 256, seg - HDR, dtype=np.uint8).tobytes())
        w = np.frombuffer(PEER + LADDR + bytes([0, 6]) + struct.pack(">H", seg) + bytes(d) + b"\0" * (seg & 1), ">u2")
        kinds.append(np.frombuffer(ip + bytes(d), np.uint8))
        sums.append(int(w.sum(dtype=np.uint64)))
    pick = rng.integers(0, 64, n)
    for k in range(64):
        rows[pick == k, 64 + DOFF:64 + DOFF + 20 + seg] = kinds[k]
    conn = np.arange(n, dtype=np.int64) % conns
    sport = 10000 + conn
    c = np.array(sums, np.int64)[pick] + sport
    c = (c & 0xFFFF) + (c >> 16)
    c = ~((c & 0xFFFF) + (c >> 16)) & 0xFFFF
    o = 64 + DOFF + 20
    rows[:, o], rows[:, o + 1] = sport >> 8, sport & 0xFF
    rows[:, o + 16], rows[:, o + 17] = c >> 8, c & 0xFF
    pool.hdr["tx_offload"] = 14 | 20 << 7 | 20 << 16
    pool.tot = 20 + seg
    pool.pcb = (1 + conn).astype(np.uint32)                         # the PCB index each mbuf finds
    pool.want = PRED_DATA if data else PRED_ACK
    reset(pool)
    return pool


def reset(pool):
    """The header fields the node moves, as ip4_proto hands them on."""
    pool.hdr["data_off"] = DOFF
    pool.hdr["data_len"] = pool.tot


class Runner:
    """One pass over the pool; `sec` collects [all queue / twin calls, submit + flush] of the pass."""

    def __init__(self, tables, pool, batch, do_churn):
        self.L, self.n, self.pool = N.lib(), pool.n, pool
        self.t, self.tc, self.tcb = tables
        self.conns, self.batch, self.do_churn = len(self.tcb) - 1, batch, do_churn
        self.ptrs = pool.ptrs(np.arange(pool.n))
        self.base = ctypes.addressof(self.ptrs)
        self.out = (ctypes.c_void_p * pool.n)()
        self.edges = np.zeros(pool.n, np.uint16)
        self.segs = np.zeros(pool.n, SEG_DT)
        self.opts = np.zeros(pool.n, OPT_DT)
        self.verdicts = np.zeros(pool.n, np.uint8)
        self.sec = [0.0, 0.0]

    def maybe_churn(self, b):
        if self.do_churn and b % self.batch == 0:
            churn(self.tc, self.tcb, self.conns)


class Twin(Runner):
    def run(self):
        L, ed, sg, op, vd = self.L, self.edges.ctypes.data, self.segs.ctypes.data, self.opts.ctypes.data, self.verdicts.ctypes.data
        for b in range(0, self.n, BURST):
            self.maybe_churn(b)
            t0 = time.perf_counter()
            rc = L.cndp_tcp_segment_node_host(self.t.h, self.tc.h, NOW, self.base + 8 * b, min(BURST, self.n - b), ed + 2 * b,
                                              sg + 16 * b, op + 16 * b, vd + b, None, 2048, None)
            self.sec[0] += time.perf_counter() - t0
            if rc:
                raise OSError(-rc, "cndp_tcp_segment_node_host")


class Loop(Runner):
    """A node's loop through one queue: mode 11 (poll_tcpseg), or with host=True mode 9
    (poll_tcp) and cndp_tcp_segment_host per burst over its records."""

    def __init__(self, q, tables, pool, batch, do_churn, host=False):
        super().__init__(tables, pool, batch, do_churn)
        self.q, self.host = q.h, host
        if host:
            n = pool.n
            self.offs = (np.arange(n, dtype=np.uint64) * FRAME + 64 + DOFF)
            self.rxmeta = np.full(n, 20 << 7, np.uint32)
            self.sel = np.ones(n, np.uint8)
            self.b = N.Batch()
            self.b.mode, self.b.slab, self.b.slab_len = N.CNDP_MODE_CNET, pool.mem.ctypes.data, pool.mem.size
            self.io = N.TcpSegIo()

    def poll(self, got):
        L, q, n = self.L, self.q, self.n
        out, ed, sg = ctypes.addressof(self.out), self.edges.ctypes.data, self.segs.ctypes.data
        if self.host:
            return L.cndp_gpu_mq_poll_tcp(q, out + 8 * got, ed + 2 * got, sg + 16 * got, n - got)
        return L.cndp_gpu_mq_poll_tcpseg(q, out + 8 * got, ed + 2 * got, sg + 16 * got, self.opts.ctypes.data + 16 * got,
                                         self.verdicts.ctypes.data + got, n - got)

    def run(self):
        L, q, n = self.L, self.q, self.n
        got = 0
        for b in range(0, n, BURST):
            self.maybe_churn(b)
            want = min(BURST, n - b)
            done = 0
            while done < want:
                t0 = time.perf_counter()
                k = L.cndp_gpu_mq_submit(q, self.base + 8 * (b + done), want - done)
                t1 = time.perf_counter()
                if k < 0:
                    raise OSError(-k, "cndp_gpu_mq_submit")
                done += k
                g = self.poll(got)
                got += g
                if k == 0 and g == 0:
                    L.cndp_gpu_mq_wait(q)
                t2 = time.perf_counter()
                self.sec[0] += t2 - t0
                self.sec[1] += t1 - t0
        t0 = time.perf_counter()
        while got < n:
            ta = time.perf_counter()
            L.cndp_gpu_mq_flush(q)
            self.sec[1] += time.perf_counter() - ta
            L.cndp_gpu_mq_wait(q)
            got += self.poll(got)
        if self.host:                                             # the lcore's own parse and triage, burst by burst
            b, io = self.b, self.io
            for lo in range(0, n, BURST):
                b.n = min(BURST, n - lo)
                b.offsets, b.rxmeta = self.offs.ctypes.data + 8 * lo, self.rxmeta.ctypes.data + 4 * lo
                io.sel, io.pcb, io.seg = self.sel.ctypes.data + lo, self.pool.pcb.ctypes.data + 4 * lo, self.segs.ctypes.data + 16 * lo
                io.opt, io.verdict = self.opts.ctypes.data + 16 * lo, self.verdicts.ctypes.data + lo
                rc = L.cndp_tcp_segment_host(self.tc.h, NOW, ctypes.byref(b), ctypes.byref(io))
                if rc:
                    raise OSError(-rc, "cndp_tcp_segment_host")
        self.sec[0] += time.perf_counter() - t0


def timed_interleaved(runners, warmup, reps, passes):
    """runners: name -> (runner, before).  Windows of `passes` passes each, the
    runners taking turns window by window; `before` runs in front of every pass,
    outside the clock.  Returns name -> [seconds, submit + flush seconds] per timed window."""
    t = {k: [] for k in runners}
    for w in range(warmup + reps):
        for name, (r, before) in runners.items():
            r.sec = [0.0, 0.0]
            for _ in range(passes):
                before()
                r.run()
            if w >= warmup:
                t[name].append(list(r.sec))
    return t


def summary(t, n, passes):
    r = sorted(n / x[0] / 1e6 for x in t)
    return {"mpps_median": float(np.median(r)), "mpps_min": r[0], "mpps_max": r[-1],
            "submit_flush_us_per_pass_median": float(np.median([x[1] for x in t])) / passes * 1e6,
            "seconds": [x[0] for x in t], "submit_flush_seconds": [x[1] for x in t]}


def verify(r, pool, name):
    r.run()
    ok = (r.edges == SEG).all() and ((r.verdicts & N.CNDP_TCPSEG_VERDICT) == pool.want).all() and (r.opts["ts_val"] == 95).all()
    if not ok:
        sys.exit(f"tcp_segment_mq_bench: {name}: not every mbuf came back on SEGMENT with the predicted verdict")
    reset(pool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--passes", type=int, default=64,
                    help="passes over the pool per timed window (a quarter of it for the 1460-byte cases and for churn)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcp_segment_mq_bench.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    if a.dry:
        for case, (conns, seg) in CASES.items():
            tables, pool = make_tables(conns), build_pool(min(a.pool, 1024), conns, seg)
            verify(Twin(tables, pool, a.batch, True), pool, case)
            print(case, "ok")
            tables[1].close()
            tables[0].close()
        print("dry OK")
        return
    if a.reps < 5:
        ap.error("--reps: at least five")
    import torch
    if not torch.cuda.is_available():
        sys.exit("tcp_segment_mq_bench: no GPU (a measurement does not fall back; --dry checks the set-up)")
    from cndp_amd.classify import Classifier
    cl = Classifier(0)
    res = {"box": torch.cuda.get_device_name(0), "hip": torch.version.hip, "cpu": _cpu_name(), "pool": a.pool, "burst": BURST,
           "batch": a.batch, "depth": a.depth, "warmup": a.warmup, "reps": a.reps, "passes": a.passes,
           "interleaved": True, "runs": 1, "cases": {}}
    for case, (conns, seg) in CASES.items():
        for mode in ("still", "churn"):
            ch = mode == "churn"
            tables = make_tables(conns)
            t, tc, _ = tables
            passes = max(1, a.passes // 4) if seg > 1000 or ch else a.passes
            pz, ps, p9 = (build_pool(a.pool, conns, seg) for _ in range(3))
            cl.host_register(pz.mem)
            cl.host_register(p9.mem)
            try:
                kw = dict(batch=a.batch, depth=a.depth, pcb_tbl=t)
                qz = MbufQueue(cl, N.CNDP_MQ_TCP_SEGMENT, umem=pz.base, tcb=tc, **kw)
                qs = MbufQueue(cl, N.CNDP_MQ_TCP_SEGMENT, tcb=tc, **kw)
                q9 = MbufQueue(cl, N.CNDP_MQ_TCP_INPUT, umem=p9.base, **kw)
                for q in (qz, qs):
                    q.set_now(NOW)
                rs = {"cpu_twin": (Twin(tables, ps, a.batch, ch), ps), "zero_copy": (Loop(qz, tables, pz, a.batch, ch), pz),
                      "staged": (Loop(qs, tables, ps, a.batch, ch), ps),
                      "mode9_host": (Loop(q9, tables, p9, a.batch, ch, host=True), p9)}
                for name, (r, pool) in rs.items():
                    verify(r, pool, f"{case}/{mode}/{name}")
                secs = timed_interleaved({k: (r, (lambda p=p: reset(p))) for k, (r, p) in rs.items()}, a.warmup, a.reps, passes)
                for name, tt in secs.items():
                    c = summary(tt, a.pool * passes, passes)
                    c["passes"] = passes
                    res["cases"][f"{case}/{mode}/{name}"] = c
                for q in (qz, qs, q9):
                    q.close()
            finally:
                cl.host_unregister(p9.mem)
                cl.host_unregister(pz.mem)
            tc.close()
            t.close()
    for k, v in res["cases"].items():
        print(f"{k:36s} {v['mpps_median']:8.2f} Mpps  ({v['mpps_min']:.2f} .. {v['mpps_max']:.2f})  "
              f"submit+flush {v['submit_flush_us_per_pass_median']:9.1f} us/pass")
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

#!/usr/bin/env python3
"""Measure the TCP option parse + header-prediction stage (cndp_gpu_tcp_segment)
on the C4 IMIX batch.

    python tools/tcp_segment_bench.py [--n 16777216] [--out profiles/tcp_segment.json]

The batch is tcp_demux_bench.py's case c: bench.py's C4 (pktgen.imix) with a
quarter of the IPv4 routes local, the frames ip4_input sends to its proto edge
rewritten as TCP segments of 4096 connections on one local port.  Every
connection has an established TCB, and the segments are what header prediction
takes:

  570- and 1500-byte frames  in-order data with NOP NOP TIMESTAMP (a 32-byte
                             header): PRED_DATA | TS_UPDATE, and the stage reads
                             the options
  64-byte frames             6 bytes of in-order data.  The 60 frame bytes of a
                             64-byte slot cannot hold a 32-byte TCP header behind
                             Ethernet and IPv4 (66 bytes), so these carry the
                             20-byte header: PRED_DATA, no frame read at all

With device events around every call (warm-up calls, then the median and the
min-max of --iters calls, each on an idle device): tcp_input (for scale) and
tcp_segment over tcp_input's arrays.  Bytes are algorithmic: per frame the
stage reads l4edge and pcb (5 B) and writes opt and verdict (17 B); per taken
frame it reads the segment record, rxmeta and the TCB entry (16 + 4 + 48 B), and
per segment with options a 64-byte line of the frame.  The host figure is
cndp_tcp_segment_host on one core over the batch's first frames.  --dry builds a
small batch on the CPU and checks the set-up (every taken frame is PRED_DATA by
the host twin and by tests/tcpseg_ref.py) without timing anything.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CONNS = 4096
NOW, TS_VAL, TS_ECR = 2000, 1000, 900
TCB = dict(rcv_nxt=1000, snd_una=5000, snd_nxt=6000, snd_max=6000, snd_wnd=1024 << 3, snd_cwnd=1 << 20,
           ts_recent=TS_VAL, last_ack_sent=900, rcv_space=65535, max_mss=1460, state=5, snd_scale=3, flags=1)


def add_options(ft, taken):
    """tcp_demux_bench.rewrite's TCP frames (20-byte header, zero payload) made
    header-prediction traffic in place: seq = rcv_nxt, ack = snd_una, window
    1024; frames of more than 64 bytes get NOP NOP TIMESTAMP.  The TCP checksum
    is set again.  Returns the number of frames with options."""
    import torch
    slab, dev = ft.slab, ft.slab.device
    lens = ft.lengths.to(dev)
    chunk = 1 << 21
    for s in range(0, ft.n, chunk):
        e = min(ft.n, s + chunk)
        m = taken[s:e]
        b4 = ft.offsets[s:e][m]
        big = lens[s:e][m] >= 66

        def put(o, v, nb, at=b4):
            v = torch.as_tensor(v, dtype=torch.int64, device=dev).expand(len(at))
            for j in range(nb):
                slab[at + o + j] = ((v >> (8 * (nb - 1 - j))) & 0xFF).to(torch.uint8)

        def be16(o):
            return slab[b4 + o].to(torch.int64) << 8 | slab[b4 + o + 1].to(torch.int64)

        def fold(v):
            v = (v >> 16) + (v & 0xFFFF)
            return (v >> 16) + (v & 0xFFFF)
        put(38, TCB["rcv_nxt"], 4)
        put(42, TCB["snd_una"], 4)
        put(46, torch.where(big, 0x8018, 0x5010), 2)         # data offset 8 + PSH|ACK, or 5 + ACK
        put(48, 1024, 2)
        put(50, 0, 2)
        bb = b4[big]
        put(54, 0x0101080A, 4, bb)
        put(58, TS_VAL, 4, bb)
        put(62, TS_ECR, 4, bb)
        l4len = be16(16) - 20
        psd = be16(26) + be16(28) + be16(30) + be16(32) + 6 + l4len
        opt_sum = 0x0101 + 0x080A + (TS_VAL >> 16) + (TS_VAL & 0xFFFF) + (TS_ECR >> 16) + (TS_ECR & 0xFFFF)
        hdr = sum(be16(o) for o in range(34, 54, 2)) + torch.where(big, opt_sum, 0)   # the payload is zero
        ck = (~fold(psd + hdr)) & 0xFFFF
        put(50, torch.where(ck == 0, torch.full_like(ck, 0xFFFF), ck), 2)
    return int((lens[taken] >= 66).sum())


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcp_segment.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import torch
    from cndp_amd import native as N
    from cndp_amd import pktgen
    from cndp_amd.l4 import TcbTable, alloc_l4_outputs, alloc_tcp_outputs, alloc_tcpseg_outputs, seg_records
    from l4_demux_bench import HBM_ACHIEVABLE_TBS, prepare
    from tcp_demux_bench import connections, rewrite, tcp_tables

    local32 = [ip for ip, d, _ in pktgen.l3fwd_routes() if d == 32]

    def tcb_table(pcbs):
        t = TcbTable(pcbs)
        for i in range(CONNS):
            t.set(i, **TCB)
        return t

    def host_rate(tcbs, ft, m, rxmeta, pcb, seg, edge):
        """cndp_tcp_segment_host over the batch's first m frames on this core."""
        end = int(ft.offsets[m]) if m < ft.n else ft.slab.numel()
        slab, offs = ft.slab[:end].cpu().numpy(), ft.offsets[:m].cpu().numpy().astype(np.uint64)
        kw = dict(l4edge=edge[:m], offsets=offs)
        got = tcbs.segment_host(slab, m, rxmeta[:m], pcb[:m], seg[:m], NOW, **kw)
        reps, dt = 0, 0.0
        while dt < 0.5:
            t0 = time.perf_counter()
            tcbs.segment_host(slab, m, rxmeta[:m], pcb[:m], seg[:m], NOW, **kw)
            dt += time.perf_counter() - t0
            reps += 1
        taken = int((got["verdict"] != 0).sum())
        return got, {"frames": m, "segments": taken, "passes": reps, "seconds": dt,
                     "Msegments_per_s": reps * taken / dt / 1e6, "Mframes_per_s": reps * m / dt / 1e6}

    if a.dry:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import l4_ref as R
        import tcp_ref as T
        import tcpseg_ref as S
        from cndp_amd.l4 import addr_net, port_net
        fr, fib, fib6, ports = prepare(min(a.n, 2048), "cpu")
        slab, offs = fr.slab.numpy(), fr.offsets.numpy()
        taken = torch.from_numpy((slab[offs + 12] == 8) & (slab[offs + 13] == 0))
        conns = connections(CONNS, 1, local32, ports)
        ft = rewrite(fr, taken, conns, 6)
        n_opt = add_options(ft, taken)
        hit, miss = tcp_tables(conns)
        tcbs = tcb_table(hit)
        ent = np.zeros(CONNS, R.ENTRY_DT)
        ent["laddr"] = [addr_net(int(x)) for x in conns[0]]
        ent["lport"] = [port_net(int(x)) for x in conns[1]]
        ent["faddr"] = [addr_net(int(x)) for x in conns[2]]
        ent["fport"] = [port_net(int(x)) for x in conns[3]]
        m = min(fr.n, 512)
        rx = np.full(m, 14 | 20 << 7, np.uint32)
        t = T.tcp_input_ref(ft.slab.numpy(), m, rx, ent, sel=taken.numpy()[:m], offsets=offs)
        assert t["stats"][0] == int(taken[:m].sum()) and not t["stats"][1:].any(), t["stats"]
        got = tcbs.segment_host(ft.slab.numpy(), m, rx, t["pcb"], t["seg"], NOW, l4edge=t["l4edge"],
                                offsets=offs.astype(np.uint64))
        want = S.tcp_segment_ref(ft.slab.numpy(), m, rx, [dict(TCB)] * CONNS, t["pcb"], t["seg"], NOW,
                                 l4edge=t["l4edge"], offsets=offs)
        assert (got["verdict"] == want["verdict"]).all() and (got["opt"] == want["opt"]).all()
        st = got["stats"].tolist()
        assert st[S.PRED_DATA] == int(taken[:m].sum()) > 0 and st[S.NONE] == m - st[S.PRED_DATA], st
        big = got["opt"]["sflags"] == S.TS_PRESENT
        assert big.sum() == int((ft.lengths[:m][taken[:m]] >= 66).sum()) > 0 and (got["opt"]["ts_ecr"][big] == TS_ECR).all()
        assert (got["opt"]["ts_val"][big] == TS_VAL).all() and ((got["verdict"][big] & 0x4F) == (S.PRED_DATA | S.TS_UPDATE)).all()
        print(f"dry: {int(taken.sum())} TCP segments of {fr.n} frames, {n_opt} with a timestamp: "
              f"first {m} frames: {st[S.PRED_DATA]} predicted data, {int(big.sum())} timestamps parsed, host twin == restatement")
        return 0
    if not torch.cuda.is_available():
        print("tcp_segment_bench: needs a GPU (no CPU fallback); --dry checks the set-up", file=sys.stderr)
        return 2

    from cndp_amd.classify import Classifier
    from cndp_amd.l4 import PcbTable
    dev = torch.device("cuda:0")
    fr, fib, fib6, ports = prepare(a.n, dev)
    cl = Classifier(0)
    cl.set_fib(fib, fib6)
    out = cl.alloc_outputs(fr.n, 64, device=dev, meta=True)
    l4 = alloc_l4_outputs(fr.n, dev)

    def timed(fn):
        ms = []
        for k in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}

    probe = PcbTable(1)
    cl.classify(fr, N.CNDP_MODE_CNET, out=out)
    cl.udp_input(fr, out, probe, l4=l4)
    torch.cuda.synchronize()
    taken = l4["l4edge"] != 0xFF
    n_taken = int(taken.sum())
    conns = connections(CONNS, 1, local32, ports)
    ft = rewrite(fr, taken, conns, 6)
    del fr
    n_opt = add_options(ft, taken)
    cl.classify(ft, N.CNDP_MODE_CNET, out=out)
    tcp_on = PcbTable(1)
    tcp_on.set_flags(tcp_enabled=True)
    cl.udp_input(ft, out, tcp_on, l4=l4)
    torch.cuda.synchronize()
    assert int((l4["l4edge"] == 0x02).sum()) == n_taken
    hit, miss = tcp_tables(conns)
    tcbs = tcb_table(hit)
    tcp = alloc_tcp_outputs(ft.n, dev, l4edge=l4["l4edge"])
    cl.tcp_input(ft, out, hit, l4=l4, tcp=tcp)
    torch.cuda.synchronize()
    assert tcp["stats"].cpu().tolist() == [n_taken, 0, 0, 0, 0], tcp["stats"]
    seg = alloc_tcpseg_outputs(ft.n, dev)
    cl.tcp_segment(ft, out, tcbs, tcp, now=NOW, seg=seg)
    torch.cuda.synchronize()
    st = seg["stats"].cpu().tolist()
    assert st == [ft.n - n_taken, 0, 0, 0, 0, 0, n_taken, 0], st
    assert int((seg["verdict"] & 0x40 != 0).sum()) == n_opt
    res = {"n": ft.n, "segments": n_taken, "segments_with_timestamp": n_opt, "connections": CONNS, "iters": a.iters,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS,
           "stats_one_call": st}
    sel = (tcp["l4edge"] == 0x21).to(torch.uint8)       # tcp_input again needs a selection: l4edge has moved on
    tcp2 = alloc_tcp_outputs(ft.n, dev)
    res["tcp_input"] = timed(lambda: cl.tcp_input(ft, out, hit, sel=sel, tcp=tcp2))
    del tcp2
    res["tcp_segment"] = timed(lambda: cl.tcp_segment(ft, out, tcbs, tcp, now=NOW, seg=seg))
    b = ft.n * (5 + 17) + n_taken * (16 + 4 + 48) + n_opt * 64
    res["tcp_segment"] |= {"bytes": b, "TBs": b / (res["tcp_segment"]["ms"] * 1e-3) / 1e12,
                           "Msegments_per_s": n_taken / (res["tcp_segment"]["ms"] * 1e-3) / 1e6}
    m = min(ft.n, a.host_frames)
    host = lambda t, dt: t[:m].cpu().numpy().view(dt)  # noqa: E731
    got, res["host_one_core"] = host_rate(tcbs, ft, m, host(out["rxmeta"], np.uint32), host(tcp["pcb"], np.uint32),
                                          seg_records(tcp["seg"][:m]), host(tcp["l4edge"], np.uint8))
    res["host_one_core"]["equal_to_device"] = bool(
        np.array_equal(got["verdict"], host(seg["verdict"], np.uint8))
        and np.array_equal(got["opt"].view(np.uint8), seg["opt"][:m].cpu().numpy().view(np.uint8).reshape(-1)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

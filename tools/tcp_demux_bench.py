#!/usr/bin/env python3
"""Measure the TCP connection demux stage (cndp_gpu_tcp_input) on the C4 IMIX batch.

    python tools/tcp_demux_bench.py [--n 16777216] [--out profiles/tcp_demux.json]

The batch is l4_demux_bench.py's: bench.py's C4 (pktgen.imix) with a quarter of
the IPv4 routes local.  The frames ip4_input sends to its proto edge are then
given connection 4-tuples -- the destination one of the /32 local addresses,
the source address and both ports those of a connection drawn per frame -- once
as UDP datagrams and once as TCP segments (20-byte header, the rest of the
frame as it was: the same number of bytes under the checksum), with the
checksums set right.  Three connection tables:

  a  512 connections on 512 local ports
  b  512 connections on one local port
  c  4096 connections on one local port

For each, with device events around every call (warm-up calls, then the median
and the min-max of --iters calls, each on an idle device):

  tcp_input        lookup + checksum + segment record, every taken frame a hit
  tcp_input_miss   the same batch against the table with every foreign address
                   changed: the image, the exact probe and the port walk cost the
                   same and nothing reaches the checksum kernel, so the
                   difference to tcp_input is the checksum pass
  udp_cksum        cndp_gpu_udp_input on the UDP form of the same frames,
                   UDP_CHKSUM_FLAG on, 512 any-address listeners (table a's ports;
                   for b and c one listener), beside udp_demux (flags off)

Bytes are algorithmic, as in l4_demux_bench.py.  The host figures are
cndp_pcb_lookup and cndp_pcb_lookup_indexed on one core over table c and a
sample of batch c's keys.  --dry builds a small batch on the CPU and checks the
set-up (every rewritten frame finds its connection, every checksum verifies)
without timing anything.
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
CASES = {"a": (512, 512), "b": (512, 1), "c": (4096, 1)}   # connections, local ports


def connections(k, n_ports, local32, ports):
    """k connection 4-tuples, host order: (laddr, lport, faddr, fport) arrays."""
    c = np.arange(k, dtype=np.int64)
    return (np.array(local32, np.int64)[c % len(local32)], np.asarray(ports, np.int64)[c % n_ports],
            0xC6130000 + c, 1024 + (c * 7) % 60000)


def rewrite(fr, taken, conns, proto, seed_field=91):
    """A copy of `fr` whose taken IPv4 frames carry a drawn connection's 4-tuple
    as UDP (17) or TCP (6), IPv4 and L4 checksums right."""
    import torch
    from cndp_amd import pktgen
    dev = fr.slab.device
    la, lp, fa, fp = (torch.from_numpy(x).to(dev) for x in conns)
    slab = fr.slab.clone()
    chunk = 1 << 21
    for s in range(0, fr.n, chunk):
        e = min(fr.n, s + chunk)
        m = taken[s:e]
        b4 = fr.offsets[s:e][m]
        idx = torch.arange(s, e, dtype=torch.int64, device=dev)[m]
        c = pktgen.rnd(pktgen.SEED, idx, seed_field) % len(la)

        def put(o, v, nb):
            for j in range(nb):
                slab[b4 + o + j] = ((v >> (8 * (nb - 1 - j))) & 0xFF).to(torch.uint8)

        def be16(o):
            return slab[b4 + o].to(torch.int64) << 8 | slab[b4 + o + 1].to(torch.int64)

        def fold(v):
            v = (v >> 16) + (v & 0xFFFF)
            return (v >> 16) + (v & 0xFFFF)
        put(26, fa[c], 4)
        put(30, la[c], 4)
        put(34, fp[c], 2)
        put(36, lp[c], 2)
        slab[b4 + 23] = proto
        put(24, torch.zeros_like(c), 2)
        put(24, (~fold(sum(be16(o) for o in range(14, 34, 2)))) & 0xFFFF, 2)
        l4len = be16(16) - 20
        psd = be16(26) + be16(28) + be16(30) + be16(32) + proto + l4len + fp[c] + lp[c]
        if proto == 17:     # the payload is zero: the sum is the pseudo header's and the UDP header's
            ck = (~fold(psd + l4len)) & 0xFFFF
            put(40, torch.where(ck == 0, torch.full_like(ck, 0xFFFF), ck), 2)
        else:               # seq = ack = 0, data offset 5, ACK, window 0xffff, no urgent pointer
            put(38, torch.zeros_like(c), 8)
            put(46, torch.full_like(c, 0x5010), 2)
            put(48, torch.full_like(c, 0xFFFF), 2)
            put(52, torch.zeros_like(c), 2)
            ck = (~fold(psd + 0x5010 + 0xFFFF)) & 0xFFFF
            put(50, torch.where(ck == 0, torch.full_like(ck, 0xFFFF), ck), 2)
    from cndp_amd.pktgen import Frames
    return Frames(slab, fr.n, stride=fr.stride, offsets=fr.offsets, data_off=fr.data_off, lengths=fr.lengths)


def tcp_tables(conns):
    """The connection table, and the same with every foreign address changed."""
    from cndp_amd.l4 import PcbTable
    la, lp, fa, fp = conns
    hit, miss = PcbTable(len(la)), PcbTable(len(la))
    for k in range(len(la)):
        hit.add(laddr=int(la[k]), lport=int(lp[k]), faddr=int(fa[k]), fport=int(fp[k]))
        miss.add(laddr=int(la[k]), lport=int(lp[k]), faddr=int(fa[k]) ^ 0x00400000, fport=int(fp[k]))
    return hit, miss


def udp_tables(lports):
    from cndp_amd.l4 import PcbTable
    off, on = PcbTable(len(lports)), PcbTable(len(lports))
    for p in lports:
        off.add(lport=int(p))
        on.add(lport=int(p), cksum=True)
    return off, on


def keys_of(fr, sel_idx):
    """struct cndp_pcb_key array of the frames `sel_idx` (IPv4 at +14, no options)."""
    import torch
    from cndp_amd.l4 import make_keys
    base = fr.offsets[sel_idx] + 14
    rd = lambda o, k: torch.stack([fr.slab[base + o + j] for j in range(k)], 1).cpu().numpy()  # noqa: E731
    return make_keys(rd(16, 4).copy().view("<u4")[:, 0], rd(22, 2).copy().view("<u2")[:, 0],
                     rd(12, 4).copy().view("<u4")[:, 0], rd(20, 2).copy().view("<u2")[:, 0])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcp_demux.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import torch
    from cndp_amd import native as N
    from cndp_amd import pktgen
    from l4_demux_bench import HBM_ACHIEVABLE_TBS, prepare

    local32 = [ip for ip, d, _ in pktgen.l3fwd_routes() if d == 32]
    if a.dry:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import l4_ref as R
        import tcp_ref as T
        from cndp_amd.l4 import addr_net, port_net
        fr, fib, fib6, ports = prepare(min(a.n, 2048), "cpu")
        slab, offs = fr.slab.numpy(), fr.offsets.numpy()
        taken = torch.from_numpy((slab[offs + 12] == 8) & (slab[offs + 13] == 0))
        for name, (k, n_ports) in CASES.items():
            conns = connections(k, n_ports, local32, ports)
            ft = rewrite(fr, taken, conns, 6)
            hit, miss = tcp_tables(conns)
            keys = keys_of(ft, torch.nonzero(taken)[:, 0])
            assert (hit.lookup_indexed(keys) != N.CNDP_PCB_NONE).all() and (hit.lookup(keys) == hit.lookup_indexed(keys)).all()
            assert (miss.lookup_indexed(keys) == N.CNDP_PCB_NONE).all()
            ent = np.zeros(k, R.ENTRY_DT)
            ent["laddr"] = [addr_net(int(x)) for x in conns[0]]
            ent["lport"] = [port_net(int(x)) for x in conns[1]]
            ent["faddr"] = [addr_net(int(x)) for x in conns[2]]
            ent["fport"] = [port_net(int(x)) for x in conns[3]]
            m = min(fr.n, 256)
            want = T.tcp_input_ref(ft.slab.numpy(), m, np.full(m, 14 | 20 << 7, np.uint32), ent, sel=taken.numpy()[:m],
                                   offsets=offs)
            assert want["stats"][0] == int(taken[:m].sum()) and not want["stats"][1:].any(), want["stats"]
            fu = rewrite(fr, taken, conns, 17)
            for i in np.nonzero(taken.numpy()[:m])[0]:
                assert R.cksum_verify(R.View(fu.slab.numpy()), int(offs[i]) + 14, 20)
            print(f"dry {name}: {int(taken.sum())} IPv4 frames of {fr.n}: every one finds its connection, "
                  f"TCP and UDP checksums verify")
        return 0
    if not torch.cuda.is_available():
        print("tcp_demux_bench: needs a GPU (no CPU fallback); --dry checks the set-up", file=sys.stderr)
        return 2

    from cndp_amd.classify import Classifier
    from cndp_amd.l4 import PcbTable, alloc_l4_outputs, alloc_tcp_outputs
    dev = torch.device("cuda:0")
    fr, fib, fib6, ports = prepare(a.n, dev)
    cl = Classifier(0)
    cl.set_fib(fib, fib6)
    out = cl.alloc_outputs(fr.n, 64, device=dev, meta=True)
    l4 = alloc_l4_outputs(fr.n, dev)
    lens = fr.lengths.to(dev)

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

    # the frames ip4_input sends to its proto edge, found once on the batch as generated
    probe = PcbTable(1)
    cl.classify(fr, N.CNDP_MODE_CNET, out=out)
    cl.udp_input(fr, out, probe, l4=l4)
    torch.cuda.synchronize()
    taken = l4["l4edge"] != 0xFF
    n_taken = int(taken.sum())
    seg_bytes = int((lens[taken] - 34).sum())     # the bytes under the L4 checksum, UDP and TCP alike
    res = {"n": fr.n, "frames_taken": n_taken, "checksum_bytes": seg_bytes, "iters": a.iters, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS, "cases": {}}
    tcp_on = PcbTable(1)
    tcp_on.set_flags(tcp_enabled=True)
    for name, (k, n_ports) in CASES.items():
        conns = connections(k, n_ports, local32, ports)
        case = {"connections": k, "local_ports": n_ports}
        # UDP form
        fu = rewrite(fr, taken, conns, 17)
        cl.classify(fu, N.CNDP_MODE_CNET, out=out)
        off, on = udp_tables(sorted(set(conns[1].tolist())))
        for nm, tbl in (("udp_demux", off), ("udp_cksum", on)):
            l4["stats"].zero_()
            cl.udp_input(fu, out, tbl, l4=l4)
            torch.cuda.synchronize()
            st = l4["stats"].cpu().tolist()
            case[nm] = timed(lambda: cl.udp_input(fu, out, tbl, l4=l4)) | {"stats_one_call": st}
            assert case[nm]["stats_one_call"][0] == n_taken, case[nm]
        del fu
        # TCP form
        ft = rewrite(fr, taken, conns, 6)
        cl.classify(ft, N.CNDP_MODE_CNET, out=out)
        cl.udp_input(ft, out, tcp_on, l4=l4)
        torch.cuda.synchronize()
        sel = (l4["l4edge"] == 0x02).to(torch.uint8)
        assert int(sel.sum()) == n_taken
        hit, miss = tcp_tables(conns)
        tcp = alloc_tcp_outputs(fr.n, dev)
        for nm, tbl in (("tcp_input", hit), ("tcp_input_miss", miss)):
            tcp["stats"].zero_()
            cl.tcp_input(ft, out, tbl, sel=sel, tcp=tcp)
            torch.cuda.synchronize()
            st = tcp["stats"].cpu().tolist()
            case[nm] = timed(lambda: cl.tcp_input(ft, out, tbl, sel=sel, tcp=tcp)) | {"stats_one_call": st}
        assert case["tcp_input"]["stats_one_call"] == [n_taken, 0, 0, 0, 0], case["tcp_input"]
        assert case["tcp_input_miss"]["stats_one_call"] == [0, n_taken, 0, 0, 0], case["tcp_input_miss"]
        assert len(torch.unique(tcp["pcb"])) == 1         # the miss table ran last
        # per frame: sel 1 B + rxmeta 4 B read, 27 B of outputs written; a 64-B line per taken
        # frame; a 16-B worklist entry written and read per hit; the segment's bytes
        case["tcp_input"]["bytes"] = fr.n * (5 + 27) + n_taken * (64 + 32) + seg_bytes
        case["tcp_input"]["TBs"] = case["tcp_input"]["bytes"] / (case["tcp_input"]["ms"] * 1e-3) / 1e12
        ck_tcp = case["tcp_input"]["ms"] - case["tcp_input_miss"]["ms"]
        ck_udp = case["udp_cksum"]["ms"] - case["udp_demux"]["ms"]
        case["cksum_pass"] = {"tcp_ms": ck_tcp, "udp_ms": ck_udp,
                              "tcp_GB_per_ms": seg_bytes / ck_tcp / 1e9 if ck_tcp > 0 else None,
                              "udp_GB_per_ms": seg_bytes / ck_udp / 1e9 if ck_udp > 0 else None}
        if name == "c":     # host lookups, one core, a sample of the taken frames' keys
            idx = torch.nonzero(sel[:min(fr.n, 1 << 20)])[:, 0]
            keys = keys_of(ft, idx)
            want = None
            for fn_name in ("lookup", "lookup_indexed"):
                fn = getattr(hit, fn_name)
                fn(keys[:1000])
                reps, dt = 0, 0.0
                while dt < 0.25:        # the indexed lookup needs many passes to fill a timing window
                    t0 = time.perf_counter()
                    got = fn(keys)
                    dt += time.perf_counter() - t0
                    reps += 1
                want = got if want is None else want
                res["host_" + fn_name] = {"keys": len(keys), "passes": reps, "seconds": dt,
                                          "Mkeys_per_s": reps * len(keys) / dt / 1e6,
                                          "equal": bool(np.array_equal(got, want))}
        res["cases"][name] = case
        del ft, hit, miss, off, on
    spread = max(c["tcp_input"]["ms_max"] - c["tcp_input"]["ms_min"] for c in res["cases"].values())
    res["c_minus_a_ms"] = res["cases"]["c"]["tcp_input"]["ms"] - res["cases"]["a"]["tcp_input"]["ms"]
    res["run_to_run_spread_ms"] = spread
    res["c_costs_no_more_than_a"] = res["c_minus_a_ms"] <= spread
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Measure the UDP socket demux stage (cndp_gpu_udp_input) on the C4 IMIX batch.

    python tools/l4_demux_bench.py [--n 16777216] [--out profiles/l4_demux.json]

The batch is bench.py's C4 (pktgen.imix, IPv4 / IPv6 mix) with a quarter of the
IPv4 routes made local (ip4_input's proto edge) and 512 UDP sockets, one
any-address listener per port; the IPv4 frames' destination ports are spread
over those ports and their UDP checksums are set right, so that with the
sockets' UDP_CHKSUM_FLAG on every matched datagram is verified (and passes).
Three stages are timed with device events (warm-up, then the median of
--iters calls, each on an idle device):

  classify     cndp_gpu_classify, CNDP_MODE_CNET, with ptype / rxmeta
  demux        cndp_gpu_udp_input, checksum flags off
  demux_cksum  cndp_gpu_udp_input, checksum flags on

Bytes are algorithmic, computed from the batch: per frame the classify outputs
the stage reads (nh, ptype, rxmeta: 12 B) and the outputs it writes (13 B), one
64-B line per taken frame, and for demux_cksum the verified datagrams' bytes.
The host figure is cndp_pcb_lookup on one core over the same keys.  --dry
builds a small batch on the CPU and checks the set-up without timing anything.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE_TBS = 6.29   # MI355X achievable HBM rate the project's figures are held against


def prepare(n, device, n_socks=512, seed=None):
    """The frames, the FIBs (a quarter of the IPv4 routes local) and the socket ports."""
    import torch
    from cndp_amd import native as N
    from cndp_amd import pktgen
    from cndp_amd.fib import Fib, Fib6, node_ip6_add_input
    routes, v6 = pktgen.l3fwd_routes(), pktgen.v6_routes()
    default = 1025
    fib = Fib("l4b-4", N.CNE_FIB_DIR24_8, default_nh=default, max_routes=1024, nh_sz=N.CNE_FIB_DIR24_8_4B,
              num_tbl8=256)
    for i, (ip, d, _) in enumerate(routes):   # cne_node_ip4_add_input's value, PROTO for every 4th route
        assert fib.add(ip, d, i | ((2 if i % 4 == 0 or d == 32 else 1) << 24)) == 0
    fib6 = Fib6("l4b-6", N.CNE_FIB_TRIE, default_nh=default, max_routes=1024, nh_sz=N.CNE_FIB_TRIE_4B,
                num_tbl8=1 << 15)
    for ip, d, i in v6:
        assert node_ip6_add_input(fib6, ip, d, i) == 0
    fr = pktgen.imix(n, v4routes=routes, v6routes=v6, device=device, **({"seed": seed} if seed else {}))
    ports = torch.arange(n_socks, dtype=torch.int64, device=device) * 97 + 1024   # host order, distinct
    # IPv4 frames: destination port from the socket set, then the UDP checksum
    # (payload bytes are zero, so the sum is the pseudo header's and the UDP header's)
    chunk = 1 << 21
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        base = fr.offsets[s:e]
        is4 = (fr.slab[base + 12] == 0x08) & (fr.slab[base + 13] == 0x00)
        b4 = base[is4]
        idx = torch.arange(s, e, dtype=torch.int64, device=device)[is4]
        dport = ports[pktgen.rnd(pktgen.SEED, idx, 77) % n_socks]

        def be16(o):
            return fr.slab[b4 + o].to(torch.int64) << 8 | fr.slab[b4 + o + 1].to(torch.int64)
        ulen = be16(38)
        c = be16(26) + be16(28) + be16(30) + be16(32) + 17 + ulen + be16(34) + dport + ulen
        c = (c >> 16) + (c & 0xFFFF)
        c = (c >> 16) + (c & 0xFFFF)
        c = (~c) & 0xFFFF
        c = torch.where(c == 0, torch.full_like(c, 0xFFFF), c)
        for o, v in ((36, dport >> 8), (37, dport & 0xFF), (40, c >> 8), (41, c & 0xFF)):
            fr.slab[b4 + o] = v.to(torch.uint8)
    return fr, fib, fib6, ports.cpu().numpy()


def tables(ports):
    from cndp_amd.l4 import PcbTable
    off, on = PcbTable(len(ports)), PcbTable(len(ports))
    for p in ports:
        off.add(lport=int(p))
        on.add(lport=int(p), cksum=True)
    return off, on


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l4_demux.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import torch
    from cndp_amd import native as N
    from cndp_amd.l4 import make_keys

    if a.dry:
        fr, fib, fib6, ports = prepare(min(a.n, 4096), "cpu")
        off, on = tables(ports)
        assert off.count() == on.count() == 512
        slab, offs = fr.slab.numpy(), fr.offsets.numpy()
        is4 = (slab[offs + 12] == 8) & (slab[offs + 13] == 0)
        lp = slab[offs[is4] + 36].astype(np.uint16) | slab[offs[is4] + 37].astype(np.uint16) << 8
        keys = make_keys(1, lp, 2, 0)
        assert (on.lookup(keys) != N.CNDP_PCB_NONE).all()
        print(f"dry: {int(is4.sum())} IPv4 frames of {fr.n}, every destination port has a socket")
        return 0
    if not torch.cuda.is_available():
        print("l4_demux_bench: needs a GPU (no CPU fallback); --dry checks the set-up", file=sys.stderr)
        return 2

    from cndp_amd.classify import Classifier
    from cndp_amd.l4 import alloc_l4_outputs
    dev = torch.device("cuda:0")
    fr, fib, fib6, ports = prepare(a.n, dev)
    off, on = tables(ports)
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
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    res = {"n": fr.n, "sockets": len(ports), "iters": a.iters, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS, "stages": {}}
    t = timed(lambda: cl.classify(fr, N.CNDP_MODE_CNET, out=out))
    res["stages"]["classify"] = {"ms": t[0], "ms_min": t[1], "ms_max": t[2], "frames": fr.n,
                                 "bytes": fr.n * (64 + 4 + 4 + 2 + 1 + 4 + 4)}
    lens = fr.lengths.to(dev)
    for name, tbl in (("demux", off), ("demux_cksum", on)):
        l4["stats"].zero_()
        cl.udp_input(fr, out, tbl, l4=l4)
        torch.cuda.synchronize()
        stats = l4["stats"].cpu().numpy().tolist()
        edge = l4["l4edge"]
        taken = int((edge != 0xFF).sum())
        matched = (edge == 0x11) | (edge == 0x10)
        dgram = int((lens[matched] - 34).sum()) if name == "demux_cksum" else 0
        t = timed(lambda: cl.udp_input(fr, out, tbl, l4=l4))
        res["stages"][name] = {"ms": t[0], "ms_min": t[1], "ms_max": t[2], "frames_taken": taken,
                               "stats_one_call": stats, "bytes": fr.n * (12 + 13) + taken * 64 + dgram,
                               "datagram_bytes": dgram}
    for st in res["stages"].values():
        st["TBs"] = st["bytes"] / (st["ms"] * 1e-3) / 1e12
        st["share_of_achievable"] = st["TBs"] / HBM_ACHIEVABLE_TBS
    res["demux_faster_than_classify"] = res["stages"]["demux"]["ms"] < res["stages"]["classify"]["ms"]

    # host cndp_pcb_lookup, one core, the same keys (a 1M-frame sample of the taken frames)
    m = min(fr.n, 1 << 20)
    sel = torch.nonzero(l4["l4edge"][:m] != 0xFF)[:, 0]
    base = fr.offsets[:m][sel] + 14
    rd = lambda o, k: torch.stack([fr.slab[base + o + j] for j in range(k)], 1).cpu().numpy()  # noqa: E731
    keys = make_keys(rd(16, 4).copy().view("<u4")[:, 0], rd(22, 2).copy().view("<u2")[:, 0],
                     rd(12, 4).copy().view("<u4")[:, 0], rd(20, 2).copy().view("<u2")[:, 0])
    on.lookup(keys[:1000])
    t0 = time.perf_counter()
    idx = on.lookup(keys)
    dt = time.perf_counter() - t0
    want = l4["pcb"][:m][sel].cpu().numpy().view(np.uint32)
    res["host_lookup"] = {"keys": len(keys), "seconds": dt, "Mkeys_per_s": len(keys) / dt / 1e6,
                          "equal_to_device": bool(np.array_equal(idx, want))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

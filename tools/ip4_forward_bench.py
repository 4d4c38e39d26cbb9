#!/usr/bin/env python3
"""Measure the ip4_forward stage (cndp_gpu_ip4_forward) on the C4 IMIX batch.

    python tools/ip4_forward_bench.py [--n 16777216] [--out profiles/ip4_forward.json]

The batch is bench.py's C4 (pktgen.imix, IPv4 / IPv6 mix) classified in cnet
mode; the IPv4 frames on the /24 routes leave ip4_input on its forward edge and
are the frames the stage takes (derived selection).  Three forwarding tables:

  direct    every route's /24 in the ARP FIB: one lookup, the MACs written
  gateway   every route's /24 in the route FIB, four gateways in the ARP FIB:
            three dependent lookups; in a 4-wide group lanes 1-3 take lane 0's ha
  miss      empty FIBs: two lookups, every taken frame to arp_request

Timing uses device events: --warmup calls, then the median (min-max) of --iters,
each on an idle device.  The stage rewrites TTL and checksum in place, so every
timed call works on the slab the previous one left (the arithmetic does not
depend on the values).  Beside them, from the same run: the cnet classify and,
on an l3fwd classify of the same batch, the ip4_rewrite stage.  Bytes are
algorithmic, computed from the batch: per frame the classify outputs the stage
reads (nh, ptype, rxmeta: 12 B) and the outputs it writes (8 B); per taken frame
one 64-B line read and written back; FIB and object reads are not counted (the
tables are cache-resident).  --dry builds a small batch and the three tables
on the CPU and checks the set-up against cndp_fwd_lookup without timing.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE_TBS = 6.29   # MI355X achievable HBM rate the project's figures are held against
ARP_N = RT_N = 1024


def cnet_fibs():
    from cndp_amd import native as N
    from cndp_amd import pktgen
    from cndp_amd.fib import Fib, Fib6, node_ip4_add_input, node_ip6_add_input
    routes, v6 = pktgen.l3fwd_routes(), pktgen.v6_routes()
    fib = Fib("fwb-4", N.CNE_FIB_DIR24_8, default_nh=1025, max_routes=1024, nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=256)
    for i, (ip, d, _) in enumerate(routes):
        assert node_ip4_add_input(fib, ip, d, i) == 0
    fib6 = Fib6("fwb-6", N.CNE_FIB_TRIE, default_nh=1025, max_routes=1024, nh_sz=N.CNE_FIB_TRIE_4B, num_tbl8=1 << 15)
    for ip, d, i in v6:
        assert node_ip6_add_input(fib6, ip, d, i) == 0
    return fib, fib6, routes, v6


def table(kind: str, routes):
    """(arp Fib, rt4 Fib, FwdTable) of one of the three shapes."""
    from cndp_amd import native as N
    from cndp_amd.fib import Fib
    from cndp_amd.fwd import FwdTable
    mk = lambda name, cap: Fib(name, N.CNE_FIB_DIR24_8, default_nh=cap + 1, max_routes=2048,  # noqa: E731
                               nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=256)
    arp, rt4 = mk("arp-fib", ARP_N), mk("rt4-fib", RT_N)
    tbl = FwdTable(arp, rt4, ARP_N, RT_N)
    for k in range(8):
        assert tbl.netif_set(k, bytes([2, 0x10, 0, 0, 0, k])) == 0
    fwd = [(ip, d) for ip, d, _ in routes if d == 24]
    if kind == "direct":
        for i in range(64):
            assert tbl.arp_set(i, i % 8, bytes([2, 0xAA, 0, 0, 0, i])) == 0
        for i, (ip, d) in enumerate(fwd):
            assert arp.add(ip, d, i % 64) == 0
    elif kind == "gateway":
        gws = [0xC0A80001 + k for k in range(4)]
        for k, g in enumerate(gws):     # the gateway's s_addr is looked up as it is stored
            assert tbl.arp_set(k, k, bytes([2, 0xBB, 0, 0, 0, k])) == 0
            assert arp.add(g, 32, k) == 0
        for i in range(64):
            assert tbl.rt_set(i, gws[i % 4], i % 8) == 0
        for i, (ip, d) in enumerate(fwd):
            assert rt4.add(ip, d, i % 64) == 0
    return arp, rt4, tbl


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip4_forward.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import torch
    from cndp_amd import native as N
    from cndp_amd import pktgen

    if a.dry:
        fib, fib6, routes, v6 = cnet_fibs()
        fr = pktgen.imix(min(a.n, 4096), v4routes=routes, v6routes=v6, device="cpu")
        slab, offs = fr.slab.numpy(), fr.offsets.numpy()
        is4 = (slab[offs + 12] == 8) & (slab[offs + 13] == 0)
        dst = np.stack([slab[offs[is4] + 30 + k] for k in range(4)], 1).copy().view("<u4")[:, 0]
        for kind, want in (("direct", lambda e: (e >= 2).mean() > 0.5), ("gateway", lambda e: (e >= 2).mean() > 0.5),
                           ("miss", lambda e: (e == 1).all())):
            arp, rt4, tbl = table(kind, routes)
            e = tbl.lookup(dst)["edge"]
            assert want(e), kind
            print(f"dry: {kind}: {int((e >= 2).sum())} of {len(e)} IPv4 destinations transmitted")
            tbl.close()
        return 0
    if not torch.cuda.is_available():
        print("ip4_forward_bench: needs a GPU (no CPU fallback); --dry checks the set-up", file=sys.stderr)
        return 2

    from cndp_amd.classify import Classifier
    from cndp_amd.fib import Fib, node_ip4_route_add
    from cndp_amd.fwd import alloc_fwd_outputs
    dev = torch.device("cuda:0")
    fib, fib6, routes, v6 = cnet_fibs()
    fr = pktgen.imix(a.n, v4routes=routes, v6routes=v6, device=dev)
    cl = Classifier(0)
    cl.set_fib(fib, fib6)
    out = cl.alloc_outputs(fr.n, 64, device=dev, meta=True)
    fwd = alloc_fwd_outputs(fr.n, dev)

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

    res = {"n": fr.n, "burst": a.burst, "iters": a.iters, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS, "stages": {}}
    st = timed(lambda: cl.classify(fr, N.CNDP_MODE_CNET, out=out))
    st.update(frames=fr.n, bytes=fr.n * (64 + 4 + 4 + 2 + 1 + 4 + 4))
    res["stages"]["classify_cnet"] = st
    for kind in ("direct", "gateway", "miss"):
        arp, rt4, tbl = table(kind, routes)
        fwd["stats"].zero_()
        cl.ip4_forward(fr, out, tbl, burst=a.burst, n_bins=8, fwd=fwd)
        torch.cuda.synchronize()
        stats = fwd["stats"].cpu().numpy().tolist()
        taken = int((fwd["fwd_edge"] != -1).sum())
        st = timed(lambda: cl.ip4_forward(fr, out, tbl, burst=a.burst, n_bins=8, fwd=fwd))
        st.update(frames_taken=taken, stats_one_call=stats, bytes=fr.n * (12 + 8) + taken * 128)
        res["stages"]["ip4_forward_" + kind] = st
        torch.cuda.synchronize()
        tbl.close()
        arp.close()
        rt4.close()
    # the l3fwd chain's forwarding stage on the same batch
    fib3 = Fib("fwb-l3", N.CNE_FIB_DIR24_8, default_nh=N.IP4_LOOKUP_NEXT_PKT_DROP << 16, max_routes=1024,
               nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=256)
    for ip, d, nh in routes:
        assert node_ip4_route_add(fib3, ip, d, nh, N.IP4_LOOKUP_NEXT_REWRITE) == 0
    cl.set_fib(fib3, fib6)
    out3 = cl.alloc_outputs(fr.n, 64, device=dev)
    cl.classify(fr, N.CNDP_MODE_L3FWD, out=out3)
    for p in range(4):
        cl.rewrite_set_next(p, p + 1)
    for nh in range(64):
        assert cl.rewrite_add(nh, bytes([2, 0xAA, 0, 0, 0, nh, 2, 0x10, 0, 0, 0, nh % 4]), nh % 4) == 0
    tx = torch.empty(fr.n, dtype=torch.int16, device=dev)
    cl.ip4_rewrite(fr, out3["nh"], burst=a.burst, tx_edge=tx)
    torch.cuda.synchronize()
    rw = int((tx != -1).sum())
    st = timed(lambda: cl.ip4_rewrite(fr, out3["nh"], burst=a.burst, tx_edge=tx))
    st.update(frames_taken=rw, bytes=fr.n * (4 + 2) + rw * 128)
    res["stages"]["ip4_rewrite"] = st
    for st in res["stages"].values():
        st["TBs"] = st["bytes"] / (st["ms"] * 1e-3) / 1e12
        st["share_of_achievable"] = st["TBs"] / HBM_ACHIEVABLE_TBS
        st["Mpps"] = fr.n / (st["ms"] * 1e-3) / 1e6
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

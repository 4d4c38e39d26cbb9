#!/usr/bin/env python3
"""Measure cndpfwd's fwd and l3fwd stage (cndp_gpu_cfwd) on the C3 batch
(bench.py's 16M packed 64-byte IPv4/UDP frames, pktgen.l3fwd_routes() packed as
48-bit next hops into an l3fwd_fib_init FIB) against what a user can compose
without it.

    python tools/cndpfwd_bench.py [--n 16777216] [--out profiles/cndpfwd_l3.json]

Four device stages, interleaved in one process: every round runs each of them
once, in this order, each on an idle device and timed with device events;
--warmup rounds, then --iters rounds.  Per stage the median (min-max) over the
rounds, and four ratios, each the median over the rounds of the per-round ratio
(so that a drift of the box hits numerator and denominator alike):

  (a) mac_swap   cndp_gpu_mac_swap on the batch
  (b) lookup     cndp_fib_lookup_dev on the batch's destination addresses from a
                 contiguous array, into a contiguous array (the same 8-byte FIB)
  (c) fwd        cndp_gpu_cfwd in FWD mode
  (d) l3fwd      cndp_gpu_cfwd in L3FWD mode

  fwd / mac_swap, l3fwd / mac_swap, l3fwd / fwd, l3fwd / (mac_swap + lookup)

(a) + (b) is what a user can compose today, and it still lacks the gather of the
addresses out of the frames, the TTL and checksum step and the MAC rewrite.  The
stages edit the slab in place; none changes what a later one reads to decide
(the destination address stays; p[5] alternates between two known ports).

Beside them cndp_cfwd_host on one core over the first --host-n frames, both modes.
Bytes are algorithmic: per frame one 64-byte line read and written back, plus
the outputs written (nh 8, tx_lport 2, echoed 1, bin_of 2; the lookup: 4 read,
8 written); FIB gathers are not counted.  --dry builds a small batch on the CPU
and checks the set-up against the host rule without timing.
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
LPORTS = (0, 1, 2, 3)


def c3_fib(routes):
    """pktgen.l3fwd_routes() as cndpfwd would hold them: next hop id k becomes
    MAC 02:00:00:00:00:k on port k % 4."""
    from cndp_amd.cfwd import l3fwd_fib, route_add
    fib = l3fwd_fib("c3")
    for ip, depth, nh in routes:
        route_add(fib, ip, depth, bytes([2, 0, 0, 0, nh >> 8, nh & 0xFF]), nh % 4)
    return fib


def dst_addrs(fr):
    """The frames' destination addresses in host order, as an int32 tensor."""
    import torch
    v = fr.slab.view(fr.n, 64)[:, 30:34].to(torch.int64)
    ip = v[:, 0] << 24 | v[:, 1] << 16 | v[:, 2] << 8 | v[:, 3]
    return torch.where(ip >= 1 << 31, ip - (1 << 32), ip).to(torch.int32).contiguous()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--host-n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cndpfwd_l3.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import torch
    from cndp_amd import native as N
    from cndp_amd import pktgen
    from cndp_amd.cfwd import alloc_cfwd_outputs, cfwd_host

    routes = pktgen.l3fwd_routes()
    fib = c3_fib(routes)
    kw = dict(in_lport=0, lports=LPORTS)
    if a.dry:
        fr = pktgen.packed_ipv4(min(a.n, 4096), routes=routes, device="cpu")
        ips = dst_addrs(fr).numpy().view(np.uint32)
        for mode, name in ((N.CNDP_CFWD_FWD, "fwd"), (N.CNDP_CFWD_L3FWD, "l3fwd")):
            r = cfwd_host(fr.slab.numpy().copy(), fr.n, mode, fib=fib, stride=64, **kw)
            print(f"dry: {name}: forward / echo = {r['stats'].tolist()}")
            if mode == N.CNDP_CFWD_L3FWD:
                assert np.array_equal(r["nh"], fib.lookup_bulk(ips))
                hit = r["nh"] != N.CNDP_CFWD_DEFAULT_NH
                print(f"dry: {int(hit.sum())} of {fr.n} addresses meet a route")
        fib.close()
        return 0
    if not torch.cuda.is_available():
        print("cndpfwd_bench: needs a GPU (no CPU fallback); --dry checks the set-up", file=sys.stderr)
        return 2

    from cndp_amd.classify import Classifier
    dev = torch.device("cuda:0")
    fr = pktgen.packed_ipv4(a.n, routes=routes, device=dev)
    cl = Classifier(0)
    out = alloc_cfwd_outputs(fr.n, dev)
    ips = dst_addrs(fr)
    nh = torch.empty(fr.n, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    stages = {
        "mac_swap": (lambda: cl.mac_swap(fr), fr.n * 128),
        "lookup": (lambda: fib.lookup_dev(ips.data_ptr(), nh.data_ptr(), fr.n, stream), fr.n * 12),
        "fwd": (lambda: cl.cndpfwd(fr, N.CNDP_CFWD_FWD, out=out, **kw), fr.n * (128 + 13)),
        "l3fwd": (lambda: cl.cndpfwd(fr, N.CNDP_CFWD_L3FWD, fib=fib, out=out, **kw), fr.n * (128 + 13)),
    }

    # one l3fwd call checked against the lookup and the host rule before anything is timed
    head = fr.slab[:4096 * 64].cpu().numpy().copy()
    stages["lookup"][0]()
    stages["l3fwd"][0]()
    torch.cuda.synchronize()
    assert torch.equal(out["nh"], nh), "cndp_gpu_cfwd and cndp_fib_lookup_dev disagree"
    want = cfwd_host(head, 4096, N.CNDP_CFWD_L3FWD, fib=fib, stride=64, **kw)
    assert np.array_equal(fr.slab[:4096 * 64].cpu().numpy(), head), "cndp_gpu_cfwd and cndp_cfwd_host disagree"
    assert np.array_equal(out["tx_lport"][:4096].cpu().numpy().view(np.uint16), want["tx_lport"])
    stats = out["stats"].cpu().numpy().tolist()
    hits = int((nh != N.CNDP_CFWD_DEFAULT_NH).sum())

    ms = {k: [] for k in stages}
    for k in range(a.warmup + a.iters):
        for name, (fn, _) in stages.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    t = {k: np.array(v) for k, v in ms.items()}

    res = {"n": fr.n, "routes": len(routes), "addresses_on_a_route": hits, "l3fwd_forward_echo_one_call": stats,
           "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS, "stages": {}, "ratios": {}}
    for name, (_, nbytes) in stages.items():
        med = float(np.median(t[name]))
        res["stages"][name] = {"ms": med, "ms_min": float(t[name].min()), "ms_max": float(t[name].max()), "bytes": nbytes,
                               "TBs": nbytes / (med * 1e-3) / 1e12, "Mpps": fr.n / (med * 1e-3) / 1e6}
        res["stages"][name]["share_of_achievable"] = res["stages"][name]["TBs"] / HBM_ACHIEVABLE_TBS
    for name, r in (("fwd_over_mac_swap", t["fwd"] / t["mac_swap"]), ("l3fwd_over_mac_swap", t["l3fwd"] / t["mac_swap"]),
                    ("l3fwd_over_fwd", t["l3fwd"] / t["fwd"]),
                    ("l3fwd_over_mac_swap_plus_lookup", t["l3fwd"] / (t["mac_swap"] + t["lookup"]))):
        res["ratios"][name] = {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())}
    # the host rule on one core over the head of the batch
    m = min(a.host_n, fr.n)
    for mode, name in ((N.CNDP_CFWD_FWD, "host_fwd"), (N.CNDP_CFWD_L3FWD, "host_l3fwd")):
        head = fr.slab[:m * 64].cpu().numpy().copy()
        cfwd_host(head, min(m, 4096), mode, fib=fib, stride=64, **kw)      # touch the code and the image once
        t0 = time.perf_counter()
        cfwd_host(head, m, mode, fib=fib, stride=64, **kw)
        dt = time.perf_counter() - t0
        res["stages"][name] = {"frames": m, "ms": dt * 1e3, "Mpps": m / dt / 1e6}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    cl.close()
    fib.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

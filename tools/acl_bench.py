#!/usr/bin/env python3
"""Measure cndpfwd's ACL stage (cndp_gpu_acl_fwd) with the default rule set on
the C3 batch (bench.py's 16M packed 64-byte IPv4/UDP frames).

    python tools/acl_bench.py [--n 16777216] [--out profiles/acl_fwd.json]

Two address mixes over the same slab:

  c3        the batch as bench.py builds it.  Few of its addresses meet a
            default rule, so nearly every frame walks all four groups and is
            denied (strict) -- the longest walk the default set has
  drawn     the same frames with src / dst rewritten on the device so that a
            quarter each is denied by dst, denied by src /8, denied by src /24
            and allowed (an early stop after 1, 2, 3 and 4 groups)

Per mix: the stage in strict mode without the swap (a read-only pass), with the
swap (forwarded frames written), and cndp_gpu_mac_swap on the same batch, which
reads and writes the same 12 bytes of every frame.  Timing uses device events:
--warmup calls, then the median (min-max) of --iters, each on an idle device.
The swap variants run on the slab the previous call left (a swap does not change
what the rule reads).  Beside them cndp_acl_classify_host on one core over the
first --host-n frames of the same mix.  Bytes are algorithmic: per frame one
64-byte line read, 8 bytes of outputs written (result, verdict, tx_lport,
bin_of) and, for a swapped frame, the line written back; image reads are not
counted (266 KiB, cache-resident).  --dry builds a small batch on the CPU and
checks both mixes against the host rule without timing.
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


def put_be32(view, col: int, val):
    for k in range(4):
        view[:, col + k] = ((val >> (24 - 8 * k)) & 0xFF).to(view.dtype)


def draw(fr):
    """Rewrite src / dst of every frame in place: i % 4 picks the rule kind."""
    import torch
    v = fr.slab.view(fr.n, 64)
    i = torch.arange(fr.n, dtype=torch.int64, device=fr.slab.device)
    kind, j = i % 4, i // 4
    lo = j & 0xFFF
    src = torch.where(kind == 1, (10 + j % 15) << 24 | (j & 0xFFFFFF),
                      torch.where(kind == 2, 101 << 24 | (j % 15) << 8 | (j & 0xFF),
                                  torch.where(kind == 3, 210 << 24 | lo, 198 << 24 | 18 << 16 | (j & 0xFFFF))))
    dst = torch.where(kind == 0, 100 << 24 | (j % 100) << 16 | (j & 0xFF), torch.where(kind == 3, 110 << 24 | lo,
                                                                                       192 << 24 | (j & 0xFFFF)))
    put_be32(v, 26, src)
    put_be32(v, 30, dst)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--host-n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acl_fwd.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import torch
    from cndp_amd import native as N
    from cndp_amd import pktgen
    from cndp_amd.acl import AclTable, alloc_acl_outputs

    acl = AclTable()
    acl.add_init_rules()
    acl.build()
    routes = pktgen.l3fwd_routes()
    kw = dict(in_lport=0, lports=(0, 1, 2, 3))
    if a.dry:
        fr = pktgen.packed_ipv4(min(a.n, 4096), routes=routes, device="cpu")
        for mix in ("c3", "drawn"):
            if mix == "drawn":
                draw(fr)
            r = acl.classify_host(fr.slab.numpy().copy(), fr.n, stride=64, **kw)
            print(f"dry: {mix}: prefilter / deny / permit = {r['stats'].tolist()}")
            if mix == "drawn":
                assert r["stats"].tolist() == [0, fr.n * 3 // 4, fr.n // 4], r["stats"]
        return 0
    if not torch.cuda.is_available():
        print("acl_bench: needs a GPU (no CPU fallback); --dry checks the set-up", file=sys.stderr)
        return 2

    from cndp_amd.classify import Classifier
    dev = torch.device("cuda:0")
    fr = pktgen.packed_ipv4(a.n, routes=routes, device=dev)
    cl = Classifier(0)
    out = alloc_acl_outputs(fr.n, dev)

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

    res = {"n": fr.n, "rules": acl.count(), "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS, "stages": {}}
    for mix in ("c3", "drawn"):
        if mix == "drawn":
            draw(fr)
        out["stats"].zero_()
        cl.acl_fwd(fr, acl, mode=N.CNDP_ACL_STRICT, swap=False, acl=out, **kw)
        torch.cuda.synchronize()
        stats = out["stats"].cpu().numpy().tolist()
        st = timed(lambda: cl.acl_fwd(fr, acl, mode=N.CNDP_ACL_STRICT, swap=False, acl=out, **kw))
        st.update(stats_one_call=stats, bytes=fr.n * (64 + 8))
        res["stages"][f"acl_fwd_{mix}"] = st
        st = timed(lambda: cl.acl_fwd(fr, acl, mode=N.CNDP_ACL_STRICT, swap=True, acl=out, **kw))
        st.update(bytes=fr.n * (64 + 8) + stats[2] * 64)
        res["stages"][f"acl_fwd_{mix}_swap"] = st
        # the host rule on one core over the head of the same mix
        m = min(a.host_n, fr.n)
        head = fr.slab[:m * 64].cpu().numpy().copy()
        acl.classify_host(head, min(m, 4096), stride=64, **kw)      # touch the image once
        t0 = time.perf_counter()
        acl.classify_host(head, m, stride=64, **kw)
        dt = time.perf_counter() - t0
        res["stages"][f"acl_host_{mix}"] = {"frames": m, "ms": dt * 1e3, "Mpps": m / dt / 1e6}
    st = timed(lambda: cl.mac_swap(fr))
    st.update(bytes=fr.n * 128)
    res["stages"]["mac_swap"] = st
    for st in res["stages"].values():
        if "bytes" in st:
            st["TBs"] = st["bytes"] / (st["ms"] * 1e-3) / 1e12
            st["share_of_achievable"] = st["TBs"] / HBM_ACHIEVABLE_TBS
            st["Mpps"] = fr.n / (st["ms"] * 1e-3) / 1e6
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    acl.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Measure the UDP transmit stage (cndp_gpu_ip4_output, CNDP_TX_UDP) on the C4
IMIX batch's slots used as transmit buffers.

    python tools/udp_output_bench.py [--n 16777216] [--out profiles/udp_output.json]

The buffers are bench.py's C4 slots (pktgen.imix: 64 / 576 / 1536 bytes at
7:4:1, packed); every buffer carries a payload of slot - 42 bytes at data offset
42, so the 42 bytes of headers fill the start of the slot.  1024 PCBs on eight
local addresses, each routed to a netif of its own; every destination has an ARP
entry, so every frame is sent.  Odd PCBs have UDP_CHKSUM_FLAG; three runs differ
only in the PCB each frame names:

  cksum_all    every datagram checksummed: the payload is read once
  cksum_none   none: the stage writes headers and never reads a payload
  cksum_64     only the frames in 64-byte slots (22-byte payloads)

Timing uses device events: --warmup calls, then the median (min-max) of --iters,
each on an idle device, per launch set (the call's four kernels).  Every timed
call works on the slab the previous one left; nothing the stage computes depends
on those bytes but the checksummed payloads, which no call changes.  Bytes are
algorithmic: per frame the five inputs (18 B) and two outputs (4 B); per sent
frame the 128-byte line its 42-byte header write touches; per checksummed frame
its UDP bytes read once (the header among them).  Tables and the two scratch
bytes per frame are not counted.  Beside them, from the same run: the same-box
rate of cndp_amd/csrc/roofline_probe.hip streaming the slab as 64-byte slots,
and cndp_tx_output_host on one core over the first --cpu-n frames.  The tool
asserts nothing about speed.  --dry builds a small batch on the CPU and checks
the set-up through cndp_tx_output_host without timing.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE_TBS = 6.29   # MI355X achievable HBM rate the project's figures are held against
NETIFS, PCBS, HEAD = 8, 1024, 42


def tables():
    """(arp Fib, rt4 Fib, FwdTable, PcbTable): local 10.k.0.7 routed to netif k, 10.200/16 known to ARP."""
    from cndp_amd import native as N
    from cndp_amd.fib import Fib
    from cndp_amd.fwd import FwdTable
    from cndp_amd.l4 import PcbTable
    mk = lambda name: Fib(name, N.CNE_FIB_DIR24_8, default_nh=65, max_routes=256,  # noqa: E731
                          nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=64)
    arp, rt4 = mk("arp-fib"), mk("rt4-fib")
    fwd = FwdTable(arp, rt4, 64, 64)
    for k in range(NETIFS):
        assert fwd.netif_set(k, bytes([2, 0x10, 0, 0, 0, k])) == 0
        assert fwd.rt_set(k + 1, 0, k) == 0 and rt4.add(0x0A000000 | k << 16, 16, k + 1) == 0
    assert fwd.arp_set(1, 0, bytes([2, 0xAA, 0, 0, 0, 1])) == 0 and arp.add(0x0AC80000, 16, 1) == 0
    pcbs = PcbTable(PCBS)
    for i in range(PCBS):
        assert pcbs.add(laddr=0x0A000007 | (i // 2 % NETIFS) << 16, lport=1024 + i, cksum=bool(i & 1)) == i
    return arp, rt4, fwd, pcbs


def batch_inputs(slot: np.ndarray, seed: int = 7):
    """Per-frame inputs for slots of `slot` bytes: (pcb per run, faddr, laddr, ports, length)."""
    from cndp_amd.l4 import addr_net, port_net
    n = len(slot)
    rng = np.random.default_rng(seed)
    sock = rng.integers(0, PCBS // 2, n).astype(np.uint32) * 2      # an even PCB: no checksum; + 1: checksum
    runs = {"cksum_all": sock + 1, "cksum_none": sock, "cksum_64": sock + (slot == 64)}
    laddr_k = np.array([addr_net(0x0A000007 | k << 16) for k in range(NETIFS)], np.uint32)
    lport = np.array([port_net(1024 + i) for i in range(PCBS)], np.uint32)
    faddr = np.array([addr_net(0x0AC80000 | int(x)) for x in rng.integers(1, 1 << 16, 4096)], np.uint32)
    faddr = faddr[rng.integers(0, 4096, n)]
    length = (slot - HEAD).astype(np.uint16)
    per_run = {}
    for name, pcb in runs.items():
        pcb = pcb.astype(np.uint32)
        per_run[name] = (pcb, laddr_k[pcb // 2 % NETIFS], (np.uint32(port_net(9)) | lport[pcb] << 16).astype(np.uint32))
    return per_run, faddr, length


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "udp_output.json"))
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    import torch
    from cndp_amd import pktgen
    from cndp_amd import tx as T

    arp, rt4, fwd, pcbs = tables()
    if a.dry:
        fr = pktgen.imix(min(a.n, 4096), device="cpu")
        offs = fr.offsets.numpy()
        slot = np.diff(np.append(offs, fr.slab.numel()))
        per_run, faddr, length = batch_inputs(slot)
        for name, (pcb, laddr, ports) in per_run.items():
            slab = fr.slab.numpy().copy()
            got = T.output_host(fwd, pcbs, slab, fr.n, pcb, faddr, laddr, ports, length, offsets=offs, data_off=HEAD,
                                n_bins=NETIFS)
            st = got["stats"].tolist()
            want_ck = {"cksum_all": fr.n, "cksum_none": 0, "cksum_64": int((slot == 64).sum())}[name]
            assert st[0] == fr.n and st[5] == want_ck and sorted(set(got["bin_of"].tolist())) == list(range(NETIFS)), st
            print(f"dry: {name}: {st[0]} of {fr.n} sent on {NETIFS} netifs, {st[5]} checksummed")
        return 0
    if not torch.cuda.is_available():
        print("udp_output_bench: needs a GPU (no CPU fallback); --dry checks the set-up", file=sys.stderr)
        return 2

    from cndp_amd.classify import Classifier
    dev = torch.device("cuda:0")
    fr = pktgen.imix(a.n, device=dev)
    fr.data_off = HEAD
    n = fr.n
    offs = fr.offsets.cpu().numpy()
    slot = np.diff(np.append(offs, fr.slab.numel()))
    per_run, faddr, length = batch_inputs(slot)
    cl = Classifier(0)
    tx = T.alloc_tx_outputs(n, dev)
    d32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.uint32).view(np.int32)).to(dev)  # noqa: E731
    faddr_t, len_t = d32(faddr), torch.from_numpy(length.view(np.int16)).to(dev)

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

    res = {"n": n, "slab_bytes": int(fr.slab.numel()), "netifs": NETIFS, "pcbs": PCBS, "iters": a.iters,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS,
           "stages": {}}
    for name, (pcb, laddr, ports) in per_run.items():
        args = (d32(pcb), faddr_t, d32(laddr), d32(ports), len_t)
        tx["stats"].zero_()
        cl.ip4_output(fr, fwd, pcbs, *args, n_bins=NETIFS, tx=tx)
        torch.cuda.synchronize()
        stats = tx["stats"].cpu().numpy().tolist()
        st = timed(lambda: cl.ip4_output(fr, fwd, pcbs, *args, n_bins=NETIFS, tx=tx))
        ck = (pcb & 1).astype(bool)
        st.update(stats_one_call=stats, frames_checksummed=int(ck.sum()),
                  bytes=int(n * (18 + 4) + stats[0] * 128 + (length[ck].astype(np.int64) + 8).sum()))
        res["stages"][name] = st
    for st in res["stages"].values():
        st["TBs"] = st["bytes"] / (st["ms"] * 1e-3) / 1e12
        st["share_of_achievable"] = st["TBs"] / HBM_ACHIEVABLE_TBS
        st["Gpps"] = n / (st["ms"] * 1e-3) / 1e9

    # the same box streaming the same slab (roofline_probe.hip: 64-byte slots read, 4 B a slot stored)
    try:
        P = ctypes.CDLL(os.path.join(ROOT, "cndp_amd", "lib", "libcndp_probe.so"))
        P.cndp_probe_slots.argtypes = [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 3 + \
            [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        slots = fr.slab.numel() // 64
        o = torch.empty(slots, dtype=torch.int32, device=dev)
        sid = torch.cuda.current_stream(dev).cuda_stream
        pr = timed(lambda: P.cndp_probe_slots(fr.slab.data_ptr(), slots, o.data_ptr(), None, None, 2, 4, sid))
        pr["bytes"] = slots * 68
        pr["TBs"] = pr["bytes"] / (pr["ms"] * 1e-3) / 1e12
        res["probe_slab_stream"] = pr
        for st in res["stages"].values():
            st["share_of_probe_rate"] = st["TBs"] / pr["TBs"]
    except Exception as ex:     # the probe library is optional for this tool
        res["probe_slab_stream"] = {"error": repr(ex)}

    # one core, the same rule over the first cpu_n frames (checksum on for all / for none)
    m = min(a.cpu_n, n)
    end = int(offs[m]) if m < n else int(fr.slab.numel())
    host_slab = fr.slab[:end].cpu().numpy()
    res["cpu_one_core"] = {}
    for name in ("cksum_all", "cksum_none"):
        pcb, laddr, ports = per_run[name]
        t0 = time.perf_counter()
        T.output_host(fwd, pcbs, host_slab, m, pcb[:m], faddr[:m], laddr[:m], ports[:m], length[:m], offsets=offs[:m],
                      data_off=HEAD, n_bins=NETIFS)
        dt = time.perf_counter() - t0
        res["cpu_one_core"][name] = {"frames": m, "ms": dt * 1e3, "Mpps": m / dt / 1e6}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

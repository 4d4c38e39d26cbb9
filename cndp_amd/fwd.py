"""ip4_forward (include/cndp_fwd.h): the forwarding table the node resolves
frames in -- cnet's ARP and route FIBs, the objects behind them and the netif
MACs -- and the output arrays of Classifier.ip4_forward.

    arp = Fib("arp-fib", default_nh=ARP_N + 1, max_routes=ARP_N)     # as cnet_arp.c creates it
    rt4 = Fib("rt4-fib", default_nh=RT_N + 1, max_routes=RT_N)
    tbl = FwdTable(arp, rt4, ARP_N, RT_N)
    tbl.netif_set(0, "02:00:00:00:00:10")
    tbl.arp_set(3, netif_idx=0, ha="02:aa:bb:cc:dd:03"); arp.add(key, 32, 3)
    tbl.rt_set(1, gateway=gw_s_addr, netif_idx=0);       rt4.add(prefix, 24, 1)
    out = c.classify(frames, CNDP_MODE_CNET, out=c.alloc_outputs(n, meta=True))
    fwd = c.ip4_forward(frames, out, tbl, burst=256)     # slab rewritten in place
    start, order = c.bin_partition(fwd["bin_of"], fwd["n_bins"])     # per-netif transmit lists

Destination addresses are the u32 a little-endian host loads from the frame
(cndp_amd.l4.addr_net); a route's gateway is its s_addr as the stack stores
it, which the node hands to the ARP FIB unswapped.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native as N

# struct cndp_fwd_result
RESULT_DT = np.dtype([("edge", "<u2"), ("s_addr", "u1", 6), ("d_addr", "u1", 6)])


def mac_bytes(mac) -> bytes:
    """A MAC as 6 bytes, from bytes or "02:00:00:00:00:01"."""
    if isinstance(mac, str):
        mac = bytes(int(x, 16) for x in mac.split(":"))
    mac = bytes(mac)
    if len(mac) != 6:
        raise ValueError("a MAC address has 6 bytes")
    return mac


class FwdTable:
    """cndp_fwd_* (include/cndp_fwd.h).  Keeps the two Fib objects alive."""

    def __init__(self, arp_fib, rt4_fib, arp_objs: int, rt_objs: int):
        self._L = N.lib()
        h = ctypes.c_void_p()
        N.check(self._L.cndp_fwd_create(arp_fib.h, rt4_fib.h, arp_objs, rt_objs, ctypes.byref(h)),
                "cndp_fwd_create")
        self.h = h
        self.arp_fib, self.rt4_fib = arp_fib, rt4_fib

    def close(self):
        if self.h:
            self._L.cndp_fwd_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def arp_set(self, idx: int, netif_idx: int, ha) -> int:
        """cndp_fwd_arp_set; returns its result (0 or -errno)."""
        if not 0 <= netif_idx <= 0xFFFF:
            return -22
        e = N.FwdArp(netif_idx, (ctypes.c_uint8 * 6)(*mac_bytes(ha)))
        return self._L.cndp_fwd_arp_set(self.h, idx, ctypes.byref(e))

    def arp_clear(self, idx: int) -> int:
        return self._L.cndp_fwd_arp_clear(self.h, idx)

    def rt_set(self, idx: int, gateway: int, netif_idx: int) -> int:
        """cndp_fwd_rt_set; gateway is s_addr as stored.  Returns 0 or -errno."""
        if not 0 <= netif_idx <= 0xFFFF:
            return -22
        e = N.FwdRt(gateway & 0xFFFFFFFF, netif_idx)
        return self._L.cndp_fwd_rt_set(self.h, idx, ctypes.byref(e))

    def rt_clear(self, idx: int) -> int:
        return self._L.cndp_fwd_rt_clear(self.h, idx)

    def netif_set(self, idx: int, mac) -> int:
        """cndp_fwd_netif_set; mac None = unset (six zero bytes)."""
        buf = ctypes.create_string_buffer(mac_bytes(mac), 6) if mac is not None else None
        return self._L.cndp_fwd_netif_set(self.h, idx, buf)

    def max_netif(self) -> int:
        r = self._L.cndp_fwd_max_netif(self.h)
        return r if r == -1 else N.check(r, "cndp_fwd_max_netif")

    def lookup(self, dst_be) -> np.ndarray:
        """cndp_fwd_lookup: RESULT_DT records for destination addresses as a
        little-endian host loads them from the frame."""
        dst = np.ascontiguousarray(dst_be, dtype=np.uint32)
        out = np.zeros(len(dst), RESULT_DT)
        N.check(self._L.cndp_fwd_lookup(self.h, dst.ctypes.data, len(dst), out.ctypes.data), "cndp_fwd_lookup")
        return out


def node_host(tbl: FwdTable, ptrs, n: int | None = None, readable_end=None) -> np.ndarray:
    """cndp_fwd_node_host (include/cndp_mqcnet.h): the ip4_forward node on the
    calling thread over one burst of n <= 256 mbufs (a ctypes array of
    pktmbuf_t addresses as MbufPool.ptrs gives it, or its address), the frames
    and the mbufs' data_off / data_len edited in place.  readable_end: the
    address at which the mbufs' region ends, None for each mbuf's own
    buf_addr + buf_len.  Returns the edges, CNDP_MQ_EDGE_FWD_GATEWAY included."""
    n = len(ptrs) if n is None else n
    edges = np.zeros(max(n, 1), np.uint16)
    N.check(N.lib().cndp_fwd_node_host(tbl.h, ptrs, n, edges.ctypes.data, readable_end), "cndp_fwd_node_host")
    return edges[:n]


def alloc_fwd_outputs(n: int, device) -> dict:
    """The output arrays of cndp_gpu_ip4_forward as torch tensors (signed
    dtypes of the same width, as Classifier.alloc_outputs uses)."""
    import torch
    m = max(n, 1)
    return {"fwd_edge": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "arp_idx": torch.empty(m, dtype=torch.int32, device=device)[:n],
            "bin_of": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "stats": torch.zeros(3, dtype=torch.int64, device=device)}

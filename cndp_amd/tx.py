"""UDP transmit (include/cndp_tx.h): udp_output + ip4_output over a batch of
transmit buffers, the PCB transmit attributes and the netifs' identification
counters, and the output arrays of Classifier.ip4_output.

    pcbs = PcbTable(512); i = pcbs.add(laddr="10.4.0.7", lport=5000, cksum=True)
    pcb_tx_set(pcbs, i, ttl=32)                              # tos 0 / ttl 64 / proto 17 by default
    fwd = FwdTable(arp, rt4, ARP_N, RT_N)                    # a route to 10.4.0.7 names the netif
    tx = c.ip4_output(frames, fwd, pcbs, pcb, faddr, laddr, ports, length)   # headers written in place
    start, order = c.bin_partition(tx["bin_of"], tx["n_bins"])               # per-netif transmit lists

`frames` gives the buffers (stride / offsets) and the headroom (data_off): the
payload of frame i starts data_off bytes into its buffer and a sent frame
starts 42 bytes earlier (34 in CNDP_TX_IP4 mode).  pcb, faddr, laddr, ports and
length are what udp_input returned or the application filled in: addresses as a
little-endian host loads them from a frame, ports as fport | lport << 16.

The functions on tables are free functions so PcbTable and FwdTable stay as
they are.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native as N

# the resolve / write kernels' launch geometry (cndp_amd/csrc/cndp_tx.hip): a
# batch of more than multiprocessors * TX_BLOCKS_PER_CU * TX_BLOCK frames gives
# every block more than one pass
TX_BLOCK = 256
TX_BLOCKS_PER_CU = 3


def pcb_tx_set(table, idx: int, tos: int = 0, ttl: int = 64, ip_proto: int = 17) -> int:
    """cndp_pcb_tx_set; returns its result (0 or -errno)."""
    a = N.PcbTx(tos, ttl, ip_proto)
    return N.lib().cndp_pcb_tx_set(table.h, idx, ctypes.byref(a))


def pcb_tx_get(table, idx: int):
    """cndp_pcb_tx_get -> (tos, ttl, ip_proto), or the negative errno."""
    a = N.PcbTx()
    r = N.lib().cndp_pcb_tx_get(table.h, idx, ctypes.byref(a))
    return (a.tos, a.ttl, a.ip_proto) if r == 0 else r


def ident_set(table, netif: int, ident: int) -> int:
    """cndp_fwd_netif_ident_set; returns its result (0 or -errno)."""
    return N.lib().cndp_fwd_netif_ident_set(table.h, netif, ident & 0xFFFF)


def ident_get(table, netif: int) -> int:
    """cndp_fwd_netif_ident_get: the netif's ip_ident after the table's last call."""
    v = ctypes.c_uint16()
    N.check(N.lib().cndp_fwd_netif_ident_get(table.h, netif, ctypes.byref(v)), "cndp_fwd_netif_ident_get")
    return v.value


def alloc_tx_outputs(n: int, device) -> dict:
    """The output arrays of cndp_gpu_ip4_output as torch tensors (signed dtypes
    of the same width, as Classifier.alloc_outputs uses)."""
    import torch
    m = max(n, 1)
    return {"tx_edge": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "bin_of": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "stats": torch.zeros(N.CNDP_TX_NSTATS, dtype=torch.int64, device=device)}


def output_host(fwd_table, pcb_table, slab: np.ndarray, n: int, pcb, faddr, laddr, ports, length,
                mode: int = N.CNDP_TX_UDP, stride: int = 0, offsets=None, data_off: int = 0, sel=None,
                n_bins: int | None = None, slab_len: int | None = None, stats=None) -> dict:
    """cndp_tx_output_host: the same rule on the calling thread.  `slab` (a
    contiguous numpy uint8 array) is rewritten in place, bounded by slab_len;
    returns tx_edge, bin_of and stats as numpy arrays."""
    assert slab.dtype == np.uint8 and slab.flags.c_contiguous
    keep = [np.ascontiguousarray(pcb, np.uint32), np.ascontiguousarray(faddr, np.uint32),
            np.ascontiguousarray(laddr, np.uint32), np.ascontiguousarray(length, np.uint16)]
    io = N.TxIo()
    io.pcb, io.faddr, io.laddr, io.len = (a.ctypes.data for a in keep)
    if ports is not None:
        keep.append(np.ascontiguousarray(ports, np.uint32))
        io.ports = keep[-1].ctypes.data
    if sel is not None:
        keep.append(np.ascontiguousarray(sel, np.uint8))
        io.sel = keep[-1].ctypes.data
    offs = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
    if n_bins is None:
        n_bins = max(1, fwd_table.max_netif() + 1)
    out = {"tx_edge": np.empty(max(n, 1), np.uint16)[:n], "bin_of": np.empty(max(n, 1), np.uint16)[:n],
           "stats": np.zeros(N.CNDP_TX_NSTATS, np.uint64) if stats is None else np.array(stats, np.uint64)}
    io.tx_edge, io.bin_of, io.n_bins, io.stats = (out["tx_edge"].ctypes.data, out["bin_of"].ctypes.data, n_bins,
                                                  out["stats"].ctypes.data)
    N.check(N.lib().cndp_tx_output_host(fwd_table.h, pcb_table.h, mode, slab.ctypes.data,
                                        len(slab) if slab_len is None else slab_len, stride,
                                        None if offs is None else offs.ctypes.data, data_off, n, ctypes.byref(io)),
            "cndp_tx_output_host")
    out["n_bins"] = n_bins
    return out


def ip4_output_node_host(fwd_table, pcb_table, ptrs, n: int | None = None, tx_mode: int = N.CNDP_TX_UDP,
                         readable_end: int = 0, stage_max: int = 0, metadata=None) -> np.ndarray:
    """cndp_ip4_output_node_host (include/cndp_mqtx.h): udp_output + ip4_output on
    the calling thread over one burst of mbuf pointers (a ctypes array, as
    MbufPool.ptrs returns); the mbufs and their frames are rewritten in place.
    metadata: a Python function of the mbuf address returning the metadata
    address (None: m + 64).  Returns the edges."""
    n = len(ptrs) if n is None else n
    edges = np.zeros(max(n, 1), np.uint16)[:n]
    fn = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p)(metadata) if metadata else None
    N.check(N.lib().cndp_ip4_output_node_host(fwd_table.h, pcb_table.h, tx_mode, ptrs, n, edges.ctypes.data,
                                              readable_end or None, stage_max,
                                              ctypes.cast(fn, ctypes.c_void_p) if fn else None),
            "cndp_ip4_output_node_host")
    return edges

"""UDP and TCP socket demux (include/cndp_l4.h, include/cndp_tcp.h,
include/cndp_tcb.h): the PCB table udp_input / tcp_input look frames up in, the
TCB table tcp_segment reads, and the output arrays of Classifier.udp_input,
Classifier.tcp_input and Classifier.tcp_segment.

    tbl = PcbTable(512)
    i = tbl.add(laddr="10.4.0.7", lport=5000, cksum=True)    # a bound listener
    out = c.classify(frames, CNDP_MODE_CNET, out=c.alloc_outputs(n, meta=True))
    l4 = c.udp_input(frames, out, tbl)                       # l4edge, pcb, bin_of, ...
    start, order = c.bin_partition(l4["bin_of"], l4["n_bins"])   # per-socket receive lists

The TCP vector is a second table; its frames are the ones udp_input left on
ip4_proto's tcp edge:

    tcp = PcbTable(4096)
    tcp.add(laddr="10.4.0.7", lport=80)                      # a listener
    tcp.add(laddr="10.4.0.7", lport=80, faddr="198.18.0.1", fport=40000)   # a connection
    tbl.set_flags(tcp_enabled=True)
    l4 = c.udp_input(frames, out, tbl)
    t = c.tcp_input(frames, out, tcp, l4=l4)                 # l4edge (in place), pcb, seg, bin_of, ...

Behind it, option parsing and the header-prediction triage (include/cndp_tcb.h)
against the connections' TCB snapshots, kept in a TcbTable beside the TCP table:

    tcbs = TcbTable(tcp)
    tcbs.set(1, state=N.CNDP_TCPS_ESTABLISHED, rcv_nxt=..., snd_una=..., ...)
    s = c.tcp_segment(frames, out, tcbs, t, now=ticks)       # opt, verdict, stats

The transmit side of those connections (include/cndp_tcpout.h): per-TCB transmit
attributes and, on the calling thread, the rule that builds options, header and
payload in front of ip4_output's CNDP_TX_IP4 mode:

    tcbs.tx_set(1, tflags=N.CNDP_TCBF_REQ_TSTAMP | N.CNDP_TCBF_RCVD_TSTAMP, rcv_scale=7)
    o = tcbs.output_host(slab, n, pcb, now=ticks, txseg=descs, snd=sendbuf, src_off=offs, stride=2048, data_off=64)

Addresses and ports are kept in network order, as the u32 / u16 a
little-endian host loads from the frame; add() and lookup keys take host
integers or dotted quads and convert.
"""
from __future__ import annotations

import ctypes
import socket
import struct

import numpy as np

from . import native as N

# struct cndp_pcb_key
KEY_DT = np.dtype([("laddr", "<u4"), ("faddr", "<u4"), ("lport", "<u2"), ("fport", "<u2")])
# struct cndp_tcp_seg
SEG_DT = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("wnd", "<u2"), ("urp", "<u2"), ("len", "<u2"),
                   ("flags", "u1"), ("offset", "u1")])


def addr_net(a) -> int:
    """An IPv4 address (dotted quad, or a host-order integer such as
    0x0A000001) as the u32 a little-endian load of its wire bytes gives."""
    if isinstance(a, str):
        return struct.unpack("<I", socket.inet_aton(a))[0]
    return struct.unpack("<I", struct.pack(">I", int(a) & 0xFFFFFFFF))[0]


def port_net(p: int) -> int:
    """A port number as the u16 a little-endian load of its wire bytes gives."""
    return struct.unpack("<H", struct.pack(">H", int(p) & 0xFFFF))[0]


def make_keys(laddr, lport, faddr, fport) -> np.ndarray:
    """Lookup keys from arrays already in network order."""
    k = np.zeros(len(np.atleast_1d(lport)), KEY_DT)
    k["laddr"], k["lport"], k["faddr"], k["fport"] = laddr, lport, faddr, fport
    return k


class PcbTable:
    """cndp_pcb_* (include/cndp_l4.h): the stack's UDP PCB vector."""

    def __init__(self, max_entries: int = 512):
        self._L = N.lib()
        h = ctypes.c_void_p()
        N.check(self._L.cndp_pcb_create(max_entries, ctypes.byref(h)), "cndp_pcb_create")
        self.h = h

    def close(self):
        if self.h:
            self._L.cndp_pcb_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_raw(self, laddr: int, faddr: int, lport: int, fport: int, opt_flag: int = 0) -> int:
        """cndp_pcb_add on network-order values; returns its result (index or -errno)."""
        e = N.PcbEntry(laddr, faddr, lport, fport, opt_flag)
        return self._L.cndp_pcb_add(self.h, ctypes.byref(e))

    def add(self, laddr=0, lport: int = 0, faddr=0, fport: int = 0, cksum: bool = False) -> int:
        """A socket bound to laddr:lport (0 = any), optionally connected to
        faddr:fport; cksum sets UDP_CHKSUM_FLAG.  Returns the PCB index."""
        return N.check(self.add_raw(addr_net(laddr), addr_net(faddr), port_net(lport), port_net(fport),
                                    N.CNDP_UDP_CHKSUM_FLAG if cksum else 0), "cndp_pcb_add")

    def delete(self, idx: int) -> int:
        """cndp_pcb_del; returns its result (0 or -errno)."""
        return self._L.cndp_pcb_del(self.h, idx)

    def set_flags(self, punt_enabled: bool = True, tcp_enabled: bool = False) -> None:
        N.check(self._L.cndp_pcb_set_flags(self.h, int(punt_enabled), int(tcp_enabled)), "cndp_pcb_set_flags")

    def count(self) -> int:
        return N.check(self._L.cndp_pcb_count(self.h), "cndp_pcb_count")

    def lookup(self, keys: np.ndarray) -> np.ndarray:
        """cndp_pcb_lookup over a KEY_DT array (make_keys): u32 indices,
        CNDP_PCB_NONE for no match."""
        keys = np.ascontiguousarray(keys, dtype=KEY_DT)
        out = np.empty(len(keys), np.uint32)
        N.check(self._L.cndp_pcb_lookup(self.h, keys.ctypes.data, len(keys), out.ctypes.data),
                "cndp_pcb_lookup")
        return out

    def lookup_indexed(self, keys: np.ndarray) -> np.ndarray:
        """cndp_pcb_lookup_indexed: lookup()'s results, answered from the
        table's TCP index (exact 4-tuple hash + per-port wildcard runs)."""
        keys = np.ascontiguousarray(keys, dtype=KEY_DT)
        out = np.empty(len(keys), np.uint32)
        N.check(self._L.cndp_pcb_lookup_indexed(self.h, keys.ctypes.data, len(keys), out.ctypes.data),
                "cndp_pcb_lookup_indexed")
        return out

    def user_set(self, idx: int, user: int) -> int:
        """cndp_pcb_user_set (include/cndp_mql4.h): the value the udp_input node
        stores in m->userptr for this PCB; returns its result (0 or -errno)."""
        return self._L.cndp_pcb_user_set(self.h, idx, user & 0xFFFFFFFFFFFFFFFF)

    def user_get(self, idx: int) -> int:
        """cndp_pcb_user_get: the PCB's user value (its index unless one was set)."""
        v = ctypes.c_uint64()
        N.check(self._L.cndp_pcb_user_get(self.h, idx, ctypes.byref(v)), "cndp_pcb_user_get")
        return int(v.value)


METADATA_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p)


def udp_input_node_host(tbl: PcbTable, ptrs, n: int | None = None, readable_end=None, stage_max: int = 0,
                        metadata=None) -> np.ndarray:
    """cndp_udp_input_node_host (include/cndp_mql4.h): ip4_proto + udp_input on
    the calling thread over one burst of n <= 256 mbufs (a ctypes array of
    pktmbuf_t addresses as MbufPool.ptrs gives it, or its address), the mbufs'
    userptr / data_off / data_len and their metadata edited in place.
    readable_end: the address at which the mbufs' region ends (None: no region);
    stage_max: the staged queue's clip (0: none); metadata: pktmbuf_metadata as
    a Python function of the mbuf address (None: m + 64).  Returns the edges."""
    n = len(ptrs) if n is None else n
    edges = np.zeros(max(n, 1), np.uint16)
    fn = METADATA_FN(metadata) if metadata else None
    N.check(N.lib().cndp_udp_input_node_host(tbl.h, ptrs, n, edges.ctypes.data, readable_end, stage_max,
                                             ctypes.cast(fn, ctypes.c_void_p) if fn else None),
            "cndp_udp_input_node_host")
    return edges[:n]


def tcp_input_node_host(tbl: PcbTable, ptrs, n: int | None = None, readable_end=None, stage_max: int = 0,
                        metadata=None):
    """cndp_tcp_input_node_host (include/cndp_mqtcp.h): tcp_input and the
    opening of cnet_tcp_input on the calling thread over one burst of n <= 256
    mbufs, the mbufs' userptr / data_off / data_len and their metadata edited
    in place.  Arguments as udp_input_node_host.  Returns (edges, segs), segs
    a SEG_DT record array."""
    n = len(ptrs) if n is None else n
    edges = np.zeros(max(n, 1), np.uint16)
    segs = np.zeros(max(n, 1), SEG_DT)
    fn = METADATA_FN(metadata) if metadata else None
    N.check(N.lib().cndp_tcp_input_node_host(tbl.h, ptrs, n, edges.ctypes.data, segs.ctypes.data, readable_end,
                                             stage_max, ctypes.cast(fn, ctypes.c_void_p) if fn else None),
            "cndp_tcp_input_node_host")
    return edges[:n], segs[:n]


def alloc_l4_outputs(n: int, device) -> dict:
    """The output arrays of cndp_gpu_udp_input as torch tensors (signed
    dtypes of the same width, as Classifier.alloc_outputs uses)."""
    import torch
    m = max(n, 1)
    return {"l4edge": torch.empty(m, dtype=torch.uint8, device=device)[:n],
            "pcb": torch.empty(m, dtype=torch.int32, device=device)[:n],
            "ports": torch.empty(m, dtype=torch.int32, device=device)[:n],
            "payload_off": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "bin_of": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "stats": torch.zeros(4, dtype=torch.int64, device=device)}


def alloc_tcp_outputs(n: int, device, l4edge=None) -> dict:
    """The output arrays of cndp_gpu_tcp_input as torch tensors.  seg is an
    (n, 4) int32 tensor, one 16-byte struct cndp_tcp_seg per row
    (seg_records() views it as SEG_DT).  l4edge: udp_input's tensor, to be
    updated in place; otherwise (for a call with `sel`) a fresh one holding
    CNDP_L4_EDGE_NONE, which is what a frame the stage does not take keeps."""
    import torch
    m = max(n, 1)
    return {"l4edge": l4edge if l4edge is not None else torch.full((m,), N.CNDP_L4_EDGE_NONE, dtype=torch.uint8,
                                                                    device=device)[:n],
            "pcb": torch.empty(m, dtype=torch.int32, device=device)[:n],
            "ports": torch.empty(m, dtype=torch.int32, device=device)[:n],
            "seg": torch.empty((m, 4), dtype=torch.int32, device=device)[:n],
            "bin_of": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "stats": torch.zeros(N.CNDP_TCP_NSTATS, dtype=torch.int64, device=device)}


def seg_records(seg) -> np.ndarray:
    """The seg tensor of Classifier.tcp_input on the host, as SEG_DT records."""
    return np.ascontiguousarray(seg.cpu().numpy()).view(SEG_DT).reshape(-1)


# ---------------------------------------------------------------------------
# TCP option parse and header-prediction triage (include/cndp_tcb.h)
# ---------------------------------------------------------------------------
# struct cndp_tcp_opt
OPT_DT = np.dtype([("ts_val", "<u4"), ("ts_ecr", "<u4"), ("wnd", "<u4"), ("mss", "<u2"), ("sflags", "<u2")])


def tcp_segment_node_host(tbl: "PcbTable", tcbs: "TcbTable", ptrs, n: int | None = None, now: int = 0,
                          readable_end=None, stage_max: int = 0, metadata=None):
    """cndp_tcp_segment_node_host (include/cndp_mqtcb.h): the mbuf queue's
    CNDP_MQ_TCP_SEGMENT mode on the calling thread over one batch of n <= 256
    mbufs, edited in place as tcp_input_node_host edits them.  Returns
    (edges, segs, opts, verdicts): SEG_DT and OPT_DT record arrays, uint8."""
    n = len(ptrs) if n is None else n
    edges = np.zeros(max(n, 1), np.uint16)
    segs = np.zeros(max(n, 1), SEG_DT)
    opts = np.zeros(max(n, 1), OPT_DT)
    verdicts = np.zeros(max(n, 1), np.uint8)
    fn = METADATA_FN(metadata) if metadata else None
    N.check(N.lib().cndp_tcp_segment_node_host(tbl.h, tcbs.h, now & 0xFFFFFFFF, ptrs, n, edges.ctypes.data,
                                               segs.ctypes.data, opts.ctypes.data, verdicts.ctypes.data,
                                               readable_end, stage_max,
                                               ctypes.cast(fn, ctypes.c_void_p) if fn else None),
            "cndp_tcp_segment_node_host")
    return edges[:n], segs[:n], opts[:n], verdicts[:n]
# struct cndp_tcp_txseg
TXSEG_DT = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("wnd", "<u2"), ("urp", "<u2"), ("len", "<u2"),
                     ("flags", "u1"), ("rsvd", "u1")])
TCB_TX_FIELDS = ("tflags", "req_recv_scale", "rcv_scale")
TCB_FIELDS = ("rcv_nxt", "snd_una", "snd_nxt", "snd_max", "snd_wnd", "snd_cwnd", "ts_recent", "last_ack_sent",
              "rcv_space", "max_mss", "state", "snd_scale", "flags")


class TcbTable:
    """cndp_tcb_* (include/cndp_tcb.h): the per-PCB snapshot of the connection
    variables tcp_do_options and the header-prediction tests read, beside the
    PcbTable that holds the TCP vector (which must stay open while this is).

        tcbs = TcbTable(tcp)
        tcbs.set(i, state=N.CNDP_TCPS_ESTABLISHED, rcv_nxt=..., snd_una=..., ...)
        t = c.tcp_input(frames, out, tcp, l4=l4)
        s = c.tcp_segment(frames, out, tcbs, t, now=ticks)        # opt, verdict, stats
    """

    def __init__(self, pcb_table: PcbTable):
        self._L = N.lib()
        self.pcb_table = pcb_table
        h = ctypes.c_void_p()
        N.check(self._L.cndp_tcb_tbl_create(pcb_table.h, ctypes.byref(h)), "cndp_tcb_tbl_create")
        self.h = h

    def close(self):
        if self.h:
            self._L.cndp_tcb_tbl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_raw(self, idx: int, **fields) -> int:
        """cndp_tcb_set; returns its result (0 or -errno).  Fields not given are 0."""
        t = N.Tcb()
        for k, v in fields.items():
            if k not in TCB_FIELDS:
                raise TypeError(f"struct cndp_tcb has no field {k!r}")
            setattr(t, k, int(v))
        return self._L.cndp_tcb_set(self.h, idx, ctypes.byref(t))

    def set(self, idx: int, **fields) -> None:
        N.check(self.set_raw(idx, **fields), "cndp_tcb_set")

    def clear(self, idx: int) -> int:
        """cndp_tcb_clear; returns its result (0 or -errno)."""
        return self._L.cndp_tcb_clear(self.h, idx)

    def get(self, idx: int):
        """The snapshot as a dict, or None when the index has no TCB."""
        t = N.Tcb()
        r = self._L.cndp_tcb_get(self.h, idx, ctypes.byref(t))
        if r == -2:
            return None
        N.check(r, "cndp_tcb_get")
        return {k: int(getattr(t, k)) for k in TCB_FIELDS}

    def tx_set_raw(self, idx: int, **fields) -> int:
        """cndp_tcb_tx_set; returns its result (0 or -errno).  Fields not given are 0."""
        a = N.TcbTx()
        for k, v in fields.items():
            if k not in TCB_TX_FIELDS:
                raise TypeError(f"struct cndp_tcb_tx has no field {k!r}")
            setattr(a, k, int(v))
        return self._L.cndp_tcb_tx_set(self.h, idx, ctypes.byref(a))

    def tx_set(self, idx: int, **fields) -> None:
        N.check(self.tx_set_raw(idx, **fields), "cndp_tcb_tx_set")

    def tx_get(self, idx: int):
        """The transmit attributes as a dict, or None when the index has no TCB."""
        a = N.TcbTx()
        r = self._L.cndp_tcb_tx_get(self.h, idx, ctypes.byref(a))
        if r == -2:
            return None
        N.check(r, "cndp_tcb_tx_get")
        return {k: int(getattr(a, k)) for k in TCB_TX_FIELDS}

    def output_host(self, slab: np.ndarray, n: int, pcb, mode: int = N.CNDP_TCPOUT_SEGMENT, now: int = 0,
                    txseg=None, seg=None, verdict=None, rxmeta=None, sel=None, snd=None, src_off=None,
                    stride: int = 0, offsets=None, data_off: int = 0, stats=None) -> dict:
        """cndp_tcp_output_host over host arrays: the stage's rule on the calling
        thread, writing `slab` (a contiguous uint8 array) in place.  Returns len
        (uint16), faddr, laddr (uint32), taken (uint8) and stats
        (uint64[CNDP_TCPOUT_NSTATS], accumulated into `stats` when given)."""
        assert slab.dtype == np.uint8 and slab.flags["C_CONTIGUOUS"] and slab.flags["WRITEABLE"]
        m = max(n, 1)
        out = {"len": np.zeros(m, np.uint16), "faddr": np.zeros(m, np.uint32), "laddr": np.zeros(m, np.uint32),
               "taken": np.zeros(m, np.uint8),
               "stats": np.zeros(N.CNDP_TCPOUT_NSTATS, np.uint64) if stats is None else np.array(stats, np.uint64)}
        keep, given = [], []
        io = N.TcpOutIo()
        for name, arr, dt in (("sel", sel, np.uint8), ("pcb", pcb, np.uint32), ("txseg", txseg, TXSEG_DT),
                              ("seg", seg, SEG_DT), ("verdict", verdict, np.uint8), ("rxmeta", rxmeta, np.uint32),
                              ("snd", snd, np.uint8), ("src_off", src_off, np.uint64)):
            if arr is not None:
                keep.append(_aligned16(arr, dt))
                given.append((name, keep[-1].copy()))
                setattr(io, name, keep[-1].ctypes.data)
        if snd is not None:
            io.snd_len = int(np.asarray(snd).size)
        for name in ("len", "faddr", "laddr", "taken", "stats"):
            setattr(io, name, out[name].ctypes.data)
        offs = None
        if offsets is not None:
            offs = np.ascontiguousarray(offsets, np.uint64)
        N.check(self._L.cndp_tcp_output_host(self.h, mode, now & 0xFFFFFFFF, slab.ctypes.data, slab.size, stride,
                                             offs.ctypes.data if offs is not None else None, data_off, n,
                                             ctypes.byref(io)), "cndp_tcp_output_host")
        for (name, before), after in zip(given, keep):
            if not np.array_equal(before, after):
                raise RuntimeError(f"cndp_tcp_output_host wrote its input {name}")
        return {k: (v if k == "stats" else v[:n]) for k, v in out.items()}

    def segment_host(self, slab: np.ndarray, n: int, rxmeta, pcb, seg, now: int, l4edge=None, sel=None,
                     stride: int = 0, offsets=None, data_off: int = 0, stats=None) -> dict:
        """cndp_tcp_segment_host over host arrays: the stage's rule on the
        calling thread.  Returns opt (OPT_DT), verdict (uint8) and stats
        (uint64[CNDP_TCPSEG_NSTATS], accumulated into `stats` when given)."""
        keep = [np.ascontiguousarray(slab, np.uint8), np.ascontiguousarray(rxmeta, np.uint32),
                np.ascontiguousarray(pcb, np.uint32), np.ascontiguousarray(seg, SEG_DT)]
        opt, verdict = np.zeros(max(n, 1), OPT_DT), np.zeros(max(n, 1), np.uint8)
        st = np.zeros(N.CNDP_TCPSEG_NSTATS, np.uint64) if stats is None else np.array(stats, np.uint64)
        b = N.Batch()
        b.mode, b.n, b.slab, b.slab_len = N.CNDP_MODE_CNET, n, keep[0].ctypes.data, len(keep[0])
        b.stride, b.data_off, b.rxmeta = stride, data_off, keep[1].ctypes.data
        if offsets is not None:
            keep.append(np.ascontiguousarray(offsets, np.uint64))
            b.offsets = keep[-1].ctypes.data
        io = N.TcpSegIo()
        for name, arr in (("sel", sel), ("l4edge", l4edge)):
            if arr is not None:
                keep.append(np.ascontiguousarray(arr, np.uint8))
                setattr(io, name, keep[-1].ctypes.data)
        io.pcb, io.seg, io.opt, io.verdict, io.stats = (keep[2].ctypes.data, keep[3].ctypes.data, opt.ctypes.data,
                                                        verdict.ctypes.data, st.ctypes.data)
        N.check(self._L.cndp_tcp_segment_host(self.h, now & 0xFFFFFFFF, ctypes.byref(b), ctypes.byref(io)),
                "cndp_tcp_segment_host")
        return {"opt": opt[:n], "verdict": verdict[:n], "stats": st}


def _aligned16(arr, dt) -> np.ndarray:
    """A contiguous copy of `arr` as dtype dt whose first byte is 16-byte aligned."""
    a = np.ascontiguousarray(arr, dt)
    raw = np.zeros(a.nbytes + 16, np.uint8)
    o = (-raw.ctypes.data) % 16
    out = raw[o:o + a.nbytes].view(dt)
    out[...] = a.reshape(-1)
    return out


def send_optlen(tflags: int, seg_flags: int) -> int:
    """cndp_tcp_send_optlen: tcp_send_options' length (0, 4, 8, 12, 16 or 20) for a
    TCB with these CNDP_TCBF_* bits and a segment with these TCP flags."""
    return int(N.lib().cndp_tcp_send_optlen(tflags & 0xFF, seg_flags & 0xFF))


def alloc_tcpseg_outputs(n: int, device) -> dict:
    """The output arrays of cndp_gpu_tcp_segment as torch tensors.  opt is an
    (n, 4) int32 tensor, one 16-byte struct cndp_tcp_opt per row (opt_records()
    views it as OPT_DT)."""
    import torch
    m = max(n, 1)
    return {"opt": torch.empty((m, 4), dtype=torch.int32, device=device)[:n],
            "verdict": torch.empty(m, dtype=torch.uint8, device=device)[:n],
            "stats": torch.zeros(N.CNDP_TCPSEG_NSTATS, dtype=torch.int64, device=device)}


def opt_records(opt) -> np.ndarray:
    """The opt tensor of Classifier.tcp_segment on the host, as OPT_DT records."""
    return np.ascontiguousarray(opt.cpu().numpy()).view(OPT_DT).reshape(-1)

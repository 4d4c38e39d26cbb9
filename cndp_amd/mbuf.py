"""pktmbuf_t pools in host memory and the asynchronous node queue (cndp_gpu_mq_*).

MbufPool lays frames out the way CNDP's pktmbuf pool does inside an AF_XDP
UMEM (lib/core/pktmbuf/pktmbuf.h:102-204, pktmbuf.c:60-80): 2 KiB frames, the
64-byte pktmbuf_t header at the frame start, buf_addr = frame + 64,
buf_len = 1984, data_off = 192, so packet data starts at frame + 256.

MbufQueue wraps the C-ABI queue: submit bursts of mbuf pointers, poll the
finished ones (fields written back, next edges returned), in order.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native as N
from .l4 import OPT_DT, SEG_DT

# struct pktmbuf_s, 64 bytes (pktmbuf.h:102-204)
MBUF_DT = np.dtype([("pooldata", "<u8"), ("buf_addr", "<u8"), ("hash", "<u4"), ("meta_index", "<u4"),
                    ("data_off", "<u2"), ("lport", "<u2"), ("buf_len", "<u2"), ("data_len", "<u2"),
                    ("packet_type", "<u4"), ("refcnt", "<u2"), ("rsvd16", "<u2"), ("tx_offload", "<u8"),
                    ("ol_flags", "<u8"), ("udata64", "<u8")])
assert MBUF_DT.itemsize == 64

FRAME = 2048
HDR = 64
HEADROOM = 192          # data_off of a fresh mbuf: packet data at frame + 256
BUF_LEN = FRAME - HDR   # 1984


class MbufPool:
    """n mbufs in one page-aligned host buffer (optionally registered with a
    Classifier for zero-copy).  hugepages: an anonymous mapping advised for
    2 MiB transparent huge pages, 2 MiB-aligned, as a UMEM from CNDP's
    mmap_alloc(MMAP_HUGEPAGE_2MB) would be (lib/core/mmap/cne_mmap.h:29)."""

    def __init__(self, n: int, hugepages: bool = False):
        self.n = n
        if hugepages:
            import mmap
            self._mm = mmap.mmap(-1, n * FRAME + (2 << 20), flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
            self._mm.madvise(mmap.MADV_HUGEPAGE)
            raw = np.frombuffer(self._mm, np.uint8)
            a = (-raw.ctypes.data) % (2 << 20)
        else:
            raw = np.zeros(n * FRAME + 4096, np.uint8)
            a = (-raw.ctypes.data) % 4096
        self._raw = raw
        self.mem = raw[a:a + n * FRAME]
        self.base = self.mem.ctypes.data
        rows = self.mem.reshape(n, FRAME)
        self.hdr = rows[:, :HDR].view(MBUF_DT)[:, 0]
        self.hdr["buf_addr"] = self.base + np.arange(n, dtype=np.uint64) * FRAME + HDR
        self.hdr["buf_len"] = BUF_LEN
        self.hdr["data_off"] = HEADROOM
        self.hdr["refcnt"] = 1

    def addr(self, i: int) -> int:
        return self.base + i * FRAME

    def data_pos(self) -> np.ndarray:
        """Byte offset of each mbuf's packet data inside self.mem."""
        return (np.arange(self.n, dtype=np.uint64) * FRAME + HDR + self.hdr["data_off"].astype(np.uint64))

    def fill(self, frames, lengths=None, max_bytes: int = BUF_LEN - HEADROOM):
        """Copy frame i of a pktgen.Frames batch into mbuf i; data_len = its
        length (frames.lengths, else the slot size), at most max_bytes."""
        slab = frames.slab.cpu().numpy() if hasattr(frames.slab, "cpu") else np.asarray(frames.slab)
        n = frames.n
        assert n <= self.n
        if frames.offsets is not None:
            offs = frames.offsets.cpu().numpy().astype(np.int64)
        else:
            offs = np.arange(n, dtype=np.int64) * frames.stride
        offs = offs + frames.data_off
        if lengths is None:
            if frames.lengths is not None:
                lengths = frames.lengths.cpu().numpy().astype(np.int64)
            else:
                lengths = np.full(n, frames.stride, np.int64)
        dpos = self.data_pos()
        if frames.offsets is None and frames.lengths is None and slab.size >= n * frames.stride \
                and np.all(self.hdr["data_off"][:n] == HEADROOM):
            ln = int(min(frames.stride, max_bytes))   # fixed-stride slab: one strided copy
            rows = self.mem.reshape(self.n, FRAME)[:n, HDR + HEADROOM:HDR + HEADROOM + ln]
            rows[:] = slab[:n * frames.stride].reshape(n, frames.stride)[:, frames.data_off:frames.data_off + ln]
            self.hdr["data_len"][:n] = lengths
            return
        for i in range(n):
            o = int(offs[i])
            ln = int(min(lengths[i], max_bytes, max(0, slab.size - o)))
            d = int(dpos[i])
            self.mem[d:d + ln] = slab[o:o + ln]
            self.hdr["data_len"][i] = lengths[i]

    def ptrs(self, idx) -> "ctypes.Array":
        idx = np.asarray(idx, dtype=np.int64)
        arr = (ctypes.c_void_p * len(idx))()
        addrs = (self.base + idx.astype(np.uint64) * FRAME).tolist()
        arr[:] = addrs
        return arr

    def index_of(self, addrs) -> np.ndarray:
        return ((np.asarray(addrs, dtype=np.uint64) - np.uint64(self.base)) // FRAME).astype(np.int64)


class MbufQueue:
    """cndp_gpu_mq_* over a Classifier's context."""

    METADATA_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p)

    def __init__(self, cl, mode: int, flags: int = 0, batch: int = 8192, depth: int = 4,
                 max_delay_us: int = 50, umem=None, lport: int = 0, stage_max: int = 0, metadata=None,
                 fib=None, acl=None, acl_mode: int = N.CNDP_ACL_STRICT, acl_flags: int = 0, lports=(),
                 fwd_tbl=None, pcb_tbl=None, tx_mode: int = N.CNDP_TX_UDP, tcb=None):
        """metadata: cnet's pktmbuf_metadata hook, a Python function of the mbuf
        address returning the metadata address (None: m + 64).
        cndpfwd modes (CNDP_MQ_CFWD_FWD / _L3FWD / CNDP_MQ_ACL_FWD, cndp_mqfwd.h):
        lport is the incoming port, lports the ports that exist, fib the l3fwd
        FIB (cfwd.l3fwd_fib), acl an AclTable with acl_mode / acl_flags; the
        FIB and the table must outlive the queue.
        CNDP_MQ_IP4_FORWARD (cndp_mqcnet.h): fwd_tbl is the FwdTable the node
        resolves in; it must outlive the queue.
        CNDP_MQ_UDP_INPUT (cndp_mql4.h): pcb_tbl is the PcbTable ip4_proto +
        udp_input demultiplex in; it must outlive the queue.  metadata is the
        hook poll calls (returning 0 / None stands for NULL).
        CNDP_MQ_TCP_INPUT (cndp_mqtcp.h): pcb_tbl is the TCP PcbTable tcp_input
        looks connections up in; the create call is chosen by the mode.
        CNDP_MQ_IP4_OUTPUT (cndp_mqtx.h): fwd_tbl and pcb_tbl are the tables
        udp_output + ip4_output resolve in, tx_mode is CNDP_TX_UDP or
        CNDP_TX_IP4; metadata is the hook submit calls.
        CNDP_MQ_TCP_SEGMENT (cndp_mqtcb.h): pcb_tbl as for CNDP_MQ_TCP_INPUT and
        tcb the l4.TcbTable made over it; metadata is called by submit and poll."""
        self._L = N.lib()
        self._keep = (fib, acl, fwd_tbl, pcb_tbl, tcb)
        c = N.MqConf()
        c.mode, c.flags, c.batch, c.depth = mode, flags, batch, depth
        c.max_delay_us, c.stage_max, c.lport = max_delay_us, stage_max, lport
        c.umem = umem
        self._md_fn = self.METADATA_FN(metadata) if metadata else None  # kept alive with the queue
        if self._md_fn:
            c.metadata = ctypes.cast(self._md_fn, ctypes.c_void_p)
        h = ctypes.c_void_p()
        self.h = None
        if mode in (N.CNDP_MQ_CFWD_FWD, N.CNDP_MQ_CFWD_L3FWD, N.CNDP_MQ_ACL_FWD):
            from .acl import lport_mask
            w = N.MqFwd()
            w.fib = fib.h if fib is not None else None
            w.acl = acl.h if acl is not None else None
            w.acl_mode, w.acl_flags = acl_mode, acl_flags
            for k, bits in enumerate(lport_mask(lports)):
                w.lport_mask[k] = bits
            N.check(self._L.cndp_gpu_mq_create_fwd(cl.h, ctypes.byref(c), ctypes.byref(w), ctypes.byref(h)),
                    "cndp_gpu_mq_create_fwd")
        elif mode == N.CNDP_MQ_IP4_OUTPUT:
            N.check(self._L.cndp_gpu_mq_create_ip4_output(cl.h, ctypes.byref(c),
                                                          fwd_tbl.h if fwd_tbl is not None else None,
                                                          pcb_tbl.h if pcb_tbl is not None else None, tx_mode,
                                                          ctypes.byref(h)), "cndp_gpu_mq_create_ip4_output")
        elif mode == N.CNDP_MQ_TCP_SEGMENT:
            N.check(self._L.cndp_gpu_mq_create_tcp_segment(cl.h, ctypes.byref(c),
                                                           pcb_tbl.h if pcb_tbl is not None else None,
                                                           tcb.h if tcb is not None else None, ctypes.byref(h)),
                    "cndp_gpu_mq_create_tcp_segment")
        elif fwd_tbl is not None:
            N.check(self._L.cndp_gpu_mq_create_ip4_forward(cl.h, ctypes.byref(c), fwd_tbl.h, ctypes.byref(h)),
                    "cndp_gpu_mq_create_ip4_forward")
        elif pcb_tbl is not None and mode == N.CNDP_MQ_TCP_INPUT:
            N.check(self._L.cndp_gpu_mq_create_tcp_input(cl.h, ctypes.byref(c), pcb_tbl.h, ctypes.byref(h)),
                    "cndp_gpu_mq_create_tcp_input")
        elif pcb_tbl is not None:
            N.check(self._L.cndp_gpu_mq_create_udp_input(cl.h, ctypes.byref(c), pcb_tbl.h, ctypes.byref(h)),
                    "cndp_gpu_mq_create_udp_input")
        else:
            N.check(self._L.cndp_gpu_mq_create(cl.h, ctypes.byref(c), ctypes.byref(h)), "cndp_gpu_mq_create")
        self.h = h
        self.cl = cl

    def close(self):
        if self.h:
            self._L.cndp_gpu_mq_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, ptrs, n: int | None = None) -> int:
        n = len(ptrs) if n is None else n
        return N.check(self._L.cndp_gpu_mq_submit(self.h, ptrs, n), "cndp_gpu_mq_submit")

    def flush(self):
        N.check(self._L.cndp_gpu_mq_flush(self.h), "cndp_gpu_mq_flush")

    def wait(self):
        N.check(self._L.cndp_gpu_mq_wait(self.h), "cndp_gpu_mq_wait")

    @property
    def pending(self) -> int:
        return self._L.cndp_gpu_mq_pending(self.h)

    def stat(self, key: int) -> int:
        """cndp_gpu_mq_stat: a CNDP_MQ_STAT_* counter."""
        return N.check(self._L.cndp_gpu_mq_stat(self.h, key), "cndp_gpu_mq_stat")

    def poll(self, max_n: int = 1 << 16):
        out = (ctypes.c_void_p * max_n)()
        edges = np.zeros(max_n, np.uint16)
        k = N.check(self._L.cndp_gpu_mq_poll(self.h, out, edges.ctypes.data, max_n), "cndp_gpu_mq_poll")
        return np.array([x or 0 for x in out[:k]], dtype=np.uint64), edges[:k].copy()

    def poll_tcp(self, max_n: int = 1 << 16):
        """cndp_gpu_mq_poll_tcp (include/cndp_mqtcp.h): poll, and each returned
        mbuf's struct cndp_tcp_seg as a record array (l4.SEG_DT)."""
        out = (ctypes.c_void_p * max_n)()
        edges = np.zeros(max_n, np.uint16)
        segs = np.zeros(max_n, SEG_DT)
        k = N.check(self._L.cndp_gpu_mq_poll_tcp(self.h, out, edges.ctypes.data, segs.ctypes.data, max_n),
                    "cndp_gpu_mq_poll_tcp")
        return np.array([x or 0 for x in out[:k]], dtype=np.uint64), edges[:k].copy(), segs[:k].copy()

    def set_now(self, now: int):
        """cndp_gpu_mq_tcp_now (include/cndp_mqtcb.h): stk_get_timer_ticks() for
        the batches launched from here on."""
        N.check(self._L.cndp_gpu_mq_tcp_now(self.h, now & 0xFFFFFFFF), "cndp_gpu_mq_tcp_now")

    def poll_tcpseg(self, max_n: int = 1 << 16):
        """cndp_gpu_mq_poll_tcpseg (include/cndp_mqtcb.h): poll_tcp, and each
        returned mbuf's struct cndp_tcp_opt (l4.OPT_DT) and verdict (uint8)."""
        out = (ctypes.c_void_p * max_n)()
        edges = np.zeros(max_n, np.uint16)
        segs = np.zeros(max_n, SEG_DT)
        opts = np.zeros(max_n, OPT_DT)
        verdicts = np.zeros(max_n, np.uint8)
        k = N.check(self._L.cndp_gpu_mq_poll_tcpseg(self.h, out, edges.ctypes.data, segs.ctypes.data, opts.ctypes.data,
                                                    verdicts.ctypes.data, max_n), "cndp_gpu_mq_poll_tcpseg")
        return (np.array([x or 0 for x in out[:k]], dtype=np.uint64), edges[:k].copy(), segs[:k].copy(),
                opts[:k].copy(), verdicts[:k].copy())

    def run_tcpseg(self, pool: MbufPool, idx, bursts):
        """run() with poll_tcpseg: (addresses, edges, segs, opts, verdicts) in
        completion order."""
        segs, opts, verdicts = [], [], []

        def poll():
            a, e, s, o, v = self.poll_tcpseg()
            segs.append(s)
            opts.append(o)
            verdicts.append(v)
            return a, e
        a, e = self.run(pool, idx, bursts, poll=poll)
        if not segs:
            return a, e, np.zeros(0, SEG_DT), np.zeros(0, OPT_DT), np.zeros(0, np.uint8)
        return a, e, np.concatenate(segs), np.concatenate(opts), np.concatenate(verdicts)

    def run_tcp(self, pool: MbufPool, idx, bursts):
        """run() with poll_tcp: (addresses, edges, segs) in completion order."""
        segs = []

        def poll():
            a, e, s = self.poll_tcp()
            segs.append(s)
            return a, e
        a, e = self.run(pool, idx, bursts, poll=poll)
        return a, e, np.concatenate(segs) if segs else np.zeros(0, SEG_DT)

    def run(self, pool: MbufPool, idx, bursts, poll=None):
        """Submit mbufs pool[idx] as graph bursts of the given sizes, polling
        as a node would (drain while the queue is full), until every mbuf has
        come back.  Returns (addresses, edges) in completion order.  poll: the
        poll to use instead of self.poll (run_tcp's)."""
        idx = np.asarray(idx, dtype=np.int64)
        got_a, got_e = [], []
        poll = poll or self.poll
        pos = 0
        for b in bursts:
            ptrs = pool.ptrs(idx[pos:pos + b])
            done = 0
            while done < b:
                k = self.submit(ctypes.addressof(ptrs) + done * ctypes.sizeof(ctypes.c_void_p), b - done)
                done += k
                a, e = poll()
                got_a.append(a)
                got_e.append(e)
                if k == 0 and a.size == 0:
                    self.wait()
            pos += b
        for _ in range(1 << 20):
            if not self.pending:
                break
            self.flush()
            self.wait()
            a, e = poll()
            got_a.append(a)
            got_e.append(e)
        return np.concatenate(got_a) if got_a else np.zeros(0, np.uint64), \
            np.concatenate(got_e) if got_e else np.zeros(0, np.uint16)

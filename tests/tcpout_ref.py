"""Python restatement of the TCP transmit stage for the tcp_output tests
(include/cndp_tcpout.h), written from the reference's text and independent of
tcpout.c: tcp_send_options (lib/cnet/tcp/cnet_tcp.c:3742-3798),
the mbuf build in tcp_output (:836-870), tcp_send_segment (:371-517),
tcp_drop_with_reset (:1120-1149) and tcp_do_response (:1020-1108).  The mbuf is
modelled as the reference handles it -- a data_off that moves forward and is
prepended to -- so where the header lands is worked out here, not assumed.

Also here: the connection model of the tests (and the product
tables made from it), a buffer layout helper (packed / umem / offsets with any
alignment, random bytes and guard bytes behind the slab) and seeded random
descriptors."""
from __future__ import annotations

import numpy as np

FIN, SYN, RST, PSH, ACK, URG = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
REQ_SCALE, RCVD_SCALE, REQ_TSTAMP, RCVD_TSTAMP = 0x01, 0x02, 0x04, 0x08
SEGMENT, RESPOND = 0, 1
SENT, NOTSEL, NOPCB, NOLADDR, TOOBIG, RST_IN, MCAST, OPTS = range(8)
NSTATS = 8
VERDICT_RESET = 1
TCP_MAXWIN = 65535
SIZEOF_TCP, SIZEOF_IP4, SIZEOF_ETHER_ADDR = 20, 20, 6
M32 = 0xFFFFFFFF
GUARD = 0xA5
TXSEG_DT = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("wnd", "<u2"), ("urp", "<u2"), ("len", "<u2"),
                     ("flags", "u1"), ("rsvd", "u1")])
SEG_DT = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("wnd", "<u2"), ("urp", "<u2"), ("len", "<u2"),
                   ("flags", "u1"), ("offset", "u1")])
TX_ZERO = dict(tflags=0, req_recv_scale=0, rcv_scale=0)
TCB_ZERO = dict(rcv_nxt=0, snd_una=0, snd_nxt=0, snd_max=0, snd_wnd=0, snd_cwnd=0, ts_recent=0, last_ack_sent=0,
                rcv_space=0, max_mss=0, state=5, snd_scale=0, flags=0)


def net32(host: int) -> int:
    """A host-order address as the u32 a little-endian load of its wire bytes gives."""
    return int.from_bytes((host & M32).to_bytes(4, "big"), "little")


def send_options(tcb, tx, flags: int, now: int) -> bytes:
    """tcp_send_options; tcb None (this build's rule for the NULL the reference
    would dereference) gives no options."""
    if tcb is None:
        return b""
    p = bytearray()
    tf = tx["tflags"]
    if flags & SYN:
        p += bytes([2, 4, (tcb["max_mss"] >> 8) & 0xFF, tcb["max_mss"] & 0xFF])
        if tf & REQ_SCALE and (not flags & ACK or tf & RCVD_SCALE):
            p += bytes([3, 3, tx["req_recv_scale"] & 0xFF, 1])
    if tf & REQ_TSTAMP and not flags & RST and ((flags & (SYN | ACK)) == SYN or tf & RCVD_TSTAMP):
        p += ((1 << 24) | (1 << 16) | (8 << 8) | 10).to_bytes(4, "big")
        p += (now & M32).to_bytes(4, "big") + (tcb["ts_recent"] & M32).to_bytes(4, "big")
    return bytes(p)


class Mbuf:
    """One buffer of the slab: bounded stores and the reference's data_off."""

    def __init__(self, slab, slab_len, start, data_off):
        self.slab, self.slab_len, self.start, self.off = slab, slab_len, start, data_off

    def mtod(self) -> int:
        return self.start + self.off

    def prepend(self, k: int) -> int:
        self.off -= k
        return self.mtod()

    def put(self, at: int, data: bytes):
        k = max(0, min(len(data), self.slab_len - at))
        if k:
            self.slab[at:at + k] = np.frombuffer(bytes(data[:k]), np.uint8)

    def rd(self, at: int) -> int:
        return int(self.slab[at]) if 0 <= at < self.slab_len else 0


def tcp_header(lport, fport, seq, ack, optlen, flags, wnd, urp) -> bytes:
    """struct cne_tcp_hdr after the memset: ports big-endian as the key holds
    them, checksum zero."""
    return (lport.to_bytes(2, "big") + fport.to_bytes(2, "big") + (seq & M32).to_bytes(4, "big")
            + (ack & M32).to_bytes(4, "big") + bytes([((SIZEOF_TCP + optlen) >> 2) << 4, flags & 0xFF])
            + (wnd & 0xFFFF).to_bytes(2, "big") + b"\0\0" + (urp & 0xFFFF).to_bytes(2, "big"))


def output_segment(m: Mbuf, c, d, now, snd, src_off):
    """tcp_output from :836 on and tcp_send_segment, for connection model c and
    descriptor d.  Returns (status, optlen, len)."""
    if not c["live"] or c["tcb"] is None:
        return NOPCB, 0, 0
    if c["laddr"] == 0:
        return NOLADDR, 0, 0
    flags, ln = int(d["flags"]), int(d["len"])
    opts = send_options(c["tcb"], c["tx"], flags, now)
    if ln > c["tcb"]["max_mss"] - len(opts):
        return TOOBIG, 0, 0
    move = SIZEOF_TCP + len(opts) + SIZEOF_IP4 + SIZEOF_ETHER_ADDR
    m.off += move                                   # :858-859
    m.put(m.mtod(), bytes(move))                    # :862-863, at the NEW mtod
    if ln:                                          # tcp_mbuf_copydata; source bytes past snd read as zero
        src = bytes(snd[src_off:src_off + ln]) if src_off < len(snd) else b""
        m.put(m.mtod(), src + bytes(ln - len(src)))
    m.put(m.prepend(len(opts)), opts)               # :387
    at = m.prepend(SIZEOF_TCP)                      # :390
    m.put(at, tcp_header(c["lport"], c["fport"], int(d["seq"]), int(d["ack"]), len(opts), flags, int(d["wnd"]),
                         int(d["urp"])))
    return SENT, len(opts), ln


def drop_with_reset(seg, mcast: bool):
    """tcp_drop_with_reset: RST_IN / MCAST (the mbuf is freed) or tcp_do_response's (seq, ack, flags)."""
    fl = int(seg["flags"])
    if fl & RST:
        return RST_IN
    if mcast:
        return MCAST
    if fl & ACK:
        return int(seg["ack"]), 0, RST
    ln = int(seg["len"])
    if fl & SYN:
        ln = (ln + 1) & 0xFFFF                      # seg->len++, a uint16_t that already counts the SYN
    seq = 0                                         # seg->seq = 0 ...
    return seq, seq + ln, RST | ACK                 # ... before seg->seq + seg->len


def do_response(m: Mbuf, c, seq, ack, flags, now, data_off):
    """tcp_do_response.  Returns optlen."""
    m.off = data_off                                # pktmbuf_reset
    tcb = c["tcb"]
    opts = send_options(tcb, c["tx"], flags, now)
    m.off += SIZEOF_TCP + len(opts) + SIZEOF_ETHER_ADDR + SIZEOF_IP4
    m.put(m.prepend(len(opts)), opts)
    at = m.prepend(SIZEOF_TCP)
    m.put(at, bytes(SIZEOF_TCP + len(opts)))
    wnd = 0
    if tcb is not None and not flags & RST:
        sc = c["tx"]["rcv_scale"] & 31
        wnd = (min(tcb["rcv_space"], (TCP_MAXWIN << sc) & M32) >> sc) & 0xFFFF
    m.put(at, tcp_header(c["lport"], c["fport"], seq, ack, len(opts), flags, wnd, 0))
    m.put(at + SIZEOF_TCP, opts)
    return len(opts)


NOBODY = dict(live=False, tcb=None, tx=TX_ZERO, laddr=0, faddr=0, lport=0, fport=0)


def tcp_output_ref(slab, slab_len, n, conns, pcb, mode=SEGMENT, now=0, txseg=None, seg=None, verdict=None,
                   rxmeta=None, sel=None, snd=None, src_off=None, stride=0, offsets=None, data_off=0, stats=None):
    """The stage's effect on `slab` (written in place, nothing at or past
    slab_len) and its outputs for one batch.  conns[i] = PCB index i's model."""
    out = {"len": np.zeros(n, np.uint16), "faddr": np.zeros(n, np.uint32), "laddr": np.zeros(n, np.uint32),
           "taken": np.zeros(n, np.uint8),
           "stats": np.zeros(NSTATS, np.uint64) if stats is None else np.array(stats, np.uint64)}
    desc = txseg is not None
    for i in range(n):
        if sel is not None:
            cand = bool(sel[i])
        else:
            cand = mode == SEGMENT or (int(verdict[i]) & 0x0F) == VERDICT_RESET
        st, optlen, ln = NOTSEL, 0, 0
        if cand:
            p = int(pcb[i])
            c = conns[p] if p < len(conns) else NOBODY
            start = int(offsets[i]) if offsets is not None else i * stride
            m = Mbuf(slab, slab_len, start, data_off)
            if mode == SEGMENT:
                d = txseg[i]
                if snd is None and c["live"] and c["tcb"] is not None and c["laddr"] != 0:
                    # the payload is already at P: keep it across the memset, as the copy would restore it
                    k = len(send_options(c["tcb"], c["tx"], int(d["flags"]), now))
                    P = start + data_off + 46 + k
                    ln0 = int(d["len"])
                    hold = bytes(slab[P:min(P + ln0, slab_len)]) if P < slab_len else b""
                    hold += bytes(ln0 - len(hold))
                    st, optlen, ln = output_segment(m, c, d, now, np.frombuffer(hold, np.uint8), 0)
                else:
                    st, optlen, ln = output_segment(m, c, d, now, snd if snd is not None else np.zeros(0, np.uint8),
                                                    int(src_off[i]) if src_off is not None else 0)
            elif not c["live"]:
                st = NOPCB
            else:
                if desc:
                    r = (int(txseg[i]["seq"]), int(txseg[i]["ack"]), int(txseg[i]["flags"]))
                else:
                    mc = False
                    if rxmeta is not None:
                        ip = m.mtod() + (int(rxmeta[i]) & 0x7F)
                        dst = sum(m.rd(ip + 16 + k) << (8 * k) for k in range(4))     # ip->dst_addr as loaded
                        mc = 0xE0000000 <= dst <= 0xEFFFFFFF or bool(m.rd(m.mtod()) & 1)
                    r = drop_with_reset(seg[i], mc)
                if isinstance(r, tuple):
                    optlen = do_response(m, c, r[0], r[1], r[2], now, data_off)
                    st = SENT
                else:
                    st = r
            if st == SENT:
                out["len"][i] = 20 + optlen + ln
                out["faddr"][i], out["laddr"][i] = net32(c["faddr"]), net32(c["laddr"])
                out["taken"][i] = 1
                if optlen:
                    out["stats"][OPTS] += 1
        out["stats"][st] += 1
    return out


# ---------------------------------------------------------------------------
# the connection model and the product's tables
# ---------------------------------------------------------------------------
def conn(laddr=0x0A040001, lport=80, faddr=0xC6120001, fport=40000, tcb=None, tx=None, live=True) -> dict:
    return dict(laddr=laddr, lport=lport, faddr=faddr, fport=fport, live=live,
                tcb=None if tcb is None else dict(TCB_ZERO, **tcb), tx=dict(TX_ZERO, **(tx or {})))


def make_tables(conns, cap=None):
    """A PcbTable and TcbTable holding `conns` (index = position)."""
    from cndp_amd.l4 import PcbTable, TcbTable
    pcbs = PcbTable(cap or max(len(conns), 1))
    for i, c in enumerate(conns):
        assert pcbs.add(laddr=c["laddr"], lport=c["lport"], faddr=c["faddr"], fport=c["fport"]) == i
    tcbs = TcbTable(pcbs)
    for i, c in enumerate(conns):
        if c["tcb"] is not None:
            tcbs.set(i, **c["tcb"])
            if any(c["tx"].values()):
                tcbs.tx_set(i, **c["tx"])
    for i, c in enumerate(conns):
        if not c["live"]:
            assert pcbs.delete(i) == 0
    return pcbs, tcbs


TFLAG_MIXES = (0, REQ_SCALE, REQ_SCALE | RCVD_SCALE, REQ_TSTAMP, REQ_TSTAMP | RCVD_TSTAMP,
               REQ_SCALE | REQ_TSTAMP, 0x0F, RCVD_SCALE | RCVD_TSTAMP)


def random_world(rng, k: int):
    """k connection models: most usable, some without a TCB, deleted, with a zero
    local address or a tiny MSS."""
    conns = []
    for i in range(k):
        tcb = dict(max_mss=int(rng.choice([1460, 1460, 536, 9000, 30, 8])), ts_recent=int(rng.integers(0, 1 << 32)),
                   rcv_space=int(rng.choice([0, 1, 1460, 65535, 65536, 1 << 20, 0xFFFFFFFF])),
                   rcv_nxt=int(rng.integers(0, 1 << 32)))
        tx = dict(tflags=int(rng.choice(TFLAG_MIXES)), req_recv_scale=int(rng.choice([0, 7, 14, 255])),
                  rcv_scale=int(rng.choice([0, 0, 3, 7, 14])))
        c = conn(laddr=0x0A040001 + (i >> 8), lport=80 + (i & 3), faddr=0xC6120000 + i, fport=1024 + i, tcb=tcb, tx=tx)
        r = rng.random()
        if r < 0.06:
            c["tcb"], c["tx"] = None, dict(TX_ZERO)
        elif r < 0.10:
            c["live"] = False
        elif r < 0.14:
            c["laddr"] = 0
        elif r < 0.17:
            c["faddr"], c["fport"] = 0, 0      # a listener: the reply goes where the key says
        conns.append(c)
    return conns


FLAG_MIXES = (ACK, ACK, ACK | PSH, SYN, SYN | ACK, FIN | ACK, RST, RST | ACK, ACK | URG, 0, SYN | RST)


def random_descs(rng, conns, n, now, lens=(0, 1, 15, 16, 17, 45, 46, 47, 66, 100, 536, 1448), pcb=None):
    """n descriptors on random connections: (pcb, TXSEG_DT array).  About one in
    twelve is over its connection's MSS; PCB indices include NONE and one past
    the table."""
    if pcb is None:
        pcb = rng.integers(0, len(conns), n).astype(np.uint32)
        odd = rng.random(n)
        pcb[odd < 0.02] = 0xFFFFFFFF
        pcb[(odd >= 0.02) & (odd < 0.04)] = len(conns)
    d = np.zeros(n, TXSEG_DT)
    d["seq"], d["ack"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
    d["wnd"], d["urp"] = rng.integers(0, 1 << 16, n), rng.choice([0, 0, 0, 7, 65535], n)
    d["flags"] = rng.choice(FLAG_MIXES, n)
    d["len"] = rng.choice(lens, n)
    for i in range(n):
        p = int(pcb[i])
        c = conns[p] if p < len(conns) else None
        if c is None or c["tcb"] is None:
            continue
        room = c["tcb"]["max_mss"] - len(send_options(c["tcb"], c["tx"], int(d["flags"][i]), now))
        r = rng.random()
        if r < 0.08:
            d["len"][i] = max(room, 0) & 0xFFFF                  # exactly the MSS
        elif r < 0.16:
            d["len"][i] = (max(room, 0) + 1) & 0xFFFF            # one over
        elif d["len"][i] > max(room, 0):
            d["len"][i] = max(room, 0)
    return pcb, d


def need_bytes(conns, pcb, d, now, data_off) -> np.ndarray:
    """Bytes of its buffer frame i can touch: H + 46 + optlen + max(len, 46 + optlen)."""
    out = np.zeros(len(pcb), np.int64)
    for i in range(len(pcb)):
        p = int(pcb[i])
        c = conns[p] if p < len(conns) else None
        k = len(send_options(c["tcb"], c["tx"], int(d["flags"][i]), now)) if c is not None else 0
        out[i] = data_off + 46 + k + max(int(d["len"][i]), 46 + k)
    return out


def layout(kind: str, need, data_off: int, seed: int = 0, align: int = 1, guard: int = 96, cut=None, slot=None):
    """Buffers for frames that touch need[i] bytes each, filled with random bytes,
    then `guard` bytes of 0xA5 that no call may change.  kind: "packed" (equal
    slots of `slot` bytes, default the largest need rounded up to 4 + 1, so the
    slots' alignment walks), "umem" (2 KiB frames; data_off is part of the
    layout's contract, pass 256) or "offsets" (end to end, each start rounded up
    to `align`).  cut: the slab ends that many bytes before (positive) the last
    frame's last touched byte + 1.  Returns (buf, slab_len, stride, offsets)."""
    need = np.asarray(need, np.int64)
    n = len(need)
    rng = np.random.default_rng(7000 + seed)
    stride, offs = 0, None
    if kind == "packed":
        stride = slot or (int(need.max(initial=1)) + 3) // 4 * 4 + 1
        starts = np.arange(n, dtype=np.int64) * stride
        total = n * stride
    elif kind == "umem":
        stride = 2048
        assert need.max(initial=0) <= 2048
        starts = np.arange(n, dtype=np.int64) * 2048
        total = n * 2048
    else:
        starts, at = np.zeros(n, np.int64), 0
        for i in range(n):
            at = (at + align - 1) // align * align
            starts[i] = at
            at += int(need[i])
        total = at
        offs = starts.astype(np.uint64)
    slab_len = total
    if cut is not None and n:
        slab_len = int(starts[-1] + need[-1]) - cut
    buf = rng.integers(0, 256, max(total, slab_len) + guard, dtype=np.uint8)
    buf[slab_len:] = GUARD
    return buf, slab_len, stride, offs

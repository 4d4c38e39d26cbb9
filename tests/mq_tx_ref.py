"""Python restatement of cnet's udp_output and ip4_output nodes over pktmbuf_t
bursts, for the tests of the mbuf queue's CNDP_MQ_IP4_OUTPUT mode and of
cndp_ip4_output_node_host (include/cndp_mqtx.h).  Written from the reference's
text (CNDP v25.08.0 lib/cnet/udp/udp_output.c:33-65, lib/cnet/ipv4/ip4_output.c:48-126,
pktmbuf.h:924-983) over an MbufPool's memory, mbuf by mbuf, effect by effect, in
submission order.  The world (FIBs as route lists, the PCB vector, the netifs'
ip_ident) and the checksums are tests/tx_ref.py's; the pools and burst helpers
are tests/mq_udp_ref.py's.  Nothing here shares code with tx.c or the kernels.

Build-defined (include/cndp_mqtx.h): the low 32 bits of m->userptr are the PCB
index and an mbuf whose userptr is above 32 bits, past the vector or names a
deleted PCB is not taken; zero-copy, an mbuf whose header or whose headroom
[max(buf_addr, mtod - 42 / 34), mtod) is not inside the region is not taken; the
L4 bytes read for a checksum are [mtod, mtod + data_len) clipped at the buffer's
end and at the region's end (zero-copy) or at stage_max (staged), bytes past the
clip read as zero and are never written."""
from __future__ import annotations

import ctypes

import numpy as np

import tx_ref as T
from mq_udp_ref import make_pool, split, _u, _put  # noqa: F401  (the tests use them through this module)

EDGE_NONE = 0xFFFF
TX_UDP, TX_IP4 = 0, 1
CKBIT = 0x1000
NOMD_C, HEADROOM_C, NOROUTE_C, PROTO_C = 1, 2, 3, 4
# the seven counters, in key order (CNDP_MQ_STAT_TX_SENT ...)
SENT, ARP, NOMD, HEADROOM, NOROUTE, PROTO, CKSUM = range(7)
NSTAT = 7
BUF_ADDR, DATA_OFF, BUF_LEN, DATA_LEN, TX_OFFLOAD, USERPTR = 8, 24, 28, 30, 40, 56
PAYLOADS = (0, 1, 2, 3, 17, 18, 64, 333, 1472)


def drop(cause: int) -> int:
    return cause << 9


def node_ref(mem: np.ndarray, base: int, tw: T.TxWorld, objs, mode: int, zero_copy: bool, stage_max: int = 2048,
             md_of=None):
    """Run the two nodes over `objs` (mbuf byte offsets into `mem`, None for an
    mbuf outside the region) on the region `mem`, whose first byte has address
    `base`; `mem` is edited in place and tw.ident moves.  md_of(mbuf offset) ->
    metadata offset or None.  Returns (edges, the seven counters)."""
    size = len(mem)
    w = tw.w
    edges, stats = [], [0] * NSTAT
    img_end = 42 if mode == TX_UDP else 34
    for mo in objs:
        if mo is None or mo < 0 or mo + 64 > size:
            edges.append(EDGE_NONE)
            continue
        up = _u(mem, mo + USERPTR, 8)
        H, blen, dlen = _u(mem, mo + DATA_OFF, 2), _u(mem, mo + BUF_LEN, 2), _u(mem, mo + DATA_LEN, 2)
        buf = _u(mem, mo + BUF_ADDR, 8) - base
        f = buf + H                                          # mtod at submit
        p = tw.pcb(up) if up <= 0xFFFFFFFF else None
        if p is None or (zero_copy and not (0 <= f - min(H, img_end) and f <= size)):
            edges.append(EDGE_NONE)
            continue
        md = mo + 64 if md_of is None else md_of(mo)
        if md is None:                                       # udp_output.c:40-42, ip4_output.c:64-66
            edges.append(drop(NOMD_C))
            stats[NOMD] += 1
            continue
        fport, faddr = bytes(mem[md + 2:md + 4]), bytes(mem[md + 4:md + 8])
        lport, laddr = bytes(mem[md + 22:md + 24]), bytes(mem[md + 24:md + 28])
        txo = _u(mem, mo + TX_OFFLOAD, 8)
        R = min(dlen, max(0, blen - H))
        R = min(R, size - f) if zero_copy else min(R, stage_max)
        pay = bytes(mem[f:f + R])
        doff, dl = H, dlen

        def leave(edge, key):
            _put(mem, mo + TX_OFFLOAD, txo, 8)
            _put(mem, mo + DATA_OFF, doff, 2)
            _put(mem, mo + DATA_LEN, dl, 2)
            edges.append(edge)
            if key is not None:
                stats[key] += 1

        def store(o, b):
            mem[buf + o:buf + o + len(b)] = np.frombuffer(bytes(b), np.uint8)

        udp = b""
        if mode == TX_UDP:                                   # udp_output
            txo = 0                                          # :46-47
            if 8 > doff:                                     # pktmbuf_adjust(m, -8)
                leave(drop(HEADROOM_C), HEADROOM)
                continue
            doff, dl = doff - 8, (dl + 8) & 0xFFFF
            udp = lport + fport + dl.to_bytes(2, "big") + b"\0\0"
            store(doff, udp)
        l4 = doff
        txo = (txo & ~(0x1FF << 7)) | 20 << 7                # m->l3_len
        if 20 > doff:                                        # pktmbuf_prepend(m, 20)
            leave(drop(HEADROOM_C), HEADROOM)
            continue
        doff, dl = doff - 20, (dl + 20) & 0xFFFF
        ip = doff
        hdr = bytearray(bytes([0x45, p.tos]) + dl.to_bytes(2, "big") + bytes([0, 0, 0, 0, p.ttl, p.proto, 0, 0])
                        + laddr + faddr)
        store(ip, hdr[:4])
        store(ip + 6, hdr[6:])                               # packet_id: not yet
        r = w.rt_obj(int.from_bytes(laddr, "big"))           # be32toh(ip->src_addr)
        if r is None:
            leave(drop(NOROUTE_C), NOROUTE)
            continue
        txo = (txo & ~0x7F) | 14                             # m->l2_len
        if 14 > doff:                                        # pktmbuf_prepend(m, 14)
            leave(drop(HEADROOM_C), HEADROOM)
            continue
        doff, dl = doff - 14, (dl + 14) & 0xFFFF
        eth = doff
        nif = w.rt[r][1]
        store(eth + 6, w.mac(nif) + b"\x08\x00")
        ident = tw.ident.get(nif, 0)
        hdr[4:6] = ident.to_bytes(2, "big")
        store(ip + 4, hdr[4:6])
        total = int.from_bytes(hdr[2:4], "big")
        tw.ident[nif] = (ident + T.bswap16(total)) & 0xFFFF  # += ip->total_length as loaded
        hdr[10:12] = T.ipv4_cksum(hdr).to_bytes(2, "little")
        store(ip + 10, hdr[10:12])
        ck = 0
        if p.proto in (17, 6):
            if p.proto == 6 or p.cksum:
                c = T.udptcp_cksum(hdr, udp + pay + bytes(65536)).to_bytes(2, "little")
                at = 6 if p.proto == 17 else 16
                for k in range(2):
                    if at + k < len(udp) + R:                # past the clip: never written
                        store(l4 + at + k, c[k:k + 1])
                ck = CKBIT
                stats[CKSUM] += 1
        else:
            leave(drop(PROTO_C), PROTO)
            continue
        a = w.arp_obj(int.from_bytes(faddr, "big"))          # be32toh(ip->dst_addr)
        if a is None:
            leave(T.ARP_REQUEST | ck, ARP)
            continue
        store(eth, w.arp[a][1])
        leave((nif + T.NEXT_MAX) | ck, SENT)                 # the route's netif, not the ARP entry's
    return np.array(edges, np.uint16), stats


# ---- the world kept twice: the restatement's and the product's tables ---------
class World:
    def __init__(self, tw: T.TxWorld):
        self.tw = tw
        self.arp, self.rt4, self.fwd, self.pt = T.make_tables(tw)

    def close(self):
        T.close_tables(self.arp, self.rt4, self.fwd, self.pt)

    def set_ident(self, ident: dict):
        from cndp_amd import tx as X
        for nif, v in ident.items():
            assert X.ident_set(self.fwd, nif, v) == 0

    def get_ident(self, nifs) -> dict:
        from cndp_amd import tx as X
        return {nif: X.ident_get(self.fwd, nif) for nif in nifs}


def rewind(world: World, want):
    """Put the restatement's and the table's counters back to where `want` began."""
    world.tw.ident = dict(want["ident0"])
    world.set_ident(want["ident0"])


def standard_world(netifs: int = 5, ident0: int = 0xFFF0) -> World:
    return World(T.standard_world(netifs, ident0))


def _hook(b0: int, md_delta, md_null):
    from cndp_amd.mbuf import FRAME
    if md_delta is None and md_null is None:
        return None

    def hook(m):
        if md_null is not None and md_null((m - b0) // FRAME):
            return None
        return m + (64 if md_delta is None else md_delta)
    return hook


def run_twin(pool, world: World, bursts, mode: int, zero_copy: bool, stage_max: int = 2048, md_delta=None,
             md_null=None):
    """cndp_ip4_output_node_host burst by burst over a copy of the pool (its
    buf_addr fields moved to the copy for the run and back after it): (edges, memory)."""
    from cndp_amd.tx import ip4_output_node_host
    from cndp_amd.mbuf import FRAME, MBUF_DT
    raw = np.zeros(pool.mem.size + 4096, np.uint8)
    a = (-raw.ctypes.data) % 4096
    mem = raw[a:a + pool.mem.size]
    mem[:] = pool.mem
    delta = np.uint64((mem.ctypes.data - pool.base) % (1 << 64))
    hdr = mem.reshape(pool.n, FRAME)[:, :64].view(MBUF_DT)[:, 0]
    with np.errstate(over="ignore"):
        hdr["buf_addr"] += delta
    hook = _hook(mem.ctypes.data, md_delta, md_null)
    edges = []
    for b in bursts:
        for lo in range(0, max(len(b), 1), 256):
            part = b[lo:lo + 256]
            ptrs = (ctypes.c_void_p * max(len(part), 1))(*[None if i is None else mem.ctypes.data + int(i) * FRAME
                                                           for i in part])
            edges.append(ip4_output_node_host(world.fwd, world.pt, ptrs, len(part), tx_mode=mode,
                                              readable_end=mem.ctypes.data + mem.size if zero_copy else 0,
                                              stage_max=0 if zero_copy else stage_max, metadata=hook))
    with np.errstate(over="ignore"):
        hdr["buf_addr"] -= delta
    return (np.concatenate(edges) if edges else np.zeros(0, np.uint16)), mem


def expect(pool, world: World, bursts, mode: int, zero_copy: bool, stage_max: int = 2048, md_delta=None,
           md_null=None):
    """What the queue must leave after `bursts` (lists of mbuf indices, None: an
    mbuf outside the region): the restatement's edges, counters, pool memory and
    netif counters, which the host twin run on a copy of the pool must reproduce
    exactly.  The table's counters are put back to where they stood, so the queue
    run that follows starts where both started."""
    from cndp_amd.mbuf import FRAME
    tw = world.tw
    mem = pool.mem.copy()
    md_of = None
    if md_delta is not None or md_null is not None:
        def md_of(mo):
            if md_null is not None and md_null(mo // FRAME):
                return None
            return mo + (64 if md_delta is None else md_delta)
    objs = [None if i is None else int(i) * FRAME for b in bursts for i in b]
    ident0 = dict(tw.ident)
    edges, stats = node_ref(mem, pool.base, tw, objs, mode, zero_copy, stage_max, md_of)
    ident1 = dict(tw.ident)
    world.set_ident(ident0)
    t_edges, t_mem = run_twin(pool, world, bursts, mode, zero_copy, stage_max, md_delta, md_null)
    assert np.array_equal(t_edges, edges), f"twin edges {t_edges.tolist()} != restatement {edges.tolist()}"
    bad = np.nonzero(t_mem != mem)[0]
    assert len(bad) == 0, (f"twin memory: {len(bad)} bytes differ from the restatement, first at mbuf "
                           f"{bad[0] // FRAME} + {bad[0] % FRAME}: {t_mem[bad[0]]:#x} != {mem[bad[0]]:#x}")
    assert world.get_ident(ident1) == ident1, "twin counters differ from the restatement's"
    world.set_ident(ident0)
    return {"edges": edges, "stats": stats, "mem": mem, "ident0": ident0, "ident1": ident1}


# ---- mbufs in the product's pools ----------------------------------------------
TXO0 = 0x5A << 24 | 8 << 16 | 20 << 7 | 14     # what udp_input / the TCP continuation left: other bits set


def put(pool, world: World, i: int, pcb: int, faddr=None, fport: int = 0x1234, length: int = 18, data_off: int = 192,
        data_len=None, userptr=None, md_at: int = 64, seed=None, laddr=None):
    """mbuf i as the application hands it to udp_output / ip4_output: `length`
    random bytes at buf_addr + data_off, the PCB index in userptr, the metadata
    at m + md_at with the PCB's local address and port (0 for an index without
    a PCB) and the given foreign ones."""
    from cndp_amd.mbuf import FRAME, HDR, BUF_LEN
    rng = np.random.default_rng(3000 + i if seed is None else seed)
    tw = world.tw
    p = tw.pcbs[pcb] if 0 <= pcb < len(tw.pcbs) else None
    m = i * FRAME
    o = m + HDR + data_off
    n = max(0, min(length, BUF_LEN - data_off))
    pool.mem[o:o + n] = rng.integers(0, 256, n, dtype=np.uint8)
    md = m + md_at
    pool.mem[md:md + 40] = 0
    pool.mem[md], pool.mem[md + 1], pool.mem[md + 20], pool.mem[md + 21] = 2, 4, 2, 4
    _put(pool.mem, md + 2, fport, 2)
    _put(pool.mem, md + 4, T.ip_n(T.FOREIGN[i % len(T.FOREIGN)]) if faddr is None else faddr, 4)
    _put(pool.mem, md + 22, p.lport if p else 0, 2)
    _put(pool.mem, md + 24, (p.laddr if p else 0) if laddr is None else laddr, 4)
    pool.hdr["data_off"][i] = data_off
    pool.hdr["data_len"][i] = (length if data_len is None else data_len) & 0xFFFF
    pool.hdr["tx_offload"][i] = TXO0
    pool.hdr["udata64"][i] = pcb if userptr is None else userptr


def craft_zero(pool, world: World, i: int, pcb: int, length: int = 18, data_off: int = 192):
    """put(), with the payload's first word chosen so that the UDP checksum
    computes to 0 and goes out as 0xFFFF (CNDP_TX_UDP, a PCB with the flag)."""
    from cndp_amd.mbuf import FRAME, HDR
    put(pool, world, i, pcb, length=length, data_off=data_off)
    p = world.tw.pcbs[pcb]
    assert p.proto == 17 and p.cksum and length >= 2
    m = i * FRAME
    o = m + HDR + data_off
    pool.mem[o:o + 2] = 0
    md = m + 64
    dl = length + 8
    udp = bytes(pool.mem[md + 22:md + 24]) + bytes(pool.mem[md + 2:md + 4]) + dl.to_bytes(2, "big") + b"\0\0"
    hdr = bytes([0x45, p.tos]) + (dl + 20).to_bytes(2, "big") + bytes([0, 0, 0, 0, p.ttl, 17, 0, 0]) \
        + bytes(pool.mem[md + 24:md + 28]) + bytes(pool.mem[md + 4:md + 8])
    c0 = T.udptcp_cksum(hdr, udp + bytes(pool.mem[o:o + length]))
    # the sum with the word at 0 is ~c0 (c0 = 0xFFFF stands for 0 too): the word c0 brings it to 0xFFFF
    pool.mem[o:o + 2] = np.frombuffer(int(c0).to_bytes(2, "little"), np.uint8)
    assert T.udptcp_cksum(hdr, udp + bytes(pool.mem[o:o + length])) == 0xFFFF


# PCBs of tx_ref.standard_world(): 0-27 UDP from LOCALS[k % 7] (k % 7 in 4, 5, 6: no route), odd ones with
# the checksum flag; 28-31 on netif 1; 32 TCP; 33 protocol 1; 34 tos / ttl; 35 deleted
ROUTED = [k for k in range(28) if k % 7 < 4] + [28, 29, 30, 31]
PCB_TCP, PCB_PROTO1, PCB_TOS, PCB_DEAD = 32, 33, 34, 35


def fill_mix(pool, world: World, mode: int, seed: int = 5, n=None):
    """The standard mix: every PCB of the world, NONE / out-of-range / deleted /
    above-32-bit userptr values, every payload length, every alignment of mtod,
    and every 11th mbuf with a headroom of 0-50."""
    n = pool.n if n is None else n
    tw = world.tw
    rng = np.random.default_rng(seed)
    pcb, faddr, _, ports, length = T.make_inputs(n, tw, seed, lens=PAYLOADS)
    for i in range(n):
        doff = 176 + int(rng.integers(0, 32))
        if i % 11 == 3:
            doff = int(rng.integers(0, 51))
        up = int(pcb[i])
        if i % 97 == 5:
            up = (1 << 32) | (up & 0xFF)
        ln = int(length[i])
        if mode == TX_IP4 and ln < 20 and i % 3:
            ln = 20 + ln
        put(pool, world, i, int(pcb[i]) if int(pcb[i]) < len(tw.pcbs) else -1, faddr=int(faddr[i]),
            fport=int(ports[i]) & 0xFFFF, length=ln, data_off=doff, userptr=up, seed=seed * 100000 + i)


def fill_headrooms(pool, world: World, mode: int):
    """Headrooms 0-50 (and the defaults around them) for a routed checksum PCB, an
    unrouted one, the TCP one and the protocol-1 one; returns the count."""
    i = 0
    for H in range(0, 51):
        for pcb in (1, 5, PCB_TCP, PCB_PROTO1):
            put(pool, world, i, pcb, length=(18, 64, 3)[H % 3] + (20 if mode == TX_IP4 else 0), data_off=H)
            i += 1
    return i


def fill_lens(pool, world: World, mode: int):
    """Every payload length at every data_off % 16, with a checksum: UDP PCBs with
    the flag and the TCP PCB; returns the count."""
    i = 0
    for ln in PAYLOADS:
        for al in range(16):
            pcb = (1, 3, PCB_TCP, 29)[(al + ln) % 4]
            put(pool, world, i, pcb, length=ln, data_off=192 + al)
            i += 1
    return i

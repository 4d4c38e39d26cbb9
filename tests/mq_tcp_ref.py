"""Python restatement of cnet's tcp_input node and the opening of
cnet_tcp_input over pktmbuf_t bursts, for the tests of the mbuf queue's
CNDP_MQ_TCP_INPUT mode and of cndp_tcp_input_node_host (include/cndp_mqtcp.h).
Written from the reference's text (CNDP v25.08.0 lib/cnet/tcp/tcp_input.c:41-119,
lib/cnet/tcp/cnet_tcp.c:3329-3414, pktmbuf.h:955-985) over an MbufPool's memory.
The lookup and the checksum verify are tests/l4_ref.py's lookup_ref and
cksum_verify, the latter over a per-frame bounded view; the pools, the table
kept twice and the burst helpers are tests/mq_udp_ref.py's.  Nothing here shares
code with pcb.c or the kernel.

Build-defined (include/cndp_mqtcp.h): userptr at submit is not read and the
family is AF_INET; a frame's readable bytes are cndp_mql4.h's; an mbuf whose
l3_len is not 20 stays as cnet_tcp_input is handed it and leaves on SEGMENT |
IPOPT with the record the batch stage computes."""
from __future__ import annotations

import ctypes

import numpy as np

import l4_ref as R
from mq_udp_ref import World, make_pool, split, _u, _put, _ip  # noqa: F401  (the tests use them through this module)

EDGE_NONE = 0xFFFF
CK, IPOPT = 0x0080, 0x0040
TCP_DROP, TCP_SEG, TCP_PUNT = 0x0500, 0x0501, 0x0502
# the eight counters, in key order (CNDP_MQ_STAT_TCP_SEGMENT ...)
SEGMENT, NOMATCH, CKSUM, NOMD, ADJUST, SHORT, BADOFF, OPT = range(8)
NSTAT = 8
BUF_ADDR, DATA_OFF, BUF_LEN, DATA_LEN, TX_OFFLOAD, USERPTR = 8, 24, 28, 30, 40, 56
# struct cndp_tcp_seg
SEG_DT = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("wnd", "<u2"), ("urp", "<u2"), ("len", "<u2"),
                   ("flags", "u1"), ("offset", "u1")])
SYN_FIN_CNT = (0, 1, 1, 2)           # tcp_syn_fin_cnt[flags & (FIN | SYN)]


def seg_of(tcp: np.ndarray, tot: int, l3: int):
    """struct seg_entry's frame fields (cnet_tcp.c:3386-3414) from the 20 header
    bytes; None where the reference takes rx_badoff."""
    offset = (int(tcp[12]) & 0xF0) >> 2
    if offset < 20 or offset > tot:
        return None
    flags = int(tcp[13]) & 0x3F
    tlen = (tot - (offset + l3)) & 0xFFFF                   # uint16_t tlen -= ...
    return (int.from_bytes(tcp[4:8].tobytes(), "big"), int.from_bytes(tcp[8:12].tobytes(), "big"),
            int.from_bytes(tcp[14:16].tobytes(), "big"), int.from_bytes(tcp[18:20].tobytes(), "big"),
            (tlen + SYN_FIN_CNT[flags & 3]) & 0xFFFF, flags, offset)


def node_ref(mem: np.ndarray, base: int, ent: np.ndarray, users, objs, zero_copy: bool, stage_max: int = 2048,
             punt: bool = True, md_of=None):
    """Run the node over `objs` (mbuf byte offsets into `mem`, None for an mbuf
    outside the region) on the region `mem`, whose first byte has address
    `base`; `mem` is edited in place.  Returns (edges, segs, the eight counters)."""
    size = len(mem)
    edges, stats = [], [0] * NSTAT
    segs = np.zeros(len(objs), SEG_DT)
    for k, mo in enumerate(objs):
        if mo is None or mo < 0 or mo + 64 > size:
            edges.append(EDGE_NONE)
            continue
        f = _u(mem, mo + BUF_ADDR, 8) - base + _u(mem, mo + DATA_OFF, 2)
        doff, blen, dlen = _u(mem, mo + DATA_OFF, 2), _u(mem, mo + BUF_LEN, 2), _u(mem, mo + DATA_LEN, 2)
        l3 = (_u(mem, mo + TX_OFFLOAD, 8) >> 7) & 0x1FF
        if zero_copy and not 0 <= f < size:
            edges.append(EDGE_NONE)
            continue
        readable = min(dlen, max(0, blen - doff))
        readable = min(readable, size - f) if zero_copy else min(readable, stage_max)
        view = R.View(mem[f:f + readable].copy())
        md = (mo + 64) if md_of is None else md_of(mo)
        if md is None:                                     # tcp_input.c:55-57
            edges.append(TCP_DROP)
            stats[NOMD] += 1
            continue
        ip, tcp = view.rd(0, 20), view.rd(l3, 20)
        faddr, laddr = int(ip[12:16].view("<u4")[0]), int(ip[16:20].view("<u4")[0])
        fport, lport = int(tcp[0:2].view("<u2")[0]), int(tcp[2:4].view("<u2")[0])
        tot = int(ip[2]) << 8 | int(ip[3])
        _put(mem, md + 2, fport, 2)                        # :91-92
        _put(mem, md + 22, lport, 2)
        p = R.lookup_ref(ent, laddr, faddr, lport, fport)
        if p == R.NONE:                                    # userptr stays
            edges.append(TCP_PUNT if punt else TCP_DROP)
            stats[NOMATCH] += 1
            continue
        if not R.cksum_verify(view, 0, l3):                # always, whatever the field holds
            edges.append(TCP_DROP | CK)
            stats[CKSUM] += 1
            continue
        _put(mem, mo + USERPTR, users[p], 8)
        for o, addr, port in ((md, faddr, fport), (md + 20, laddr, lport)):
            mem[o:o + 20] = 0
            mem[o], mem[o + 1] = 2, 4                      # AF_INET, sizeof(struct in_addr)
            _put(mem, o + 2, port, 2)
            _put(mem, o + 4, addr, 4)
        sg = seg_of(tcp, tot, l3)
        if l3 != 20:                                       # build-defined: as at cnet_tcp_input's call
            if sg is not None:
                segs[k] = sg
            edges.append(TCP_SEG | IPOPT)
            stats[OPT] += 1
            continue
        if l3 > dlen or l3 + doff > blen:                  # pktmbuf_adjust(m, l3_len) == NULL
            edges.append(TCP_DROP)
            stats[ADJUST] += 1
            continue
        doff, dlen = (doff + l3) & 0xFFFF, (dlen - l3) & 0xFFFF
        _put(mem, mo + DATA_OFF, doff, 2)
        _put(mem, mo + DATA_LEN, dlen, 2)
        if dlen < 20:                                      # rx_short
            edges.append(TCP_DROP)
            stats[SHORT] += 1
            continue
        offset = (int(tcp[12]) & 0xF0) >> 2
        if not (offset > dlen or offset + doff > blen):    # pktmbuf_adj_offset(m, offset)
            _put(mem, mo + DATA_OFF, (doff + offset) & 0xFFFF, 2)
            _put(mem, mo + DATA_LEN, (dlen - offset) & 0xFFFF, 2)
        if sg is None:                                     # rx_badoff
            edges.append(TCP_DROP)
            stats[BADOFF] += 1
            continue
        segs[k] = sg
        edges.append(TCP_SEG)
        stats[SEGMENT] += 1
    return np.array(edges, np.uint16), segs, stats


# ---- frames in the product's pools -------------------------------------------
def put(pool, i: int, src="198.18.0.1", dst="10.4.0.7", sport=40000, dport=5000, seglen=32, l3=20, data_off=192,
        cksum="good", tot=None, data_len=None, nib=5, flags=0x10, proto=6, seed=None, clip=None, fix=None):
    """mbuf i as ip4_proto hands it on: an IPv4 header of l3 bytes (IHL = l3 / 4)
    and a TCP segment of `seglen` bytes (its 20-byte header included) at
    buf_addr + data_off; l2_len 14, l3_len, l4_len 20 in tx_offload; data_len =
    total_length unless given.  nib: the data offset nibble; flags: byte 13.
    The sum is made right over the frame's first `clip` bytes with zeros behind
    them (None: the whole frame), by the 16-bit word at frame offset `fix` (None:
    the TCP checksum field; 12: the source address, for a frame whose TCP header
    cannot be read).  cksum: "good"; "zero" (the field cleared after a good sum:
    fails); "ffff" (the urgent pointer chosen so that the right field is 0x0000,
    which travels: passes); "alias" (that segment with 0xFFFF in the field: the
    same sum); "first" / "last" (bit 0 of the segment's first / bit 5 of its last
    byte flipped after a good sum)."""
    from cndp_amd.mbuf import FRAME, HDR
    rng = np.random.default_rng(2000 + i if seed is None else seed)
    total = l3 + seglen if tot is None else tot
    fr = bytearray(rng.integers(0, 256, l3 + max(seglen, 20), dtype=np.uint8).tobytes())
    fr[0] = 0x40 | (l3 // 4)
    fr[2:4] = (total & 0xFFFF).to_bytes(2, "big")
    fr[6:8] = b"\x00\x00"
    fr[9] = proto
    fr[12:16], fr[16:20] = _ip(src), _ip(dst)
    fr[l3:l3 + 2], fr[l3 + 2:l3 + 4] = sport.to_bytes(2, "big"), dport.to_bytes(2, "big")
    fr[l3 + 12] = nib << 4
    fr[l3 + 13] = flags
    fr[l3 + 16:l3 + 18] = b"\x00\x00"

    def total_sum():
        """the verify's sum over the clipped frame, folded"""
        v = np.zeros(l3 + 65536, np.uint8)
        m = len(fr) if clip is None else min(clip, len(fr))
        v[:m] = np.frombuffer(bytes(fr[:m]), np.uint8)
        L = max(total - (fr[0] & 0xF) * 4, 0) if m > 3 else 0
        psd = np.concatenate([v[12:20], np.array([0, v[9], (L >> 8) & 0xFF, L & 0xFF], np.uint8)])
        return R._fold(R.raw_cksum(v[l3:l3 + L]) + R.raw_cksum(psd)) & 0xFFFF

    def solve(o):
        """the 16-bit word at frame offset o that makes the sum 0xFFFF"""
        fr[o:o + 2] = b"\x00\x00"
        fr[o:o + 2] = ((0xFFFF - total_sum()) & 0xFFFF).to_bytes(2, "little")
        return int.from_bytes(fr[o:o + 2], "little")

    ckf = l3 + 16
    if cksum in ("ffff", "alias"):
        assert fix is None and solve(l3 + 18) is not None and total_sum() == 0xFFFF   # with the field still zero
        if cksum == "alias":
            fr[ckf:ckf + 2] = b"\xff\xff"
            assert total_sum() == 0xFFFF
    else:
        c = solve(ckf if fix is None else fix)
        assert tot is not None or total_sum() == 0xFFFF
        if cksum == "zero":
            assert fix is None
            if c == 0:
                fr[l3 + 19] ^= 1
                solve(ckf)
            fr[ckf:ckf + 2] = b"\x00\x00"
        elif cksum == "first":
            fr[l3] ^= 0x01
        elif cksum == "last":
            fr[l3 + seglen - 1] ^= 0x20
    frame = np.frombuffer(bytes(fr), np.uint8)
    o = i * FRAME + HDR + data_off
    m = min(len(frame), (i + 1) * FRAME - o)
    pool.mem[o:o + m] = frame[:m]
    pool.hdr["data_off"][i] = data_off
    pool.hdr["data_len"][i] = (total if data_len is None else data_len) & 0xFFFF
    pool.hdr["tx_offload"][i] = 14 | l3 << 7 | 20 << 16


def run_twin(pool, world: World, bursts, zero_copy: bool, stage_max: int = 2048, md_delta=None, md_null=None):
    """cndp_tcp_input_node_host burst by burst over a copy of the pool (its
    buf_addr fields moved to the copy for the run and back after it): (edges,
    segs, memory).  md_delta / md_null as tests/mq_udp_ref.py's run_twin."""
    from cndp_amd.l4 import tcp_input_node_host
    from cndp_amd.mbuf import FRAME, MBUF_DT
    raw = np.zeros(pool.mem.size + 4096, np.uint8)
    a = (-raw.ctypes.data) % 4096
    mem = raw[a:a + pool.mem.size]
    mem[:] = pool.mem
    delta = np.uint64((mem.ctypes.data - pool.base) % (1 << 64))
    hdr = mem.reshape(pool.n, FRAME)[:, :64].view(MBUF_DT)[:, 0]
    with np.errstate(over="ignore"):
        hdr["buf_addr"] += delta
    hook = None
    if md_delta is not None or md_null is not None:
        b0 = mem.ctypes.data

        def hook(m):
            if md_null is not None and md_null((m - b0) // FRAME):
                return None
            return m + (64 if md_delta is None else md_delta)
    edges, segs = [], []
    for b in bursts:
        for lo in range(0, max(len(b), 1), 256):
            part = b[lo:lo + 256]
            ptrs = (ctypes.c_void_p * max(len(part), 1))(*[None if i is None else mem.ctypes.data + int(i) * FRAME
                                                           for i in part])
            e, s = tcp_input_node_host(world.tbl, ptrs, len(part),
                                       readable_end=mem.ctypes.data + mem.size if zero_copy else None,
                                       stage_max=0 if zero_copy else stage_max, metadata=hook)
            edges.append(e)
            segs.append(s)
    with np.errstate(over="ignore"):
        hdr["buf_addr"] -= delta
    return (np.concatenate(edges) if edges else np.zeros(0, np.uint16),
            np.concatenate(segs) if segs else np.zeros(0, SEG_DT), mem)


def expect(pool, world: World, bursts, zero_copy: bool, stage_max: int = 2048, md_delta=None, md_null=None):
    """What the queue must leave after `bursts` (lists of mbuf indices, None: an
    mbuf outside the region): the restatement's edges, records, counters and pool
    memory, which the host twin run on a copy of the pool must reproduce exactly."""
    from cndp_amd.mbuf import FRAME
    mem = pool.mem.copy()
    md_of = None
    if md_delta is not None or md_null is not None:
        def md_of(mo):
            if md_null is not None and md_null(mo // FRAME):
                return None
            return mo + (64 if md_delta is None else md_delta)
    objs = [None if i is None else int(i) * FRAME for b in bursts for i in b]
    edges, segs, stats = node_ref(mem, pool.base, world.ent, world.users, objs, zero_copy, stage_max, world.punt, md_of)
    t_edges, t_segs, t_mem = run_twin(pool, world, bursts, zero_copy, stage_max, md_delta, md_null)
    assert np.array_equal(t_edges, edges), f"twin edges {t_edges.tolist()} != restatement {edges.tolist()}"
    bad = np.nonzero(t_segs.view(np.uint8).reshape(-1, 16) != segs.view(np.uint8).reshape(-1, 16))[0]
    assert len(bad) == 0, f"twin records differ from the restatement's, first at mbuf {bad[0]}: " \
                          f"{t_segs[bad[0]]} != {segs[bad[0]]}"
    bad = np.nonzero(t_mem != mem)[0]
    assert len(bad) == 0, f"twin memory: {len(bad)} bytes differ from the restatement, first at {bad[0]}"
    return {"edges": edges, "segs": segs, "stats": stats, "mem": mem}


# ---- scenarios shared by the host and the GPU tests ----------------------------
LADDR, OTHER = "10.4.0.7", "10.4.0.9"
PEER, PEER2 = "198.18.0.1", "198.18.0.2"
SEG_LENS = [20, 21, 23, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1460]
NCONN = 72                               # established connections on the listening port 5000


def tcp_hash(laddr: int, faddr: int, ports: int) -> int:
    """pcb_tcp_hash (pcb_internal.h), to find keys that collide on the CPU."""
    M = 0xFFFFFFFF
    x = (laddr * 0x9E3779B1) & M
    x ^= x >> 15
    x = (x + faddr * 0x85EBCA77) & M
    x ^= x >> 13
    x = (x + ports * 0xC2B2AE3D) & M
    x ^= x >> 16
    x = (x * 0x27D4EB2F) & M
    x ^= x >> 15
    return x


def colliding_sports(n_full: int, dport: int = 5001, first: int = 20000):
    """Two foreign ports whose (LADDR, PEER, ports) tuples share a slot of the
    exact-tuple hash when the table holds n_full fully specified entries (HE = the
    power of two at or above 2 * n_full)."""
    from cndp_amd.l4 import addr_net, port_net
    HE = 2
    while HE < 2 * n_full:
        HE <<= 1
    seen = {}
    for sp in range(first, first + 20000):
        h = tcp_hash(addr_net(LADDR), addr_net(PEER), port_net(sp) | port_net(dport) << 16) & (HE - 1)
        if h in seen:
            return seen[h], sp
        seen[h] = sp
    raise AssertionError("no colliding tuples")


def standard_world(max_entries: int = 128) -> World:
    """A wildcard listener and a listener bound to an address on port 5000 with
    NCONN established connections behind them, a deleted connection, a port with
    connections only (5001) holding two tuples that collide in the exact hash,
    user values as a binding's pcb_entry pointers look."""
    w = World(max_entries)
    w.add(lport=5000)                                              # 0 any/any
    w.add(laddr=LADDR, lport=5000)                                 # 1 bound listener
    for k in range(NCONN):                                         # 2 ... NCONN + 1
        w.add(laddr=LADDR, lport=5000, faddr=PEER, fport=40000 + k)
    w.add(laddr=LADDR, lport=5000, faddr=PEER2, fport=40000)       # NCONN + 2, deleted below
    a, b = colliding_sports(NCONN + 3)
    w.add(laddr=LADDR, lport=5001, faddr=PEER, fport=a)            # NCONN + 3
    w.add(laddr=LADDR, lport=5001, faddr=PEER, fport=b)            # NCONN + 4
    w.delete(NCONN + 2)
    w.sports = (a, b)
    for i in (1, 2, 5, NCONN + 4):
        w.user_set(i, 0x7F0000002000 + i * 0x140)
    return w


def fill_lookup(pool):
    """Frames for every lookup class of standard_world; returns the count."""
    a, b = colliding_sports(NCONN + 3)
    cases = [dict(sport=40000), dict(sport=40003), dict(sport=40000 + NCONN - 1),   # connections 2, 5, NCONN + 1
             dict(sport=39999),                                        # only the bound listener (1)
             dict(src=PEER2, sport=40000),                             # the deleted connection: listener 1
             dict(dst=OTHER, sport=40000),                             # only the wildcard listener (0)
             dict(dport=5001, sport=a), dict(dport=5001, sport=b),     # the colliding tuples
             dict(dport=5001, sport=a + 1 if a + 1 != b else a + 2),   # none: connections only
             dict(dport=4999),                                         # none
             dict(dport=0, sport=7)]                                   # the deleted entry answers port 0
    n = 0
    for rep in range(3):
        for c in cases:
            put(pool, n, data_off=192 + 5 * rep, seglen=20 + 7 * rep, **c)
            n += 1
    return n


def fill_mix(pool, seed: int = 5):
    """Every mbuf of the pool: random traffic over standard_world's classes,
    every outcome but the no-metadata one among them."""
    rng = np.random.default_rng(seed)
    for i in range(pool.n):
        r = int(rng.integers(0, 20))
        kw = dict(src=PEER, dst=LADDR, sport=40000 + int(rng.integers(0, NCONN)), dport=5000,
                  seglen=int(rng.choice([20, 24, 33, 100, 300, 1460])), data_off=192 + int(rng.integers(0, 16)),
                  flags=int(rng.choice([0x10, 0x02, 0x11, 0x03, 0x18])))
        if r < 3:
            kw["dport"] = [4999, 5001, 81][r]
        elif r < 6:
            kw["cksum"] = ["first", "last", "zero"][r - 3]
        elif r == 6:
            kw["l3"] = int(rng.choice([24, 60]))
        elif r == 7:                                               # pktmbuf_adjust fails: the ports read as zero, which
            kw.update(seglen=20, data_len=19, clip=19, fix=12)     # the deleted entry answers, and the zeros sum right
        elif r == 8:
            kw.update(seglen=20, data_len=39, clip=39)             # rx_short
        elif r == 9:
            kw.update(nib=int(rng.choice([0, 4])))                 # rx_badoff
        elif r == 10:
            kw.update(nib=15, seglen=int(rng.choice([40, 60, 61])))  # offset 60 above, at and below the segment
        elif r == 11:
            kw.update(dst=OTHER)
        put(pool, i, **kw)


def fill_cksum(pool):
    """The checksum cases over standard_world's connection 2: every length of
    SEG_LENS at mtod alignments 0-15 rotating, good sums, then the first or the
    last byte corrupted; then the special cases.  Returns (mbufs filled, index
    of the first special case)."""
    n = 0
    for kind in ("good", "bad"):
        for li, L in enumerate(SEG_LENS):
            for al in (0, 1, 2, 3, 5, 8, 13, 15):
                ck = "good" if kind == "good" else ("first" if (li + al) & 1 else "last")
                put(pool, n, seglen=L, data_off=192 + al, cksum=ck)
                n += 1
    first_special = n
    specials = [dict(seglen=64, cksum="zero"),                          # 0 a zero field is verified: fails
                dict(seglen=64, cksum="ffff"), dict(seglen=257, cksum="ffff"),   # 1, 2 the right field is zero: passes
                dict(seglen=64, cksum="alias"),                         # 3 0xFFFF where 0x0000 is right: the same sum
                dict(seglen=64, tot=19, data_len=84),                   # 4 total_length below the IHL: fails
                dict(seglen=64, data_len=50),                           # 5 total_length beyond data_len: zeros are read
                dict(seglen=300, data_len=200),                         # 6
                dict(seglen=64, tot=20 + 80),                           # 7 total_length past the segment: what lies behind counts
                dict(seglen=1460, cksum="last"),                        # 8 one flipped bit in the last byte
                dict(seglen=256), dict(seglen=256, cksum="last"),       # 9, 10 what stage_max = 128 clips
                dict(seglen=64, data_len=50, clip=50)]                  # 11 as 5, right over the zeros: passes
    for al in (0, 3, 8, 13):
        for s in specials:
            put(pool, n, data_off=192 + al, **s)
            n += 1
    return n, first_special


def fill_waves(pool):
    """Five waves of 64 mbufs holding exactly 0, 1, 4, 5 and 64 segments that
    hit (and so are summed), the rest misses (port 4999): idle lanes join the
    cooperative sum; every third hit of a wave with several fails.  Returns the
    number of mbufs (320)."""
    n = 0
    for need in (0, 1, 4, 5, 64):
        where = set(range(64)) if need == 64 else set([7, 16, 17, 33, 63][:need])
        for k in range(64):
            if k in where:
                put(pool, n, seglen=40 + k, data_off=192 + k % 16, sport=40000 + k % NCONN,
                    cksum="last" if len(where) > 1 and k % 3 == 1 else "good")
            else:
                put(pool, n, dport=4999, seglen=30)
            n += 1
    return n


def fill_steps(pool):
    """The header steps of cnet_tcp_input's opening, one mbuf each; returns the
    count.  See test_header_steps for what each must give."""
    put(pool, 0, l3=24, seglen=40)                                      # IPOPT
    put(pool, 1, l3=24, seglen=40, nib=4)                               # IPOPT, the batch stage's rx_badoff: zero record
    put(pool, 2, seglen=40, data_len=19, clip=19, fix=12)               # l3_len > data_len: ADJUST (the ports read as zero:
                                                                        # the deleted entry; the sum is right over the zeros)
    put(pool, 3, seglen=40, clip=19, fix=12)
    pool.hdr["buf_len"][3] = 192 + 19                                   # l3_len + data_off > buf_len: ADJUST
    put(pool, 4, seglen=20, data_len=39, clip=39)                       # 19 left: SHORT
    put(pool, 5, seglen=20, data_len=40)                                # 20 left: SEGMENT, data_len 0
    put(pool, 6, seglen=40, nib=4)                                      # offset 16: BADOFF, adj_offset done
    put(pool, 7, seglen=60, nib=15)                                     # offset 60 == segment: SEGMENT
    put(pool, 8, seglen=40, nib=15)                                     # offset 60 <= total_length 60 but > data_len 40 after the adjust: SEGMENT, header unchanged, len wraps
    put(pool, 9, seglen=24, nib=15)                                     # offset 60 > total_length 44: BADOFF, no adj
    put(pool, 10, seglen=21, flags=0x02)                                # SYN: len 2
    put(pool, 11, seglen=20, flags=0x11)                                # FIN | ACK: len 1
    put(pool, 12, seglen=20, flags=0x03)                                # SYN | FIN: len 2
    put(pool, 13, seglen=20, nib=6, flags=0x10)                         # offset 24 > the 20 bytes: len wraps to 0xFFFC
    return 14


def big_world() -> World:
    """A full table of 4096 entries: two listeners on port 5000 and 4094
    connections behind them, every 97th deleted."""
    w = World(4096)
    w.add(lport=5000)
    w.add(laddr=LADDR, lport=5000)
    for k in range(4094):
        w.add(laddr=LADDR, lport=5000, faddr=PEER if k & 1 else PEER2, fport=10000 + k)
    for i in range(2 + 50, 4096, 97):
        w.delete(i)
    w.user_set(4095, 0x7F00DEAD0000)
    return w


def fill_big(pool):
    """Connections spread over big_world's vector, its last entry and deleted
    ones among them, and a key nobody holds."""
    for i in range(pool.n):
        k = (i * 4093 // max(pool.n - 1, 1)) if i % 9 else 50 + 97 * (i // 9)
        put(pool, i, src=PEER if k & 1 else PEER2, sport=10000 + k, seglen=20 + i % 50, data_off=192 + i % 16,
            dport=5000 if i % 31 != 30 else 5003)

"""Python restatement of cnet's ip4_forward node over pktmbuf_t bursts, for the
tests of the mbuf queue's CNDP_MQ_IP4_FORWARD mode and of cndp_fwd_node_host
(include/cndp_mqcnet.h).  Written from the reference's text (CNDP v25.08.0
lib/cnet/ipv4/ip4_forward.c:50-335, pktmbuf.h:955-985): per burst the first
k & ~3 mbufs in groups of four, the rest one by one; per mbuf the destination
load, ipv4_adjust_cksum, pktmbuf_adjust(m, -l2_len), the lookups, the MACs at
the new mtod.  The lookups and the group rules are tests/fwd_ref.py's, imported
unchanged; nothing here shares code with fwd.c or the kernel.

Build-defined where the reference is undefined (include/cndp_mqcnet.h):
 - l2_len > data_off: TTL / checksum edit and edge as usual, no MAC byte, the
   header fields stay;
 - l2_len < 12: the MAC bytes are written after the TTL / checksum bytes;
 - an mbuf that is not taken (zero-copy: it or its frame outside the region)
   keeps its place in its group, hits nothing and comes back EDGE_NONE;
 - bytes at or past the readable end read as zero and are never written: the
   end of the region when zero-copy, buf_addr + buf_len when staged."""
from __future__ import annotations

import numpy as np

from fwd_ref import World, adjust_cksum, four_wide, one_wide, standard_world  # noqa: F401

EDGE_NONE = 0xFFFF
GATEWAY = 0x0400
# pktmbuf_t (pktmbuf.h:102-204)
BUF_ADDR, DATA_OFF, BUF_LEN, DATA_LEN, TX_OFFLOAD = 8, 24, 28, 30, 40
# what a member that is not taken hands to four_wide: an address that must miss
# both FIBs of the world, so that it hits nothing and, as lane 0, has no gateway
MISS_DST_BE = int.from_bytes(bytes([203, 0, 113, 77]), "little")


def _u(mem, o, k):
    return int.from_bytes(mem[o:o + k].tobytes(), "little")


def node_ref(mem: np.ndarray, base: int, w: World, bursts, zero_copy: bool):
    """Run the node over `bursts` (lists of mbuf byte offsets into `mem`, None
    for an mbuf outside the region) on the region `mem`, whose first byte has
    address `base`; `mem` is edited in place.  Returns (edges in submission
    order, [direct, gateway, arp_request])."""
    size = len(mem)
    key = int.from_bytes(MISS_DST_BE.to_bytes(4, "little"), "big")
    assert w.arp_obj(key) is None and w.rt_obj(key) is None
    edges, stats = [], [0, 0, 0]

    def head(mo):
        """:112-115 for one mbuf -> None when it is not taken, else its state."""
        if mo is None or mo < 0 or mo + 64 > size:
            return None
        buf = _u(mem, mo + BUF_ADDR, 8) - base
        doff, blen, dlen = _u(mem, mo + DATA_OFF, 2), _u(mem, mo + BUF_LEN, 2), _u(mem, mo + DATA_LEN, 2)
        l2 = _u(mem, mo + TX_OFFLOAD, 8) & 0x7F
        f = buf + doff
        lim = size if zero_copy else buf + blen
        if zero_copy and not 0 <= f < size:
            return None

        def rd(o):
            return int(mem[o]) if o < lim else 0

        dst = rd(f + 16) | rd(f + 17) << 8 | rd(f + 18) << 16 | rd(f + 19) << 24
        ttl, ck = adjust_cksum(rd(f + 8), rd(f + 10) | rd(f + 11) << 8)
        for o, v in ((f + 8, ttl), (f + 10, ck & 0xFF), (f + 11, ck >> 8)):
            if o < lim:
                mem[o] = v
        eth = None
        if l2 <= doff:                      # pktmbuf_adj_offset(m, -l2_len)
            mem[mo + DATA_OFF:mo + DATA_OFF + 2] = np.frombuffer(((doff - l2) & 0xFFFF).to_bytes(2, "little"), np.uint8)
            mem[mo + DATA_LEN:mo + DATA_LEN + 2] = np.frombuffer(((dlen + l2) & 0xFFFF).to_bytes(2, "little"), np.uint8)
            eth = f - l2
        return {"dst": dst, "eth": eth, "lim": lim}

    def finish(st, res):
        if st is None:
            edges.append(EDGE_NONE)
            return
        edge, nif, ha, kind = res
        stats[{"direct": 0, "gateway": 1, "arp_request": 2}[kind]] += 1
        edges.append(edge | (GATEWAY if kind == "gateway" else 0))
        if ha is None or st["eth"] is None:
            return
        for k, v in enumerate(w.arp[ha][1] + w.mac(nif)):       # d_addr, s_addr
            if 0 <= st["eth"] + k < st["lim"]:   # zero-copy: nothing in front of the region either
                mem[st["eth"] + k] = v

    for objs in bursts:
        k = 0
        while len(objs) - k >= 4:           # :88
            sts = [head(mo) for mo in objs[k:k + 4]]
            res = four_wide(w, [s["dst"] if s is not None else MISS_DST_BE for s in sts])
            for s, r in zip(sts, res):
                finish(s, r)
            k += 4
        while k < len(objs):                # :271
            s = head(objs[k])
            finish(s, one_wide(w, s["dst"]) if s is not None else None)
            k += 1
    return np.array(edges, np.uint16), stats


# ---- the same bursts in the product's pools ---------------------------------
def make_pool(n: int, seed: int = 11):
    """n mbufs laid out like CNDP's, every byte behind the headers random."""
    from cndp_amd.mbuf import FRAME, MbufPool
    pool = MbufPool(n)
    rng = np.random.default_rng(seed)
    pool.mem.reshape(n, FRAME)[:, 64:] = rng.integers(0, 256, (n, FRAME - 64), dtype=np.uint8)
    pool.hdr["udata64"] = 0xABABABABABABABAB
    return pool


def put(pool, i: int, dst: str, ttl: int = 64, l2: int = 14, data_off: int = 192 + 14, ck=None):
    """mbuf i as ip4_input hands it on: an IPv4 header (+ 8 bytes) for `dst` at
    buf_addr + data_off, l2_len = l2 in tx_offload; the bytes in front of the
    header -- where the MACs will go -- stay random."""
    from cndp_amd.mbuf import FRAME, HDR
    from fwd_ref import ip4_frame
    ip = ip4_frame(dst, ttl=ttl, l2=14, ck=ck)[14:42]
    o = i * FRAME + HDR + data_off
    m = min(len(ip), (i + 1) * FRAME - o)
    pool.mem[o:o + m] = ip[:m]
    pool.hdr["data_off"][i] = data_off
    pool.hdr["data_len"][i] = 46
    pool.hdr["tx_offload"][i] = l2 | 20 << 7


def offsets_of(bursts):
    """Bursts of mbuf indices (None: outside the pool) -> bursts of byte offsets."""
    from cndp_amd.mbuf import FRAME
    return [[None if i is None else int(i) * FRAME for i in b] for b in bursts]


def run_twin(pool, tbl, bursts, zero_copy: bool):
    """cndp_fwd_node_host burst by burst over a copy of the pool (its buf_addr
    fields moved to the copy for the run and back after it): (edges, memory)."""
    import ctypes
    from cndp_amd.fwd import node_host
    from cndp_amd.mbuf import FRAME, MBUF_DT
    raw = np.zeros(pool.mem.size + 4096, np.uint8)
    a = (-raw.ctypes.data) % 4096
    mem = raw[a:a + pool.mem.size]
    mem[:] = pool.mem
    delta = np.uint64((mem.ctypes.data - pool.base) % (1 << 64))
    hdr = mem.reshape(pool.n, FRAME)[:, :64].view(MBUF_DT)[:, 0]
    with np.errstate(over="ignore"):
        hdr["buf_addr"] += delta
    edges = []
    for b in bursts:
        ptrs = (ctypes.c_void_p * max(len(b), 1))(*[None if i is None else mem.ctypes.data + int(i) * FRAME for i in b])
        edges.append(node_host(tbl, ptrs, len(b), readable_end=mem.ctypes.data + mem.size if zero_copy else None))
    with np.errstate(over="ignore"):
        hdr["buf_addr"] -= delta
    return np.concatenate(edges) if edges else np.zeros(0, np.uint16), mem


def expect(pool, w: World, tbl, bursts, zero_copy: bool):
    """What the queue must leave after `bursts` (lists of mbuf indices): the
    restatement's edges, counters and pool memory, which the host twin run on a
    copy of the pool must reproduce byte for byte."""
    mem = pool.mem.copy()
    edges, stats = node_ref(mem, pool.base, w, offsets_of(bursts), zero_copy)
    t_edges, t_mem = run_twin(pool, tbl, bursts, zero_copy)
    assert np.array_equal(t_edges, edges), f"twin edges {t_edges.tolist()} != restatement {edges.tolist()}"
    bad = np.nonzero(t_mem != mem)[0]
    assert len(bad) == 0, f"twin memory: {len(bad)} bytes differ from the restatement, first at {bad[0]}"
    return {"edges": edges, "stats": stats, "mem": mem}


# ---- scenarios shared by the host and the GPU tests --------------------------
BURST_SIZES = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256]      # 733 mbufs
L2_LENS = [0, 2, 14, 18, 22]


def split(idx, sizes):
    """Consecutive bursts of the given sizes out of the index list idx."""
    out, pos = [], 0
    for s in sizes:
        out.append(list(idx[pos:pos + s]))
        pos += s
    assert pos == len(idx)
    return out


def fill_random(pool, seed: int, l2s=(14, 18, 22), data_offs=(192 + 22,), dsts=None):
    """Every mbuf of the pool: a destination of fwd_ref.DST_POOL (or dsts), a
    random TTL, l2_len and data_off drawn from the given sets."""
    from fwd_ref import DST_POOL
    dsts = dsts or DST_POOL
    rng = np.random.default_rng(seed)
    for i in range(pool.n):
        put(pool, i, dsts[int(rng.integers(0, len(dsts)))], ttl=int(rng.integers(0, 256)),
            l2=int(l2s[int(rng.integers(0, len(l2s)))]), data_off=int(data_offs[int(rng.integers(0, len(data_offs)))]))


# test_group_rules of tests/test_fwd_gpu.py over mbufs: the taken frames of its
# bursts A-E, then A's four mbufs again as four bursts of one
D, G1, G2, G4, G6 = "10.1.0.2", "10.2.0.5", "10.3.1.1", "10.8.3.3", "10.10.1.1"
X, NR, U = "10.4.1.1", "192.0.2.1", "10.5.1.1"
GROUP_BURSTS = [[D, G1, G2, G4],
                [D, G1, G2, G4, G1],
                [G1, G2, G4, G6, X, NR, G2, U],
                [NR, NR, NR, NR, G1, G2, G4],
                [G1, NR, G2, G4, NR, NR, "10.7.0.1", "10.7.0.2"],
                [D], [G1], [G2], [G4]]
GW = GATEWAY
GROUP_EDGES = [[1 + 2, 1, 1, 1],                                   # A: one direct hit: the routed members go to arp_request
               [1 + 2, 1, 1, 1, 2 + 2 | GW],                       # B: the same, the tail through its gateway
               [2 + 2 | GW, 3 + 2 | GW, 4 + 2 | GW, 0 + 2 | GW,    # C: four gateways, lanes 1-3 with lane 0's ha
                1, 1, 3 + 2 | GW, 1],                              #    lane 0 without a gateway entry: lane 2 its own
               [1, 1, 1, 1, 2 + 2 | GW, 3 + 2 | GW, 4 + 2 | GW],   # D: a tail of three, each its own gateway
               [2 + 2 | GW, 1, 3 + 2 | GW, 4 + 2 | GW, 1, 1, 1, 1],  # E: a member without a route object
               [1 + 2], [2 + 2 | GW], [3 + 2 | GW], [4 + 2 | GW]]  # A one by one: where the reference differs


def fill_groups(pool):
    """GROUP_BURSTS into mbufs 0 ...; returns the bursts of indices."""
    flat = [d for b in GROUP_BURSTS for d in b]
    for i, d in enumerate(flat):
        put(pool, i, d, ttl=64 + i)
    return split(list(range(len(flat))), [len(b) for b in GROUP_BURSTS])


def fill_l2(pool):
    """Every l2_len of L2_LENS at data_off 206 ... 209 (all four alignments of
    the frame), transmitted directly and through a gateway, then l2_len above
    data_off (14 > 10, 127 > 100); returns how many mbufs were filled."""
    i = 0
    for dst in (D, G1, NR):
        for l2 in L2_LENS:
            for doff in (206, 207, 208, 209):
                put(pool, i, dst, ttl=1 + i, l2=l2, data_off=doff)
                i += 1
    for l2, doff in ((14, 10), (127, 100), (1, 0), (22, 21)):
        for dst in (D, G2):
            put(pool, i, dst, ttl=7, l2=l2, data_off=doff)
            i += 1
    return i

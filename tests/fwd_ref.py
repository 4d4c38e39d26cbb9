"""Python restatement of the cnet ip4_forward node for the forwarding tests,
written from the reference's text (CNDP v25.08.0 lib/cnet/ipv4/ip4_forward.c:50-335,
cnet_ipv4.h:159-170, incs/cnet_fib_info.h:52-61,239-251,330-377) burst by burst
and group of four by group of four, the way the node's two loops run.  The
FIBs are plain longest-prefix matches over route lists, so nothing here shares
code, table images or vector tricks with fwd.c or the kernel.

Build-defined where the reference is undefined (include/cndp_fwd.h): a group
member without a route object has no gateway (a miss); lanes 1-3 take lane 0's
gateway entry's ha, their own when lane 0 has none; an unset netif's MAC is six
zero bytes; bytes at or past slab_len read as zero and are never written."""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF
EDGE_NONE = 0xFFFF
ARP_REQUEST = 1
OUTPUT_OFFSET = 2
IP4_INPUT_TYPES = (0x0211, 0x0111, 0x0231, 0x0291)  # p_nxt[] == ip4_input, tests/golden/ptype_ref.json


def bswap32(x: int) -> int:
    return int.from_bytes(int(x & 0xFFFFFFFF).to_bytes(4, "little"), "big")


def adjust_cksum(ttl: int, ck: int):
    """ipv4_adjust_cksum on (time_to_live, hdr_checksum as a little-endian host
    loads it): time_to_live--, cksum = (int32)(ck ^ 0xFFFF) + (int32)htobe16(0xFEFF),
    hdr_checksum = ~(cksum + (cksum >> 16))."""
    c = (ck ^ 0xFFFF) + 0xFFFE        # htobe16((1 << 8) ^ 0xFFFF) on a little-endian host
    return (ttl - 1) & 0xFF, ~(c + (c >> 16)) & 0xFFFF


class RefFib:
    """A FIB as its route list: longest prefix wins, else the default."""

    def __init__(self, default: int):
        self.default = default
        self.routes = {}
        self._memo = {}

    def add(self, ip: int, depth: int, nh: int):
        mask = (0xFFFFFFFF << (32 - depth)) & 0xFFFFFFFF if depth else 0
        self.routes[(ip & mask, depth)] = nh
        self._memo = {}

    def delete(self, ip: int, depth: int):
        mask = (0xFFFFFFFF << (32 - depth)) & 0xFFFFFFFF if depth else 0
        del self.routes[(ip & mask, depth)]
        self._memo = {}

    def lookup(self, ip: int) -> int:
        if ip not in self._memo:
            v = self.default
            for depth in range(32, -1, -1):
                mask = (0xFFFFFFFF << (32 - depth)) & 0xFFFFFFFF if depth else 0
                if (ip & mask, depth) in self.routes:
                    v = self.routes[(ip & mask, depth)]
                    break
            self._memo[ip] = v
        return self._memo[ip]


class World:
    """What the node reads of this_cnet."""

    def __init__(self, arp_cap: int = 64, rt_cap: int = 64):
        self.arp_cap, self.rt_cap = arp_cap, rt_cap
        self.arp_fib = RefFib(arp_cap + 1)      # cnet_arp.c:189-190
        self.rt_fib = RefFib(rt_cap + 1)        # cnet_route4.c:174-175
        self.arp = {}       # idx -> (netif_idx, ha bytes)
        self.rt = {}        # idx -> (gateway s_addr, netif_idx)
        self.netif = {}     # idx -> mac bytes

    # fib_info_lookup: object v & 0xFFFFFF, below the capacity and set
    def arp_obj(self, key: int):
        idx = self.arp_fib.lookup(key) & 0xFFFFFF
        return idx if idx < self.arp_cap and idx in self.arp else None

    def rt_obj(self, key: int):
        idx = self.rt_fib.lookup(key) & 0xFFFFFF
        return idx if idx < self.rt_cap and idx in self.rt else None

    def mac(self, netif: int) -> bytes:
        return self.netif.get(netif, bytes(6))


def one_wide(w: World, dst_be: int):
    """:271-318 -> (edge, netif or None, ARP object written or None, 'direct' / 'gateway' / 'arp_request')."""
    key = bswap32(dst_be)
    a = w.arp_obj(key)
    if a is not None:
        nif = w.arp[a][0]
        return nif + OUTPUT_OFFSET, nif, a, "direct"
    r = w.rt_obj(key)
    if r is not None:
        g = w.arp_obj(w.rt[r][0])
        if g is not None:
            nif = w.rt[r][1]
            return nif + OUTPUT_OFFSET, nif, g, "gateway"
    return ARP_REQUEST, None, None, "arp_request"


def four_wide(w: World, dst_be4):
    """:88-269 for one group of four -> four answers like one_wide's."""
    keys = [bswap32(d) for d in dst_be4]
    res = [(ARP_REQUEST, None, None, "arp_request")] * 4
    arp_fib = [w.arp_obj(k) for k in keys]
    if any(a is not None for a in arp_fib):                     # :134
        for k in range(4):
            if arp_fib[k] is not None:
                nif = w.arp[arp_fib[k]][0]
                res[k] = (nif + OUTPUT_OFFSET, nif, arp_fib[k], "direct")
        return res
    ip_fib = [w.rt_obj(k) for k in keys]
    if any(r is not None for r in ip_fib):                      # :164
        # no route object: gateway[k] is uninitialised there; here no lookup, a miss
        arp_fib = [w.arp_obj(w.rt[r][0]) if r is not None else None for r in ip_fib]
        if any(a is not None for a in arp_fib):                 # :178
            for k in range(4):
                if arp_fib[k] is not None:
                    nif = w.rt[ip_fib[k]][1]
                    # :190,196,202 read arp_fib[0]; NULL there, the lane's own entry here
                    ha = arp_fib[k] if k == 0 or arp_fib[0] is None else arp_fib[0]
                    res[k] = (nif + OUTPUT_OFFSET, nif, ha, "gateway")
    return res


def ip4_forward_ref(slab, n, rxmeta, burst, w: World, sel=None, nh=None, ptype=None, stride=0, offsets=None,
                    data_off=0, n_bins=8, stats=None, slab_len=None) -> dict:
    """The stage's outputs (include/cndp_fwd.h) for one batch; `slab` (a numpy
    uint8 array) is rewritten in place, bounded by slab_len."""
    L = len(slab) if slab_len is None else slab_len
    out = {"fwd_edge": np.full(n, EDGE_NONE, np.uint16), "arp_idx": np.full(n, NONE, np.uint32),
           "bin_of": np.full(n, n_bins + 1, np.uint16),
           "stats": np.zeros(3, np.uint64) if stats is None else np.array(stats, np.uint64)}

    def rd(o):
        return int(slab[o]) if o < L else 0

    def wr(o, v):
        if o < L:
            slab[o] = v

    def frame(i):
        return int(offsets[i] if offsets is not None else i * stride) + data_off

    def is_taken(i):
        if sel is not None:
            return bool(sel[i])
        return int(nh[i]) != NONE and int(nh[i]) >> 24 == 1 and (int(ptype[i]) & 0xFFFF) in IP4_INPUT_TYPES

    def head(i):
        """Everything before the lookups: TTL, checksum; returns dst_addr as loaded."""
        m = frame(i) + (int(rxmeta[i]) & 0x7F)
        ttl, ck = adjust_cksum(rd(m + 8), rd(m + 10) | rd(m + 11) << 8)
        dst = rd(m + 16) | rd(m + 17) << 8 | rd(m + 18) << 16 | rd(m + 19) << 24
        wr(m + 8, ttl)
        wr(m + 10, ck & 0xFF)
        wr(m + 11, ck >> 8)
        return dst

    def finish(i, res):
        edge, nif, ha, kind = res
        out["fwd_edge"][i] = edge
        out["stats"][{"direct": 0, "gateway": 1, "arp_request": 2}[kind]] += 1
        if ha is None:
            out["bin_of"][i] = n_bins
            return
        out["arp_idx"][i] = ha
        out["bin_of"][i] = edge - OUTPUT_OFFSET
        f = frame(i)                                # eth = mtod - l2_len: the frame start
        for k, v in enumerate(w.arp[ha][1]):
            wr(f + k, v)                            # d_addr
        for k, v in enumerate(w.mac(nif)):
            wr(f + 6 + k, v)                        # s_addr

    for b0 in range(0, n, burst):
        objs = [i for i in range(b0, min(n, b0 + burst)) if is_taken(i)]
        k = 0
        while len(objs) - k >= 4:                   # :88
            grp = objs[k:k + 4]
            res = four_wide(w, [head(i) for i in grp])
            for i, r in zip(grp, res):
                finish(i, r)
            k += 4
        while k < len(objs):                        # :271
            i = objs[k]
            finish(i, one_wide(w, head(i)))
            k += 1
    return out


# ---- the same world in the product's tables ---------------------------------
def make_tables(w: World):
    """(arp Fib, rt4 Fib, FwdTable) holding what `w` holds."""
    from cndp_amd import native as N
    from cndp_amd.fib import Fib
    from cndp_amd.fwd import FwdTable
    arp = Fib("arp-fib", N.CNE_FIB_DIR24_8, default_nh=w.arp_fib.default, max_routes=1024,
              nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=256)
    rt4 = Fib("rt4-fib", N.CNE_FIB_DIR24_8, default_nh=w.rt_fib.default, max_routes=1024,
              nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=256)
    for (ip, d), v in w.arp_fib.routes.items():
        assert arp.add(ip, d, v) == 0
    for (ip, d), v in w.rt_fib.routes.items():
        assert rt4.add(ip, d, v) == 0
    tbl = FwdTable(arp, rt4, w.arp_cap, w.rt_cap)
    for i, (nif, ha) in w.arp.items():
        assert tbl.arp_set(i, nif, ha) == 0
    for i, (gw, nif) in w.rt.items():
        assert tbl.rt_set(i, gw, nif) == 0
    for i, mac in w.netif.items():
        assert tbl.netif_set(i, mac) == 0
    return arp, rt4, tbl


def close_tables(arp, rt4, tbl):
    tbl.close()
    arp.close()
    rt4.close()


def ip_h(a: str) -> int:
    """Dotted quad -> host-order integer (what be32toh(dst_addr) gives)."""
    p = [int(x) for x in a.split(".")]
    return p[0] << 24 | p[1] << 16 | p[2] << 8 | p[3]


def standard_world() -> World:
    """A world that reaches every outcome.  Destinations (host order):
       10.1.0.k  k = 1..6   direct ARP entries on netifs 0..5 (object k)
       10.1.0.9             direct ARP entry on netif 7, whose MAC was never set
       10.2.x.x  /16        route 1 via gateway 10.1.0.1 (ARP object 1), netif 2
       10.3.x.x  /16        route 2 via gateway 10.9.0.2 (ARP object 12, netif 5), netif 3
       10.4.x.x  /16        route 3 via a gateway without an ARP entry
       10.5.x.x  /16        route FIB value 5, object not set
       10.6.x.x  /16        route FIB value rt_cap (at capacity)
       10.7.0.1             ARP FIB value 20, object cleared
       10.7.0.2             ARP FIB value arp_cap (at capacity)
       10.8.x.x  /16        route 4 via gateway 10.9.0.4 (ARP object 14), netif 4
       10.10.x.x /16        route 6 via gateway 10.9.0.5 (ARP object 15), netif 0
       anything else        both defaults: arp_request
    Gateways are stored as s_addr and looked up raw: a gateway g has its ARP
    route under the key g itself."""
    w = World(64, 32)
    for k in range(6):
        w.netif[k] = bytes([0x02, 0x11, 0x22, 0x33, 0x44, k])
    for k in range(1, 7):
        w.arp[k] = (k - 1, bytes([0x02, 0xAA, 0, 0, 0, k]))
        w.arp_fib.add(ip_h(f"10.1.0.{k}"), 32, k)
    w.arp[9] = (7, bytes([0x02, 0xAA, 0, 0, 0, 9]))
    w.arp_fib.add(ip_h("10.1.0.9"), 32, 9)
    gw1, gw2, gw3, gw4 = ip_h("10.1.0.1"), ip_h("10.9.0.2"), ip_h("10.9.0.3"), ip_h("10.9.0.4")
    gw5 = ip_h("10.9.0.5")
    w.arp[15] = (2, bytes([0x02, 0xBB, 0, 0, 0, 15]))
    w.arp_fib.add(gw5, 32, 15)
    w.arp[12] = (5, bytes([0x02, 0xBB, 0, 0, 0, 12]))
    w.arp_fib.add(gw2, 32, 12)
    w.arp[14] = (1, bytes([0x02, 0xBB, 0, 0, 0, 14]))
    w.arp_fib.add(gw4, 32, 14)
    for idx, (net, gw, nif) in {1: ("10.2.0.0", gw1, 2), 2: ("10.3.0.0", gw2, 3), 3: ("10.4.0.0", gw3, 0),
                                4: ("10.8.0.0", gw4, 4), 6: ("10.10.0.0", gw5, 0)}.items():
        w.rt[idx] = (gw, nif)
        w.rt_fib.add(ip_h(net), 16, idx)
    w.rt_fib.add(ip_h("10.5.0.0"), 16, 5)
    w.rt_fib.add(ip_h("10.6.0.0"), 16, w.rt_cap)
    w.arp_fib.add(ip_h("10.7.0.1"), 32, 20)
    w.arp_fib.add(ip_h("10.7.0.2"), 32, w.arp_cap)
    return w


DST_POOL = ["10.1.0.1", "10.1.0.2", "10.1.0.3", "10.1.0.6", "10.1.0.9", "10.2.0.5", "10.2.200.1", "10.3.1.1",
            "10.4.1.1", "10.5.1.1", "10.6.1.1", "10.7.0.1", "10.7.0.2", "10.8.3.3", "192.0.2.1", "10.9.0.2", "10.10.1.1"]


def ip4_frame(dst: str, ttl: int = 64, l2: int = 14, src: str = "198.18.0.1", ck=None, size: int = 60) -> np.ndarray:
    """An Ethernet (plain, VLAN for l2 18, QinQ for l2 22) + IPv4 + UDP frame."""
    eth = bytes.fromhex("0200000000010200000000ff")
    tags = {14: b"", 18: b"\x81\x00\x00\x05", 22: b"\x88\xa8\x00\x05\x81\x00\x00\x06"}[l2]
    tot = size - l2
    h = bytearray(20)
    h[0], h[2], h[3], h[8], h[9] = 0x45, tot >> 8, tot & 0xFF, ttl, 17
    h[12:16] = bytes(int(x) for x in src.split("."))
    h[16:20] = bytes(int(x) for x in dst.split("."))
    if ck is None:
        s = sum(h[k] << 8 | h[k + 1] for k in range(0, 20, 2))
        while s >> 16:
            s = (s >> 16) + (s & 0xFFFF)
        ck = ~s & 0xFFFF
        h[10], h[11] = ck >> 8, ck & 0xFF
    else:                       # as a little-endian host would load it
        h[10], h[11] = ck & 0xFF, ck >> 8
    f = eth + tags + b"\x08\x00" + bytes(h) + bytes(8)
    return np.frombuffer((f + bytes(size))[:size], np.uint8)

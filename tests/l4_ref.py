"""Python restatement of ip4_proto + udp_input for the L4 tests: the PCB
best-match rule written from the reference's comment table
(lib/cnet/pcb/cnet_pcb.c:25-37), cne_ipv4_udptcp_cksum_verify
(net/cne_ip.h:131-178, :235-260, :275-349) over a bounded byte view, and the
stage's outputs as include/cndp_l4.h defines them.  Independent of pcb.c and of
the kernels: numpy over the same frames and classify outputs."""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF
CHK = 0x0080
ENTRY_DT = np.dtype([("laddr", "<u4"), ("faddr", "<u4"), ("lport", "<u2"), ("fport", "<u2"), ("flag", "<u2")])
IP4_INPUT_TYPES = (0x0211, 0x0111, 0x0231, 0x0291)  # p_nxt[] == ip4_input, tests/golden/ptype_ref.json


def lookup_ref(ent: np.ndarray, laddr: int, faddr: int, lport: int, fport: int) -> int:
    """One key against the vector `ent` (ENTRY_DT, vector order).

       PCB addr | key addr | type           wildcards
       non-zero | non-zero | exact: must be equal (foreign: the port too)   0
       non-zero | zero     | best                                           1
       zero     | non-zero | best                                           1
       zero     | zero     | nothing to compare                             0
    The first entry with the fewest wildcards wins."""
    if len(ent) == 0:
        return NONE
    ok = ent["lport"] == lport
    e_l, e_f = ent["laddr"] != 0, ent["faddr"] != 0
    if laddr:
        ok &= ~e_l | (ent["laddr"] == laddr)
        wl = ~e_l
    else:
        wl = e_l
    if faddr:
        ok &= ~e_f | ((ent["faddr"] == faddr) & (ent["fport"] == fport))
        wf = ~e_f
    else:
        wf = e_f
    if not ok.any():
        return NONE
    score = (wl.astype(np.int64) + wf.astype(np.int64)) * (len(ent) + 1) + np.arange(len(ent))
    score[~ok] = np.iinfo(np.int64).max
    return int(np.argmin(score))


class View:
    """The batch's bounded view: bytes at or past the slab's end read as zero."""

    def __init__(self, slab: np.ndarray):
        self.s = slab
        self.n = len(slab)

    def rd(self, o: int, k: int) -> np.ndarray:
        out = np.zeros(k, np.uint8)
        if o < self.n and k:
            m = min(k, self.n - o)
            out[:m] = self.s[o:o + m]
        return out


def _fold(s: int) -> int:
    return (s >> 16) + (s & 0xFFFF)


def raw_cksum(b: np.ndarray) -> int:
    """cne_raw_cksum: host-order (little-endian) 16-bit words, a last odd byte
    as the low byte of a final word, two folds."""
    w = b[:len(b) & ~1].astype(np.int64)
    s = int(w[0::2].sum() + 256 * w[1::2].sum())
    if len(b) & 1:
        s += int(b[-1])
    return _fold(_fold(s & 0xFFFFFFFF)) & 0xFFFF


def cksum_verify(view: View, ip_off: int, l3_len: int) -> bool:
    """cne_ipv4_udptcp_cksum_verify(ip, ip + l3_len) == 0."""
    ip = view.rd(ip_off, 20)
    ihl = (int(ip[0]) & 0xF) * 4
    tot = int(ip[2]) << 8 | int(ip[3])
    if tot < ihl:
        return False        # __ipv4_udptcp_cksum returns 0, not 0xffff
    l4 = tot - ihl
    ck = raw_cksum(view.rd(ip_off + l3_len, l4))
    psd = np.concatenate([ip[12:20], np.array([0, ip[9], (l4 >> 8) & 0xFF, l4 & 0xFF], np.uint8)])
    ck += raw_cksum(psd)
    return (_fold(ck) & 0xFFFF) == 0xFFFF


def udp_input_ref(slab, n, nh, rxmeta, ent, ptype=None, sel=None, stride=0, offsets=None, data_off=0,
                  punt=True, tcp=False, n_bins=None, stats=None) -> dict:
    """The stage's outputs (include/cndp_l4.h) for one batch."""
    view = View(np.asarray(slab, np.uint8))
    n_bins = max(1, len(ent)) if n_bins is None else n_bins
    out = {"l4edge": np.full(n, 0xFF, np.uint8), "pcb": np.full(n, NONE, np.uint32),
           "ports": np.zeros(n, np.uint32), "payload_off": np.zeros(n, np.uint16),
           "bin_of": np.full(n, n_bins + 1, np.uint16),
           "stats": np.zeros(4, np.uint64) if stats is None else np.array(stats, np.uint64)}
    for i in range(n):
        if sel is not None:
            if not sel[i]:
                continue
        elif not (int(nh[i]) != NONE and int(nh[i]) >> 24 == 2 and (int(ptype[i]) & 0xFFFF) in IP4_INPUT_TYPES):
            continue
        rx = int(rxmeta[i])
        l2, l3, l4 = rx & 0x7F, (rx >> 7) & 0x1FF, (rx >> 16) & 0xFF
        m = int(offsets[i] if offsets is not None else i * stride) + data_off + l2
        ip = view.rd(m, 20)
        proto = int(ip[9])
        if proto != 17:                       # ip4_proto
            if proto == 6 and tcp:
                out["l4edge"][i] = 0x02
            else:
                out["l4edge"][i] = 0x00
                out["bin_of"][i] = n_bins
                out["stats"][3] += 1
            continue
        udp = view.rd(m + l3, 8)
        faddr, laddr = int(ip[12:16].view("<u4")[0]), int(ip[16:20].view("<u4")[0])
        fport, lport = int(udp[0:2].view("<u2")[0]), int(udp[2:4].view("<u2")[0])
        out["ports"][i] = fport | lport << 16
        p = lookup_ref(ent, laddr, faddr, lport, fport)
        if p == NONE:
            out["l4edge"][i] = 0x12 if punt else 0x10
            if not punt:
                out["bin_of"][i] = n_bins
            out["stats"][1] += 1
            continue
        if (int(ent["flag"][p]) & CHK) and (udp[6] or udp[7]) and not cksum_verify(view, m, l3):
            out["l4edge"][i] = 0x10
            out["bin_of"][i] = n_bins
            out["stats"][2] += 1
            continue
        out["l4edge"][i] = 0x11
        out["pcb"][i] = p
        out["bin_of"][i] = p
        out["payload_off"][i] = l2 + l3 + l4
        out["stats"][0] += 1
    return out


def random_table(rng, n, addrs, ports, deleted_frac=0.05):
    """n entries from a small pool (collisions are common): any/any listeners,
    bound and connected sockets, duplicates, entries that differ only in
    fport; returns (ENTRY_DT array as the vector holds it, indices to delete)."""
    ent = np.zeros(n, ENTRY_DT)
    for i in range(n):
        kind = rng.integers(0, 6)
        ent["lport"][i] = ports[rng.integers(0, len(ports))]
        if kind >= 1:
            ent["laddr"][i] = addrs[rng.integers(0, len(addrs))]
        if kind >= 3:
            ent["faddr"][i] = addrs[rng.integers(0, len(addrs))]
            ent["fport"][i] = ports[rng.integers(0, len(ports))]
        if kind == 5 and i:            # a copy of an earlier entry, sometimes with another fport
            ent[i] = ent[rng.integers(0, i)]
            if rng.integers(0, 2):
                ent["fport"][i] = ports[rng.integers(0, len(ports))]
        ent["flag"][i] = CHK if rng.integers(0, 2) else 0
    dele = np.nonzero(rng.random(n) < deleted_frac)[0]
    return ent, dele


def fill_table(tbl, ent, dele=()):
    """Add `ent` to a PcbTable, delete `dele`; returns the vector as it is then."""
    for e in ent:
        assert tbl.add_raw(int(e["laddr"]), int(e["faddr"]), int(e["lport"]), int(e["fport"]), int(e["flag"])) >= 0
    ent = ent.copy()
    for i in dele:
        assert tbl.delete(int(i)) == 0
        ent[int(i)] = 0
    return ent

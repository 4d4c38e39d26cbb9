"""Python restatement of tcp_input for the TCP tests, written from the
reference's text: tcp_input_lookup (lib/cnet/tcp/tcp_input.c:41-119: key from
the IPv4 header at mtod and the TCP ports at mtod + l3_len, ports stored, then a
best-match lookup, the checksum verify on every hit, punt or drop on a miss) and
the state-free opening of cnet_tcp_input (lib/cnet/tcp/cnet_tcp.c:3386-3414:
offset, the rx_badoff test, the seg fields, len in uint16_t arithmetic), with
the stage's outputs as include/cndp_tcp.h defines them.  Independent of pcb.c
and of the kernels; the lookup rule, the bounded view and the checksum are
l4_ref's."""
from __future__ import annotations

import numpy as np

from l4_ref import NONE, View, cksum_verify, lookup_ref

SEG_DT = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("wnd", "<u2"), ("urp", "<u2"), ("len", "<u2"),
                   ("flags", "u1"), ("offset", "u1")])
TAKE = 0x02                                   # ip4_proto's tcp edge, as udp_input reports it
E_DROP, E_SEG, E_PUNT = 0x20, 0x21, 0x22      # node 2 << 4 | tcp_input_priv.h's edge
S_SEG, S_NOMATCH, S_CKSUM, S_BADOFF = 0, 1, 2, 3
TCP_MASK, SYN_FIN = 0x3F, 0x03
SYN_FIN_CNT = (0, 1, 1, 2)                    # tcp_syn_fin_cnt, cnet_tcp.c:3338


def be(b) -> int:
    return int.from_bytes(bytes(b), "big")


def tcp_input_ref(slab, n, rxmeta, ent, l4edge=None, sel=None, stride=0, offsets=None, data_off=0,
                  punt=True, n_bins=None, stats=None) -> dict:
    """The stage's outputs for one batch.  l4edge: udp_input's array (copied);
    without sel, its TAKE entries are the frames taken."""
    view = View(np.asarray(slab, np.uint8))
    n_bins = max(1, len(ent)) if n_bins is None else n_bins
    out = {"l4edge": np.full(n, 0xFF, np.uint8) if l4edge is None else np.array(l4edge, np.uint8),
           "pcb": np.full(n, NONE, np.uint32), "ports": np.zeros(n, np.uint32),
           "seg": np.zeros(n, SEG_DT), "bin_of": np.full(n, n_bins + 1, np.uint16),
           "stats": np.zeros(5, np.uint64) if stats is None else np.array(stats, np.uint64)}
    for i in range(n):
        if sel is not None:
            if not sel[i]:
                continue
        elif out["l4edge"][i] != TAKE:
            continue
        rx = int(rxmeta[i])
        l2, l3 = rx & 0x7F, (rx >> 7) & 0x1FF
        m = int(offsets[i] if offsets is not None else i * stride) + data_off + l2
        ip, tcp = view.rd(m, 20), view.rd(m + l3, 20)
        faddr, laddr = int(ip[12:16].view("<u4")[0]), int(ip[16:20].view("<u4")[0])
        fport, lport = int(tcp[0:2].view("<u2")[0]), int(tcp[2:4].view("<u2")[0])
        out["ports"][i] = fport | lport << 16
        p = lookup_ref(ent, laddr, faddr, lport, fport)
        if p == NONE:
            out["l4edge"][i] = E_PUNT if punt else E_DROP
            if not punt:
                out["bin_of"][i] = n_bins
            out["stats"][S_NOMATCH] += 1
            continue
        if not cksum_verify(view, m, l3):          # always: no zero-field exemption for TCP
            out["l4edge"][i] = E_DROP
            out["bin_of"][i] = n_bins
            out["stats"][S_CKSUM] += 1
            continue
        out["pcb"][i] = p                           # m->userptr = pcb, then cnet_tcp_input
        tlen = be(ip[2:4])
        offset = (int(tcp[12]) & 0xF0) >> 2
        if offset < 20 or offset > tlen:
            out["l4edge"][i] = E_DROP
            out["bin_of"][i] = n_bins
            out["stats"][S_BADOFF] += 1
            continue
        flags = int(tcp[13]) & TCP_MASK
        tl16 = (tlen - (offset + l3)) & 0xFFFF      # uint16_t tlen -= ...
        out["seg"][i] = (be(tcp[4:8]), be(tcp[8:12]), be(tcp[14:16]), be(tcp[18:20]),
                         (tl16 + SYN_FIN_CNT[flags & SYN_FIN]) & 0xFFFF, flags, offset)
        out["l4edge"][i] = E_SEG
        out["bin_of"][i] = p
        out["stats"][S_SEG] += 1
    return out


def outcome(ent, laddr, faddr, lport, fport) -> str:
    """Which path of the indexed lookup a key's answer comes from, by the linear
    rule alone: 'exact', 'wild1', 'wild2' or 'miss'."""
    p = lookup_ref(ent, laddr, faddr, lport, fport)
    if p == NONE:
        return "miss"
    e = ent[p]
    w = int((e["laddr"] != 0) != (laddr != 0)) + int((e["faddr"] != 0) != (faddr != 0))
    return ("exact", "wild1", "wild2")[w]

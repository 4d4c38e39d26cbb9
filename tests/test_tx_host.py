"""Host side of the transmit stage (include/cndp_tx.h, cndp_amd/csrc/tx.c): the
restatement's two checksum steps against the reference's own recorded results
(tests/golden/ip4_output_cksum_ref.npz, tools/gen_ip4_output_golden.py), the
argument checks, the defaults of a new PCB entry and a new table's counters,
cndp_tx_output_host against the Python restatement (tests/tx_ref.py) -- slab
byte for byte, edges, bins, counters, identification counters -- on tables
built to reach every outcome and at every headroom around the three prepends,
the new exports, and tx.c under the address / undefined-behaviour sanitizers in
a stand-alone program.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd import tx as T
from cndp_amd.l4 import PcbTable

import fwd_ref as F
import tx_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ip4_output_cksum_ref.npz")
HEADROOMS = [7, 8, 27, 28, 41, 42, 43, 256]


def test_cksum_restatement_against_reference_golden():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 512 * 1024
    kinds = g["kind"].tolist()
    n = len(kinds)
    assert n >= 300 and set(g["proto"].tolist()) == {6, 17}
    for proto, want in ((17, 0xFFFF), (6, 0)):      # a regenerated file cannot silently lose these
        zs = [i for i in range(n) if kinds[i].startswith("zero-sum") and g["proto"][i] == proto]
        assert len(zs) >= 8 and all(int(g["l4_cksum"][i]) == want for i in zs), proto
    lens = {(int(g["proto"][i]), int(g["off"][i + 1] - g["off"][i]) - 20) for i in range(n)}
    assert lens >= {(p, l) for p in (6, 17) for l in (8, 9, 10, 11, 23, 24, 25, 63, 64, 65, 255, 256, 257, 1471,
                                                      1472, 1480)}
    for i in range(n):
        s = g["data"][g["off"][i]:g["off"][i + 1]]
        assert R.ipv4_cksum(s[:20]) == int(g["ip_cksum"][i]), kinds[i]
        assert R.udptcp_cksum(s[:20], s[20:]) == int(g["l4_cksum"][i]), kinds[i]


def _tables(netifs=5):
    tw = R.standard_world(netifs)
    return tw, R.make_tables(tw)


def test_argument_checks():
    L = N.lib()
    tw, (arp, rt4, fwd, pt) = _tables()
    try:
        a = N.PcbTx(1, 2, 3)
        cnt = pt.count()
        assert L.cndp_pcb_tx_set(None, 0, ctypes.byref(a)) == -22 and L.cndp_pcb_tx_set(pt.h, 0, None) == -22
        assert L.cndp_pcb_tx_get(None, 0, ctypes.byref(a)) == -22 and L.cndp_pcb_tx_get(pt.h, 0, None) == -22
        assert T.pcb_tx_set(pt, cnt, 0, 1, 17) == -22 and T.pcb_tx_get(pt, cnt) == -22      # outside the vector
        assert T.pcb_tx_set(pt, 35, 0, 1, 17) == -2 and T.pcb_tx_get(pt, 35) == -2          # deleted: -ENOENT
        v = ctypes.c_uint16()
        assert L.cndp_fwd_netif_ident_set(None, 0, 1) == -22 and L.cndp_fwd_netif_ident_set(fwd.h, 256, 1) == -22
        assert L.cndp_fwd_netif_ident_get(None, 0, ctypes.byref(v)) == -22
        assert L.cndp_fwd_netif_ident_get(fwd.h, 256, ctypes.byref(v)) == -22
        assert L.cndp_fwd_netif_ident_get(fwd.h, 0, None) == -22
        assert T.ident_set(fwd, 255, 0x1234) == 0 and T.ident_get(fwd, 255) == 0x1234

        n = 4
        slab = np.zeros(n * 128, np.uint8)
        u32, u16 = np.zeros(n, np.uint32), np.zeros(n, np.uint16)
        io = N.TxIo()
        io.pcb = io.faddr = io.laddr = io.ports = u32.ctypes.data
        io.len = io.tx_edge = u16.ctypes.data

        def host(ft=fwd.h, p=pt.h, mode=N.CNDP_TX_UDP, s=slab.ctypes.data, io_=io, n_=n):
            return L.cndp_tx_output_host(ft, p, mode, s, len(slab), 128, None, 64, n_, ctypes.byref(io_) if io_ else None)

        assert host() == 0
        assert host(ft=None) == -22 and host(p=None) == -22 and host(mode=2) == -22 and host(io_=None) == -22
        assert host(s=None) == -22 and host(s=None, n_=0) == 0
        for field in ("pcb", "faddr", "laddr", "ports", "len", "tx_edge"):
            bad = N.TxIo.from_buffer_copy(io)
            setattr(bad, field, None)
            want = 0 if field == "ports" else -22
            assert host(io_=bad, mode=N.CNDP_TX_IP4) == want, field
            assert host(io_=bad) == -22, field
        bins = N.TxIo.from_buffer_copy(io)
        bins.bin_of = u16.ctypes.data
        for nb, want in ((7, -22), (8, 0), (65533, 0), (65534, -22)):   # the table's largest netif is 7
            bins.n_bins = nb
            assert host(io_=bins) == want, nb
        # the device call refuses the same things before it touches a device
        assert L.cndp_gpu_ip4_output(None, None, None, None, 0, None, None) == -22
    finally:
        R.close_tables(arp, rt4, fwd, pt)


def test_defaults():
    arp = F.World(4, 4)
    a, r, fwd = F.make_tables(arp)
    pt = PcbTable(4)
    try:
        assert [T.ident_get(fwd, k) for k in (0, 1, 255)] == [0, 0, 0]      # the reference seeds from rdtsc
        assert pt.add(laddr="10.0.0.1", lport=7) == 0
        assert T.pcb_tx_get(pt, 0) == (0, 64, 17)       # TOS_DEFAULT, TTL_DEFAULT, UDP
        assert T.pcb_tx_set(pt, 0, 0x10, 9, 6) == 0 and T.pcb_tx_get(pt, 0) == (0x10, 9, 6)
        assert pt.add(laddr="10.0.0.1", lport=8) == 1 and T.pcb_tx_get(pt, 1) == (0, 64, 17)   # added after a look
        assert pt.delete(0) == 0 and T.pcb_tx_get(pt, 0) == -2
        assert T.pcb_tx_get(pt, 1) == (0, 64, 17)
    finally:
        pt.close()
        F.close_tables(a, r, fwd)


def _ident(tw):
    return [tw.ident.get(k, 0) for k in range(256)]


@pytest.mark.parametrize("mode", [R.TX_UDP, R.TX_IP4])
@pytest.mark.parametrize("headroom", HEADROOMS)
def test_host_equals_restatement(headroom, mode):
    tw, (arp, rt4, fwd, pt) = _tables()
    try:
        n = 300
        pcb, faddr, laddr, ports, length = R.make_inputs(n, tw, seed=headroom * 2 + mode)
        kind = ("packed", "imix", "umem")[headroom % 3]
        if mode == R.TX_IP4:
            length = (length + 20).astype(np.uint16)    # the L4 header is counted
        buf, slab_len, stride, offs, data_off, length = R.layout(kind, length, headroom, seed=headroom, guard=64)
        want_slab = buf.copy()
        sel = None
        stats = None
        for call in range(2):       # the second continues from the first's counters
            got = T.output_host(fwd, pt, buf, n, pcb, faddr, laddr, ports if mode == R.TX_UDP else None, length,
                                mode=mode, stride=stride, offsets=offs, data_off=data_off, sel=sel, n_bins=8,
                                slab_len=slab_len, stats=stats)
            want = R.ip4_output_ref(want_slab, n, tw, pcb, faddr, laddr, ports, length, mode=mode, stride=stride,
                                    offsets=offs, data_off=data_off, sel=sel, n_bins=8, stats=stats,
                                    slab_len=slab_len)
            for k in ("tx_edge", "bin_of", "stats"):
                assert np.array_equal(got[k], want[k]), (call, k, got[k][:16], want[k][:16])
            bad = np.nonzero(buf != want_slab)[0]
            assert len(bad) == 0, f"call {call}: {len(bad)} bytes differ, first at {bad[0]}"
            assert [T.ident_get(fwd, k) for k in range(256)] == _ident(tw)
            assert (buf[slab_len:] == 0xA5).all()
            sel = (np.arange(n) % 3 == 0).astype(np.uint8)
            stats = got["stats"]
        st = want["stats"]
        need = 42 if mode == R.TX_UDP else 34
        if headroom >= need:        # every outcome but the headroom drop; the counters wrapped
            assert st[R.SENT] and st[R.ARP_REQ] and st[R.DROP_NOROUTE] and st[R.DROP_PROTO] and st[R.CKSUM]
            assert st[R.DROP_HEADROOM] == 0 and st[R.CKSUM] < st[R.SENT] + st[R.ARP_REQ]
            assert any(v < 0xFFF0 for v in tw.ident.values())
            assert (want["tx_edge"] == R.EDGE_NONE).sum() > 0
        else:
            assert st[R.SENT] == 0 and st[R.DROP_HEADROOM] > 0 and _ident(tw)[:6] == [0xFFF0 + k for k in range(6)]
            # with room for the IPv4 header a frame without a route is dropped for that
            assert (st[R.DROP_NOROUTE] > 0) == (headroom >= need - 14)
    finally:
        R.close_tables(arp, rt4, fwd, pt)


def test_untouched_bytes_and_field_values():
    """Spelt out on single frames: the bytes of a sent frame, d_addr left alone on
    an ARP miss, packet_id left alone without a route, the counter's step."""
    tw, (arp, rt4, fwd, pt) = _tables()
    try:
        pay = 18
        for faddr, laddr, pcb_i, what in (("10.1.0.2", "10.3.0.7", 34, "sent"), ("192.0.2.1", "10.3.0.7", 34, "arp"),
                                          ("10.1.0.2", "10.1.0.1", 4, "noroute")):
            buf = np.full(128, 0xEE, np.uint8)
            buf[64:64 + pay] = np.arange(pay)
            before = T.ident_get(fwd, 3)
            got = T.output_host(fwd, pt, buf, 1, [pcb_i], [R.ip_n(faddr)], [R.ip_n(laddr)],
                                [R.bswap16(4000) | tw.pcbs[pcb_i].lport << 16], [pay], stride=128, data_off=64,
                                n_bins=8)
            f = bytes(buf[22:64])
            assert bytes(buf[:22]) == b"\xEE" * 22 and bytes(buf[64:64 + pay]) == bytes(range(pay))
            if what == "noroute":
                assert got["tx_edge"][0] == 0 and f[:14] == b"\xEE" * 14 and f[18:20] == b"\xEE\xEE"
                assert f[14:18] == bytes([0x45, 0, 0, 46]) and f[24:26] == b"\0\0" and T.ident_get(fwd, 3) == before
                continue
            assert f[6:14] == tw.w.netif[3] + b"\x08\x00"
            assert f[14:18] == bytes([0x45, 0xB8, 0, 46]) and f[18:20] == before.to_bytes(2, "big")
            assert f[20:24] == bytes([0, 0, 1, 17]) and f[26:30] == bytes([10, 3, 0, 7])
            assert f[34:42] == (82).to_bytes(2, "big") + (4000).to_bytes(2, "big") + (26).to_bytes(2, "big") + f[40:42]
            assert R.raw_cksum(f[14:34]) == 0xFFFF      # the header verifies
            psd = f[26:34] + bytes([0, 17, 0, 26])
            assert R.raw_cksum(psd + f[34:] + bytes(range(pay))) == 0xFFFF      # and so does the datagram
            assert T.ident_get(fwd, 3) == (before + R.bswap16(46)) & 0xFFFF     # total_length as loaded: 0x2E00
            if what == "sent":
                assert got["tx_edge"][0] == 3 + 2 and got["bin_of"][0] == 3 and f[:6] == tw.w.arp[2][1]
            else:
                assert got["tx_edge"][0] == 1 and got["bin_of"][0] == 8 and f[:6] == b"\xEE" * 6
    finally:
        R.close_tables(arp, rt4, fwd, pt)


def test_tx_header_exports():
    """Every function include/cndp_tx.h declares is exported by the built library."""
    names = N.l4_exported_symbols("cndp_tx.h")
    assert set(names) == {"cndp_pcb_tx_set", "cndp_pcb_tx_get", "cndp_fwd_netif_ident_set",
                          "cndp_fwd_netif_ident_get", "cndp_gpu_ip4_output", "cndp_tx_output_host"}
    L = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert hasattr(L, nm), nm


def test_launch_geometry_constants():
    """cndp_amd.tx names the block size the GPU tests size their largest batch by."""
    import re
    src = open(os.path.join(HERE, "..", "cndp_amd", "csrc", "cndp_tx.hip")).read()
    assert int(re.search(r"#define TX_BLOCK (\d+)u", src).group(1)) == T.TX_BLOCK
    assert int(re.search(r"#define TX_BLOCKS_PER_CU (\d+)u", src).group(1)) == T.TX_BLOCKS_PER_CU


def test_tx_under_sanitizers():
    """tests/tx_host/tx_san: tx.c (over pcb.c, fwd.c, fib.c, rib.c) built with
    -fsanitize=address,undefined in a program of its own, run as a child process."""
    d = os.path.join(HERE, "tx_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "tx_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    flags = open(os.path.join(d, "Makefile")).read()
    assert "-fsanitize=address,undefined" in flags

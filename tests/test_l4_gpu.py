"""UDP socket demux on the GPU (cndp_gpu_udp_input, include/cndp_l4.h): every
output array and the counters must equal the Python restatement
(tests/l4_ref.py) applied to the same frames and to the cnet classify outputs
the stage itself read.  Shapes are the smallest that can still go wrong: one
frame, a wave and its neighbours, more than one block, more blocks than fit
the grid's first trip; packed slots, the UMEM stride, odd byte offsets; tables
from empty to full, one long run, all-distinct ports."""
import os

import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd import pktgen
from cndp_amd.l4 import PcbTable, addr_net, port_net

import l4_ref as R
from helpers import cnet_fibs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FOREIGN = [(0xC6120001, 9), (0xC6120002, 53), (0xC6120001, 5000)]
PORTS_H = (9, 53, 5000, 5001, 65535)
UDT = {"l4edge": np.uint8, "pcb": np.uint32, "ports": np.uint32, "payload_off": np.uint16,
       "bin_of": np.uint16, "stats": np.uint64}


@pytest.fixture(scope="module")
def cnet(gpu):
    from cndp_amd.classify import Classifier
    fib, fib6, routes, v6, v4vals, v6vals = cnet_fibs()
    cl = Classifier(0)
    cl.set_fib(fib, fib6)
    local = [ip for ip, d, _ in routes if d == 32]      # ip4_input's proto edge
    other = [routes[0][0] | 5, routes[1][0] | 9]        # forwarded, never taken
    assert len(local) >= 8
    yield cl, local, other
    cl.close()


def pools(local):
    addrs = [addr_net(a) for a in local[:4]] + [addr_net(a) for a, _ in FOREIGN[:2]]
    return addrs, [port_net(p) for p in PORTS_H]


def sockets(local, other=()):
    # 4444 is nobody's port: those frames find no PCB
    return [(a, p) for a in list(local[:5]) + list(other) for p in PORTS_H[:4]] + [(local[0], 4444)]


def classify(cl, fr):
    # a fresh ptype-node state: a state left on a type whose edge is pkt_drop (an ICMP
    # frame of an earlier batch) would send every quiet 4-group of this one there
    cl.set_tuning(cnet_spec=256)
    out = cl.alloc_outputs(fr.n, 64, device=fr.slab.device, meta=True)
    cl.classify(fr, N.CNDP_MODE_CNET, out=out)
    return out


def host(t, dt):
    return t.cpu().numpy().view(dt)


def check(cl, fr, tbl, ent, out=None, sel=None, punt=True, tcp=False, n_bins=None, l4=None, stats0=None):
    """One call of the stage against the restatement; returns (got, want)."""
    out = classify(cl, fr) if out is None else out
    sel_t = torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).to(fr.slab.device) if sel is not None else None
    got_t = cl.udp_input(fr, out, tbl, sel=sel_t, n_bins=n_bins, l4=l4)
    torch.cuda.synchronize()
    got = {k: host(got_t[k], dt) for k, dt in UDT.items()}
    offs = fr.offsets.cpu().numpy() if fr.offsets is not None else None
    want = R.udp_input_ref(fr.slab.cpu().numpy(), fr.n, host(out["nh"], np.uint32), host(out["rxmeta"], np.uint32),
                           ent, ptype=host(out["ptype"], np.uint32), sel=sel, stride=fr.stride, offsets=offs,
                           data_off=fr.data_off, punt=punt, tcp=tcp, n_bins=got_t["n_bins"], stats=stats0)
    for k in UDT:
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, (f"{k}: {len(bad)} differ, first at {bad[0]}: got {got[k][bad[0]]:#x} "
                               f"want {want[k][bad[0]]:#x}")
    return got, want


def make_table(rng, n, local, ports=None, cap=None):
    addrs, pp = pools(local)
    tbl = PcbTable(cap or max(n, 1))
    ent, dele = R.random_table(rng, n, addrs, ports or pp, deleted_frac=0.05)
    return tbl, R.fill_table(tbl, ent, dele)


LAYOUTS = {"packed": dict(layout="packed", slot=128), "umem": dict(layout="umem"),
           "odd": dict(layout="offsets", align=1)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_sizes_and_layouts(cnet, gpu, n, layout):
    cl, local, other = cnet
    rng = np.random.default_rng(n)
    tbl, ent = make_table(rng, 512, local)
    try:
        fr = pktgen.udp_socket_frames(n, sockets(local, other), FOREIGN, seed=n, device=gpu,
                                      payload_lens=(0, 1, 7, 8, 9, 55, 56, 57), ihl=(5, 5, 6, 15), vlan_frac=0.2,
                                      cksum=("ok", "bad", "zero"), proto=(17, 17, 17, 17, 6, 1), **LAYOUTS[layout])
        got, want = check(cl, fr, tbl, ent)
        if n >= 63:
            assert want["stats"][0] and (want["l4edge"] == 0xFF).any()
        if n >= 257:   # the larger batches reach every outcome
            assert want["stats"].all()
    finally:
        tbl.close()


@pytest.mark.parametrize("case", ["empty", "one", "full", "one_port", "distinct512", "distinct4096"])
def test_table_shapes(cnet, gpu, case):
    """Table sizes 0, 1 and 4096 from the collision-heavy pool; 512 entries on
    one port (the longest run); 512 and 4096 distinct ports (the directory; the
    last stages more than 64 KiB of LDS)."""
    cl, local, other = cnet
    rng = np.random.default_rng(7)
    addrs, pp = pools(local)
    socks = sockets(local)
    if case in ("empty", "full"):
        tbl, ent = make_table(rng, {"empty": 0, "full": 4096}[case], local)
    elif case == "one":
        tbl = PcbTable(1)
        ent = R.fill_table(tbl, np.array([(addrs[0], 0, pp[2], 0, R.CHK)], R.ENTRY_DT))
    elif case == "one_port":
        tbl, ent = make_table(rng, 512, local, ports=[pp[2]])
    else:
        k = 512 if case == "distinct512" else 4096
        ports = rng.permutation(65535)[:k] + 1
        ent = np.zeros(k, R.ENTRY_DT)
        ent["lport"] = [port_net(int(p)) for p in ports]
        ent["laddr"] = rng.choice(addrs[:4] + [0], k)
        ent["flag"] = rng.choice([0, R.CHK], k)
        tbl = PcbTable(k)
        ent = R.fill_table(tbl, ent)
        socks = [(local[i % 4], int(p)) for i, p in enumerate(ports[:: max(1, k // 64)])] + [(local[0], 0)]
    try:
        fr = pktgen.udp_socket_frames(257, socks, FOREIGN, seed=11, device=gpu, payload_lens=(0, 3, 18),
                                      cksum=("ok", "bad"), layout="packed", slot=128)
        got, want = check(cl, fr, tbl, ent)
        if case not in ("empty",):
            assert want["stats"][0] > 0
        if case == "empty":
            assert want["stats"][1] == (want["l4edge"] != 0xFF).sum()
    finally:
        tbl.close()


def test_checksum_cases(cnet, gpu):
    """Flag on and off per socket, zero / correct / corrupted sums, the golden
    file's lengths (L4 8..65 and 1472), IHL 5-15, a VLAN tag, odd addresses."""
    cl, local, other = cnet
    addrs, pp = pools(local)
    ent = np.zeros(8, R.ENTRY_DT)
    for i in range(8):      # sockets on local[i % 4]: port 5000 with the flag, 5001 without
        ent[i] = (addrs[i % 4], 0, pp[2 + i // 4], 0, R.CHK if i < 4 else 0)
    tbl = PcbTable(8)
    try:
        ent = R.fill_table(tbl, ent)
        socks = [(a, p) for a in local[:4] for p in (5000, 5001)]
        fr = pktgen.udp_socket_frames(330, socks, FOREIGN, seed=3, device=gpu, layout="offsets", align=1,
                                      payload_lens=(0, 1, 7, 8, 9, 55, 56, 57, 1464), ihl=tuple(range(5, 16)),
                                      vlan_frac=0.3, cksum=("ok", "bad", "zero"))
        out = classify(cl, fr)
        got, want = check(cl, fr, tbl, ent, out=out)
        assert want["stats"][2] > 20 and want["stats"][0] > 100
        # tagged frames leave the ptype node by another edge; selected by hand, their
        # l2_len of 18 moves every header by 4 more bytes
        rx = host(out["rxmeta"], np.uint32)
        sel = np.ones(fr.n, np.uint8)
        got, want = check(cl, fr, tbl, ent, out=out, sel=sel)
        tagged = (rx & 0x7F) == 18
        assert tagged.sum() > 50 and (want["l4edge"][tagged] == 0x11).any() and (want["l4edge"][tagged] == 0x10).any()
        # an empty worklist: no socket asks for a verify, every matched frame is received
        tbl2 = PcbTable(8)
        try:
            e2 = ent.copy()
            e2["flag"] = 0
            e2 = R.fill_table(tbl2, e2)
            got, want = check(cl, fr, tbl2, e2)
            assert want["stats"][2] == 0
        finally:
            tbl2.close()
    finally:
        tbl.close()


def test_golden_vectors_and_slab_end(cnet, gpu):
    """The reference's recorded verdicts (tests/golden/udp_cksum_ref.npz), each
    string behind an Ethernet header, laid end to end at odd addresses and
    selected by hand (their IPv4 headers carry no checksum of their own).  The
    last string's datagram claims 8 bytes past slab_len, which read as zero --
    and with them its sum is right; the one before it ends exactly at the next
    frame."""
    cl, local, other = cnet
    g = np.load(os.path.join(HERE, "golden", "udp_cksum_ref.npz"))
    off, verify, kinds = g["off"], g["verify"], [str(k) for k in g["kind"]]
    assert kinds[-1] == "claims+8/valid-over-zeros" and verify[-1] == 0
    nv = len(verify)
    eth = np.frombuffer(bytes.fromhex("020000000001020000000002") + b"\x08\x00", np.uint8)
    strings = [g["data"][off[i]:off[i + 1]] for i in range(nv)]
    offs = np.zeros(nv, np.int64)
    offs[1:] = np.cumsum([14 + len(s) for s in strings])[:-1]
    slab = np.concatenate([np.concatenate([eth, s]) for s in strings])
    assert offs[-1] + 14 + len(strings[-1]) == len(slab)      # the last datagram ends exactly at slab_len
    fr = pktgen.Frames(torch.from_numpy(slab).to(gpu), nv, offsets=torch.from_numpy(offs).to(gpu))
    tbl = PcbTable(512)
    try:
        ports = sorted({int(s[int(l3) + 2:int(l3) + 4].view("<u2")[0]) for s, l3 in zip(strings, g["l3_len"])
                        if len(s) >= int(l3) + 4})
        ent = np.zeros(len(ports), R.ENTRY_DT)
        ent["lport"], ent["flag"] = ports, R.CHK
        ent = R.fill_table(tbl, ent)
        out = classify(cl, fr)
        got, want = check(cl, fr, tbl, ent, out=out, sel=np.ones(nv, np.uint8))
        rx = host(out["rxmeta"], np.uint32)
        seen = 0
        for i in range(nv):
            s, l3 = strings[i], int(g["l3_len"][i])
            if (rx[i] & 0x7F) != 14 or ((rx[i] >> 7) & 0x1FF) != l3 or s[9] != 17 or not (s[l3 + 6] or s[l3 + 7]):
                continue
            seen += 1
            assert (got["l4edge"][i] == 0x11) == (verify[i] == 0), kinds[i]
        assert seen >= 200 and got["l4edge"][-1] == 0x11
    finally:
        tbl.close()


@pytest.mark.parametrize("punt", [True, False])
@pytest.mark.parametrize("tcp", [True, False])
def test_flags(cnet, gpu, punt, tcp):
    cl, local, other = cnet
    rng = np.random.default_rng(5)
    tbl, ent = make_table(rng, 64, local)
    try:
        tbl.set_flags(punt_enabled=punt, tcp_enabled=tcp)
        fr = pktgen.udp_socket_frames(257, sockets(local) + [(local[0], 4444)], FOREIGN, seed=9, device=gpu,
                                      proto=(17, 17, 6, 1, 255), cksum=("ok", "bad"), layout="packed", slot=128)
        check(cl, fr, tbl, ent, punt=punt, tcp=tcp)
        # ICMP and protocol 255 reach ip4_proto only when the ptype node's speculation
        # sends them to ip4_input: the caller's own selection stands for that here
        got, want = check(cl, fr, tbl, ent, punt=punt, tcp=tcp, sel=np.ones(257, np.uint8))
        e = want["l4edge"]
        assert (e == 0x02).any() == tcp and (e == 0x12).any() == punt and (e == 0x00).any()
        assert (e == 0x10).any() and (e == 0x11).any() and want["stats"][3] == (e == 0x00).sum()
    finally:
        tbl.close()


def test_selection(cnet, gpu):
    cl, local, other = cnet
    rng = np.random.default_rng(6)
    tbl, ent = make_table(rng, 64, local)
    try:
        fr = pktgen.udp_socket_frames(257, sockets(local, other), FOREIGN, seed=10, device=gpu, layout="umem")
        out = classify(cl, fr)
        got_d, _ = check(cl, fr, tbl, ent, out=out)                       # derived
        sel = (rng.random(257) < 0.5).astype(np.uint8)
        got_s, _ = check(cl, fr, tbl, ent, out=out, sel=sel)              # given
        assert ((got_s["l4edge"] != 0xFF) == (sel != 0)).all()
        assert (got_d["l4edge"] != 0xFF).any() and (got_d["l4edge"] == 0xFF).any()
        # no taken frame: every l4edge 0xFF, the counters as they were
        fr0 = pktgen.udp_socket_frames(65, [(a, 9) for a in other], FOREIGN, seed=12, device=gpu)
        from cndp_amd.l4 import alloc_l4_outputs
        l4 = alloc_l4_outputs(65, gpu)
        l4["stats"] += torch.tensor([5, 6, 7, 8], dtype=torch.int64, device=gpu)
        got, want = check(cl, fr0, tbl, ent, l4=l4, stats0=[5, 6, 7, 8])
        assert (got["l4edge"] == 0xFF).all() and got["stats"].tolist() == [5, 6, 7, 8]
        # and += on a batch that does count
        got, want = check(cl, fr, tbl, ent, out=out, l4=alloc_l4_outputs(257, gpu) | {"stats": l4["stats"]},
                          stats0=[5, 6, 7, 8])
        assert got["stats"].sum() > 26
    finally:
        tbl.close()


def test_classify_demux_partition(cnet, gpu):
    """cnet classify -> udp_input -> cndp_gpu_bin_partition on bin_of: every
    socket's receive list is its frames' indices in arrival order."""
    cl, local, other = cnet
    rng = np.random.default_rng(8)
    tbl, ent = make_table(rng, 512, local)
    try:
        n = 4099
        fr = pktgen.udp_socket_frames(n, sockets(local, other), FOREIGN, seed=13, device=gpu, proto=(17, 17, 17, 6),
                                      cksum=("ok", "bad", "zero"), layout="packed", slot=128)
        out = classify(cl, fr)
        l4 = cl.udp_input(fr, out, tbl)
        nb = l4["n_bins"]
        assert nb == 512
        start, order = cl.bin_partition(l4["bin_of"], nb)
        torch.cuda.synchronize()
        check(cl, fr, tbl, ent, out=out)
        bins, start, order = host(l4["bin_of"], np.uint16), host(start, np.uint32), host(order, np.uint32)
        assert start[0] == 0 and start[nb + 2] == n
        used = 0
        for b in range(nb + 2):
            want = np.nonzero(bins == b)[0]
            assert np.array_equal(order[start[b]:start[b + 1]], want), b
            used += b < nb and len(want) > 0
        assert used >= 8
    finally:
        tbl.close()


def test_table_changes_between_calls(cnet, gpu):
    """add, then delete, between calls on one stream: each call sees the table
    as it is when the call is made."""
    cl, local, other = cnet
    addrs, pp = pools(local)
    tbl = PcbTable(16)
    try:
        fr = pktgen.udp_socket_frames(129, [(local[0], 5000), (local[1], 5000)], FOREIGN, seed=14, device=gpu)
        out = classify(cl, fr)
        ent = np.zeros(0, R.ENTRY_DT)
        got, _ = check(cl, fr, tbl, ent, out=out)
        assert not (got["l4edge"] == 0x11).any()
        ent = R.fill_table(tbl, np.array([(addrs[0], 0, pp[2], 0, 0)], R.ENTRY_DT))
        got, _ = check(cl, fr, tbl, ent, out=out)
        n1 = (got["l4edge"] == 0x11).sum()
        assert n1 > 0
        more = np.array([(0, 0, pp[2], 0, R.CHK)], R.ENTRY_DT)
        R.fill_table(tbl, more)
        ent = np.concatenate([ent, more])
        got, _ = check(cl, fr, tbl, ent, out=out)
        assert (got["pcb"] == 1).any()
        assert tbl.delete(0) == 0
        ent[0] = 0
        got, _ = check(cl, fr, tbl, ent, out=out)
        assert not (got["pcb"] == 0).any() and (got["pcb"] == 1).any()
    finally:
        tbl.close()

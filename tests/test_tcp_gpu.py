"""TCP connection demux on the GPU (cndp_gpu_tcp_input, include/cndp_tcp.h):
every output array and the counters must equal the Python restatement
(tests/tcp_ref.py) applied to the same frames, to the cnet classify outputs and
to the l4edge array udp_input left.  Shapes are the smallest that can still go
wrong: one frame, a wave and its neighbours, more than one 1024-lane block;
packed slots, the UMEM stride, odd byte offsets; tables from empty to 4096
connections on one port."""
import os

import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd import pktgen
from cndp_amd.l4 import SEG_DT, PcbTable, addr_net, alloc_tcp_outputs, port_net

import l4_ref as R
import tcp_ref as T
from helpers import cnet_fibs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FOREIGN = [(0xC6120001, 40000), (0xC6120002, 40001), (0xC6120001, 40002), (0xC6120003, 50000)]
LPORTS = (80, 443, 8080)
NOBODY = 4444                      # no entry has this local port
ODT = {"l4edge": np.uint8, "pcb": np.uint32, "ports": np.uint32, "bin_of": np.uint16, "stats": np.uint64}
LAYOUTS = {"packed": dict(layout="packed", slot=128), "umem": dict(layout="umem"),
           "odd": dict(layout="offsets", align=1)}
# data offsets: sane, too small (rx_badoff), past a short segment's end, and a
# header claim that fits total_length but not total_length - l3_len (len wraps)
DOFFS = (5, 5, 5, 6, 8, 15, 2, 4, (15, 5), (12, 5))


@pytest.fixture(scope="module")
def cnet(gpu):
    from cndp_amd.classify import Classifier
    fib, fib6, routes, v6, v4vals, v6vals = cnet_fibs()
    cl = Classifier(0)
    cl.set_fib(fib, fib6)
    local = [ip for ip, d, _ in routes if d == 32]      # ip4_input's proto edge
    other = [routes[0][0] | 5, routes[1][0] | 9]        # forwarded, never taken
    assert len(local) >= 8
    udp = PcbTable(4)                                   # the UDP vector: empty, ip4_proto built with TCP
    udp.set_flags(punt_enabled=True, tcp_enabled=True)
    yield cl, local, other, udp
    udp.close()
    cl.close()


def pools(local):
    addrs = [addr_net(a) for a in local[:4]] + [addr_net(a) for a, _ in FOREIGN[:3]]
    return addrs, [port_net(p) for p in LPORTS + tuple(p for _, p in FOREIGN)]


def pairs(local, other=()):
    return ([((a, p), f) for a in list(local[:5]) + list(other) for p in LPORTS for f in FOREIGN]
            + [((local[0], NOBODY), FOREIGN[0])])


def make_table(rng, n, local, cap=None):
    """n entries from the collision-heavy pool, the first few fixed so that a
    connection, its listeners and a duplicate are there whatever the draw."""
    addrs, pp = pools(local)
    ent, dele = R.random_table(rng, n, addrs, pp, deleted_frac=0.05)
    if n >= 8:
        f = FOREIGN[0]
        ent[0] = (addrs[0], addr_net(f[0]), pp[0], port_net(f[1]), 0)
        ent[1] = ent[0]
        ent[2] = (addrs[0], 0, pp[0], 0, 0)
        ent[3] = (0, 0, pp[1], 0, 0)
        dele = dele[dele > 3]
    tbl = PcbTable(cap or max(n, 1))
    return tbl, R.fill_table(tbl, ent, dele)


def classify(cl, fr):
    cl.set_tuning(cnet_spec=256)     # a fresh ptype-node state, as in test_l4_gpu
    out = cl.alloc_outputs(fr.n, 64, device=fr.slab.device, meta=True)
    cl.classify(fr, N.CNDP_MODE_CNET, out=out)
    return out


def host(t, dt):
    return t.cpu().numpy().view(dt)


def check(cnet, fr, tbl, ent, out=None, l4=None, sel=None, punt=True, n_bins=None, tcp=None, stats0=None):
    """classify -> udp_input -> tcp_input against the restatement on the same
    arrays; returns (got, want, classify outputs)."""
    cl, _, _, udp = cnet
    out = classify(cl, fr) if out is None else out
    l4 = cl.udp_input(fr, out, udp) if l4 is None else l4
    torch.cuda.synchronize()
    edge0 = host(l4["l4edge"], np.uint8).copy()
    sel_t = torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).to(fr.slab.device) if sel is not None else None
    got_t = cl.tcp_input(fr, out, tbl, l4=l4, sel=sel_t, n_bins=n_bins, tcp=tcp)
    torch.cuda.synchronize()
    got = {k: host(got_t[k], dt) for k, dt in ODT.items()}
    got["seg"] = np.ascontiguousarray(got_t["seg"].cpu().numpy()).view(SEG_DT).reshape(-1)
    offs = fr.offsets.cpu().numpy() if fr.offsets is not None else None
    want = T.tcp_input_ref(fr.slab.cpu().numpy(), fr.n, host(out["rxmeta"], np.uint32), ent, l4edge=edge0, sel=sel,
                           stride=fr.stride, offsets=offs, data_off=fr.data_off, punt=punt,
                           n_bins=got_t["n_bins"], stats=stats0)
    for k in list(ODT) + ["seg"]:
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[0]}: got {got[k][bad[0]]} want {want[k][bad[0]]}"
    assert got["stats"][4] == (0 if stats0 is None else stats0[4])
    return got, want, out


def all_reached(want, punt=True):
    e = want["l4edge"]
    assert want["stats"][:4].all(), want["stats"]
    assert (e == T.E_SEG).any() and (e == T.E_DROP).any() and (e == 0xFF).any()
    assert (e == T.E_PUNT).any() == punt


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_sizes_and_layouts(cnet, gpu, n, layout):
    cl, local, other, _ = cnet
    rng = np.random.default_rng(n)
    tbl, ent = make_table(rng, 512, local)
    try:
        fr = pktgen.tcp_socket_frames(n, pairs(local, other), seed=n, device=gpu,
                                      payload_lens=(0, 1, 7, 8, 9, 55, 56, 57), ihl=(5, 5, 6, 15), vlan_frac=0.2,
                                      cksum=("ok", "ok", "bad", "zero"), data_off=DOFFS, **LAYOUTS[layout])
        got, want, _ = check(cnet, fr, tbl, ent)
        if n >= 257:   # the larger batches reach every counter and every edge value
            all_reached(want)
    finally:
        tbl.close()


def _one_port_table(local, k):
    """k - 1 connections on local[0]:80 and, in the middle of the vector, its listener."""
    addrs, pp = pools(local)
    ent = np.zeros(k, R.ENTRY_DT)
    fa = [0xC6130000 + (i % 251) for i in range(k)]
    fp = [1024 + i for i in range(k)]
    ent["laddr"], ent["lport"] = addrs[0], pp[0]
    ent["faddr"] = [addr_net(a) for a in fa]
    ent["fport"] = [port_net(p) for p in fp]
    ent[k // 2] = (addrs[0], 0, pp[0], 0, 0)
    step = max(1, k // 96)
    prs = [((local[0], 80), (fa[i], fp[i])) for i in range(0, k, step) if i != k // 2]
    prs += [((local[0], 80), FOREIGN[0]), ((local[1], 80), (fa[1], fp[1])), ((local[0], 443), (fa[2], fp[2]))]
    return ent, prs


@pytest.mark.parametrize("case", ["empty", "listener", "one_port4096", "mixed4096"])
def test_table_shapes(cnet, gpu, case):
    """No entry; one listener; 4095 connections on one port plus its listener
    (the exact hash at its fullest, one run of 4096); 4096 mixed entries."""
    cl, local, other, _ = cnet
    rng = np.random.default_rng(17)
    addrs, pp = pools(local)
    prs = pairs(local)
    if case == "empty":
        tbl, ent = make_table(rng, 0, local)
    elif case == "listener":
        tbl = PcbTable(1)
        ent = R.fill_table(tbl, np.array([(addrs[0], 0, pp[0], 0, 0)], R.ENTRY_DT))
    elif case == "mixed4096":
        tbl, ent = make_table(rng, 4096, local)
    else:
        ent, prs = _one_port_table(local, 4096)
        tbl = PcbTable(4096)
        ent = R.fill_table(tbl, ent)
    try:
        fr = pktgen.tcp_socket_frames(257, prs, seed=21, device=gpu, payload_lens=(0, 3, 18), cksum=("ok", "ok", "bad"),
                                      layout="packed", slot=128)
        got, want, _ = check(cnet, fr, tbl, ent)
        if case == "empty":
            assert want["stats"][T.S_NOMATCH] == (want["l4edge"] == T.E_PUNT).sum() > 0
        else:
            assert want["stats"][T.S_SEG] > 0 and want["stats"][T.S_CKSUM] > 0
        if case == "one_port4096":
            hit = got["pcb"][got["l4edge"] == T.E_SEG]
            assert len(np.unique(hit)) > 50 and (hit == 2048).any()       # connections and the listener
            assert want["stats"][T.S_NOMATCH] > 0
    finally:
        tbl.close()


def test_duplicates_and_deletes_between_calls(cnet, gpu):
    """Of two equal connections the lower index answers; once it is deleted the
    other does, then the listener, then nobody: punt, or drop with the punt flag
    off.  Each call sees the table as it is when the call is made."""
    cl, local, other, _ = cnet
    addrs, pp = pools(local)
    f = FOREIGN[1]
    conn = (addrs[0], addr_net(f[0]), pp[0], port_net(f[1]), 0)
    tbl = PcbTable(8)
    try:
        ent = R.fill_table(tbl, np.array([(0, 0, pp[1], 0, 0), (addrs[0], 0, pp[0], 0, 0), conn, conn], R.ENTRY_DT))
        fr = pktgen.tcp_socket_frames(129, [((local[0], 80), f)], seed=5, device=gpu, cksum=("ok",))
        out = classify(cl, fr)
        got, _, _ = check(cnet, fr, tbl, ent, out=out)
        taken = got["l4edge"] != 0xFF
        assert taken.sum() > 100 and (got["pcb"][taken] == 2).all() and (got["bin_of"][taken] == 2).all()
        for idx, then in ((2, 3), (3, 1)):
            assert tbl.delete(idx) == 0
            ent[idx] = 0
            got, _, _ = check(cnet, fr, tbl, ent, out=out)
            assert (got["pcb"][taken] == then).all()
        assert tbl.delete(1) == 0
        ent[1] = 0
        got, _, _ = check(cnet, fr, tbl, ent, out=out)
        assert (got["l4edge"][taken] == T.E_PUNT).all() and (got["bin_of"][taken] == 5).all()
        tbl.set_flags(punt_enabled=False)
        got, _, _ = check(cnet, fr, tbl, ent, out=out, punt=False)
        assert (got["l4edge"][taken] == T.E_DROP).all() and (got["bin_of"][taken] == 4).all()
        assert (got["pcb"] == N.CNDP_PCB_NONE).all() and not got["seg"].view(np.uint8).any()
    finally:
        tbl.close()


def test_golden_vectors_and_slab_end(cnet, gpu):
    """The reference's recorded verdicts (tests/golden/tcp_cksum_ref.npz) through
    the kernel: each string behind an Ethernet header, laid end to end at odd
    addresses and selected by hand.  The last string's segment claims 8 bytes past
    slab_len, which read as zero -- and with them its sum is right."""
    cl, local, other, _ = cnet
    g = np.load(os.path.join(HERE, "golden", "tcp_cksum_ref.npz"))
    off, verify, desc = g["off"], g["verify"], [str(k) for k in g["desc"]]
    assert desc[-1] == "claims+8/valid-over-zeros" and verify[-1] == 0
    nv = len(verify)
    eth = np.frombuffer(bytes.fromhex("020000000001020000000002") + b"\x08\x00", np.uint8)
    strings = [g["data"][off[i]:off[i + 1]] for i in range(nv)]
    offs = np.zeros(nv, np.int64)
    offs[1:] = np.cumsum([14 + len(s) for s in strings])[:-1]
    slab = np.concatenate([np.concatenate([eth, s]) for s in strings])
    assert offs[-1] + 14 + len(strings[-1]) == len(slab)      # the last segment is cut by slab_len
    fr = pktgen.Frames(torch.from_numpy(slab).to(gpu), nv, offsets=torch.from_numpy(offs).to(gpu))
    tbl = PcbTable(512)
    try:
        ports = sorted({int(s[int(l3) + 2:int(l3) + 4].view("<u2")[0]) for s, l3 in zip(strings, g["l3_len"])
                        if len(s) >= int(l3) + 4})
        ent = np.zeros(len(ports), R.ENTRY_DT)
        ent["lport"] = ports
        ent = R.fill_table(tbl, ent)
        got, want, out = check(cnet, fr, tbl, ent, sel=np.ones(nv, np.uint8))
        rx = host(out["rxmeta"], np.uint32)
        seen = 0
        for i in range(nv):
            s, l3 = strings[i], int(g["l3_len"][i])
            if (rx[i] & 0x7F) != 14 or ((rx[i] >> 7) & 0x1FF) != l3:
                continue
            seen += 1
            assert (got["l4edge"][i] == T.E_SEG) == (verify[i] == 0), desc[i]
        assert seen >= 200 and got["l4edge"][-1] == T.E_SEG
        zf = np.nonzero(g["kind"] == "zero_field_valid")[0]
        assert (got["l4edge"][zf] == T.E_SEG).sum() >= 100    # a zero checksum field is no exemption, and none is needed
    finally:
        tbl.close()


@pytest.mark.parametrize("punt", [True, False])
def test_punt_flag(cnet, gpu, punt):
    cl, local, other, _ = cnet
    rng = np.random.default_rng(5)
    tbl, ent = make_table(rng, 64, local)
    try:
        tbl.set_flags(punt_enabled=punt)
        fr = pktgen.tcp_socket_frames(257, pairs(local, other), seed=9, device=gpu, cksum=("ok", "bad"),
                                      data_off=DOFFS, ihl=(5, 15), layout="packed", slot=128)
        got, want, _ = check(cnet, fr, tbl, ent, punt=punt)
        all_reached(want, punt)
        miss = want["stats"][T.S_NOMATCH]
        assert miss == ((want["l4edge"] == T.E_PUNT).sum() if punt else (want["bin_of"] == 64).sum()
                        - want["stats"][T.S_CKSUM] - want["stats"][T.S_BADOFF])
    finally:
        tbl.close()


def _concat(a, b):
    """Two packed batches of one slot size as one."""
    assert a.stride == b.stride and a.offsets is None and b.offsets is None and a.data_off == b.data_off == 0
    return pktgen.Frames(torch.cat([a.slab, b.slab]), a.n + b.n, stride=a.stride,
                         lengths=torch.cat([a.lengths, b.lengths]))


def test_selection(cnet, gpu):
    """Both forms.  In place, a batch that also carries UDP datagrams for real
    UDP sockets: every entry tcp_input does not take keeps udp_input's value."""
    cl, local, other, _ = cnet
    rng = np.random.default_rng(6)
    tbl, ent = make_table(rng, 64, local)
    udp = PcbTable(4)
    try:
        udp.set_flags(tcp_enabled=True)
        assert udp.add(laddr=local[0], lport=5000) == 0
        fu = pktgen.udp_socket_frames(130, [(local[0], 5000), (local[1], 5000), (other[0], 5000)], seed=3, device=gpu)
        ft = pktgen.tcp_socket_frames(127, pairs(local, other), seed=10, device=gpu, cksum=("ok", "bad"), data_off=DOFFS)
        fr = _concat(fu, ft)
        out = classify(cl, fr)
        l4 = cl.udp_input(fr, out, udp)
        torch.cuda.synchronize()
        before = host(l4["l4edge"], np.uint8).copy()
        assert {0x11, 0x12, 0x02, 0xFF} <= set(before.tolist())
        got, want, _ = check(cnet, fr, tbl, ent, out=out, l4=l4)                  # derived, in place
        keep = before != T.TAKE
        assert keep.any() and (got["l4edge"][keep] == before[keep]).all()
        assert ((got["l4edge"] >> 4) == 2).sum() == (~keep).sum()
        assert (got["bin_of"][keep] == 65).all() and not got["seg"][keep].view(np.uint8).any()
        # given: sel alone decides, whatever l4edge holds; a fresh l4edge starts as "not taken"
        sel = (rng.random(fr.n) < 0.5).astype(np.uint8)
        sel[:130] = 0
        l4b = {"l4edge": alloc_tcp_outputs(fr.n, gpu)["l4edge"]}
        got_s, _, _ = check(cnet, fr, tbl, ent, out=out, l4=l4b, sel=sel)
        assert ((got_s["l4edge"] != 0xFF) == (sel != 0)).all()
        # no taken frame: the counters as they were; then += on a batch that counts
        tcp = alloc_tcp_outputs(fr.n, gpu, l4edge=l4b["l4edge"])
        tcp["stats"] += torch.tensor([5, 6, 7, 8, 0], dtype=torch.int64, device=gpu)
        got, _, _ = check(cnet, fr, tbl, ent, out=out, l4=l4b, sel=np.zeros(fr.n, np.uint8), tcp=tcp,
                          stats0=[5, 6, 7, 8, 0])
        assert got["stats"].tolist() == [5, 6, 7, 8, 0]
        got, _, _ = check(cnet, fr, tbl, ent, out=out, l4=l4b, sel=sel, tcp=tcp, stats0=[5, 6, 7, 8, 0])
        assert got["stats"].sum() > 26
    finally:
        udp.close()
        tbl.close()


def test_classify_udp_tcp_partition(cnet, gpu):
    """cnet classify -> udp_input -> tcp_input -> cndp_gpu_bin_partition on
    bin_of: every connection's list is its SEGMENT frames in arrival order."""
    cl, local, other, _ = cnet
    rng = np.random.default_rng(8)
    tbl, ent = make_table(rng, 512, local)
    try:
        n = 4099
        fr = pktgen.tcp_socket_frames(n, pairs(local, other), seed=13, device=gpu, cksum=("ok", "ok", "bad", "zero"),
                                      data_off=DOFFS, layout="packed", slot=128)
        got, want, out = check(cnet, fr, tbl, ent)
        nb = 512
        bins_t = torch.from_numpy(got["bin_of"].view(np.int16)).to(gpu)
        start, order = cl.bin_partition(bins_t, nb)
        torch.cuda.synchronize()
        start, order = host(start, np.uint32), host(order, np.uint32)
        assert start[0] == 0 and start[nb + 2] == n
        used = 0
        for b in range(nb + 2):
            idx = np.nonzero(got["bin_of"] == b)[0]
            assert np.array_equal(order[start[b]:start[b + 1]], idx), b
            if b < nb:
                assert np.array_equal(idx, np.nonzero((got["l4edge"] == T.E_SEG) & (got["pcb"] == b))[0])
                used += len(idx) > 0
        assert used >= 8
    finally:
        tbl.close()


def test_bad_offsets_and_len_wrap(cnet, gpu):
    """data_off < 5, an offset past total_length, and the reference's unchecked
    uint16_t subtraction: a header claim that fits total_length but not what is
    left after l3_len gives a len just under 65536."""
    cl, local, other, _ = cnet
    addrs, pp = pools(local)
    tbl = PcbTable(2)
    try:
        ent = R.fill_table(tbl, np.array([(0, 0, pp[0], 0, 0)], R.ENTRY_DT))
        fr = pktgen.tcp_socket_frames(257, [((local[0], 80), FOREIGN[0])], seed=31, device=gpu, ihl=(5, 15),
                                      payload_lens=(0, 3), cksum=("ok", "ok", "ok", "bad"),
                                      data_off=(0, 2, 4, 5, 15, (15, 5), (12, 5), (6, 5)), layout="offsets", align=1)
        got, want, _ = check(cnet, fr, tbl, ent)
        seg = got["seg"][got["l4edge"] == T.E_SEG]
        assert want["stats"][T.S_BADOFF] > 30 and want["stats"][T.S_CKSUM] > 10
        assert (seg["len"] > 65000).any() and (seg["len"] < 8).any() and (seg["offset"] == 60).any()
        bad = (got["l4edge"] == T.E_DROP) & (got["pcb"] == 0)          # rx_badoff: after m->userptr was set
        assert bad.sum() == want["stats"][T.S_BADOFF] and (got["bin_of"][bad] == 1).all()
        assert not got["seg"][bad].view(np.uint8).any()
    finally:
        tbl.close()


def test_errno_rules_and_empty_batch(cnet, gpu):
    """cndp_gpu_udp_input's rules: -EINVAL for an n_bins below the table's count
    or above 65533 and for what the call cannot run (here: a seg that is not
    16-byte aligned); an empty batch is accepted and writes nothing."""
    cl, local, other, _ = cnet
    rng = np.random.default_rng(4)
    tbl, ent = make_table(rng, 16, local)
    try:
        fr = pktgen.tcp_socket_frames(65, pairs(local), seed=2, device=gpu)
        out = classify(cl, fr)
        sel = torch.ones(65, dtype=torch.uint8, device=gpu)
        for nb in (15, 65534):
            with pytest.raises(OSError) as e:
                cl.tcp_input(fr, out, tbl, sel=sel, n_bins=nb)
            assert e.value.errno == 22
        tcp = alloc_tcp_outputs(65, gpu)
        tcp["seg"] = torch.empty(66 * 4 + 1, dtype=torch.int32, device=gpu)[1:]      # 4 bytes off
        with pytest.raises(OSError) as e:
            cl.tcp_input(fr, out, tbl, sel=sel, tcp=tcp)
        assert e.value.errno == 22
        torch.cuda.synchronize()
        fr0 = pktgen.Frames(fr.slab, 0, stride=fr.stride, lengths=fr.lengths[:0])
        tcp = alloc_tcp_outputs(0, gpu)
        got = cl.tcp_input(fr0, {"rxmeta": out["rxmeta"][:0]}, tbl, sel=sel[:0], tcp=tcp)
        torch.cuda.synchronize()
        assert got["stats"].tolist() == [0, 0, 0, 0, 0]
    finally:
        tbl.close()

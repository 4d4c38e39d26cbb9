"""udp_output + ip4_output on the GPU (cndp_gpu_ip4_output, include/cndp_tx.h):
tx_edge, bin_of, the counters, the netifs' identification counters read back and
the WHOLE slab, byte for byte and with the 0xA5 guard bytes after it, must equal
the Python restatement (tests/tx_ref.py) applied to the same buffers, inputs and
tables.  The buffers start out as random bytes, so a frame not taken, d_addr on
an ARP miss or packet_id without a route show if they are touched.  Shapes are
the smallest that can still go wrong: one frame, a wave and its neighbours, more
than one block, one batch just above blocks launched x frames per block so every
block takes a second pass; headers at odd and even addresses; frames of several
netifs interleaved, so the identification sum crosses lanes, waves, passes and
blocks for each netif."""
import os

import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd import pktgen
from cndp_amd import tx as T
from cndp_amd.l4 import PcbTable
from cndp_amd.tx import alloc_tx_outputs

import fwd_ref as F
import tx_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
UDT = {"tx_edge": np.uint16, "bin_of": np.uint16, "stats": np.uint64}
SIZES = [1, 3, 4, 5, 63, 64, 65, 257, 1027]
SELS = ["all", "none", "third", "eighth"]
# (layout, data offsets): headers land at even (42, 64, 256) and odd (43) addresses
LAYOUTS = {"packed": (42, 43, 64), "umem": (256,), "imix": (42, 43, 64)}


def make_sel(kind: str, n: int):
    if kind == "all":
        return None
    s = np.zeros(n, np.uint8)
    if kind == "third":
        s[::3] = 1
    elif kind == "eighth":
        s[:] = np.random.default_rng(1000 + n).random(n) < 0.125
    return s


def host(t, dt):
    return t.cpu().numpy().view(dt)


def dev32(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(gpu)


def idents(tw):
    return [tw.ident.get(k, 0) for k in range(256)]


def run(cl, tabs, tw, lay, inp, gpu, mode=R.TX_UDP, sel=None, n_bins=8, stats0=None, tx=None, stream=None,
        slab_t=None, want_slab=None, ref=True):
    """One call of the stage against the restatement; returns (got, want, slab tensor, expected slab)."""
    _, _, fwd, pt = tabs
    buf, slab_len, stride, offs, data_off, _ = lay
    pcb, faddr, laddr, ports, length = inp
    n = len(pcb)
    if slab_t is None:
        slab_t = torch.from_numpy(buf.copy()).to(gpu)
        want_slab = buf.copy()
    offs_t = torch.from_numpy(offs).to(gpu) if offs is not None else None
    fr = pktgen.Frames(slab_t[:slab_len], n, stride=stride, offsets=offs_t, data_off=data_off)
    sel_t = torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).to(gpu) if sel is not None else None
    args = [dev32(pcb, gpu), dev32(faddr, gpu), dev32(laddr, gpu), dev32(ports, gpu) if mode == R.TX_UDP else None,
            torch.from_numpy(np.ascontiguousarray(length, np.uint16).view(np.int16)).to(gpu)]
    if stream is not None:
        torch.cuda.synchronize()        # the inputs above were made on the current stream
    got_t = cl.ip4_output(fr, fwd, pt, *args, mode=mode, sel=sel_t, n_bins=n_bins, tx=tx, stream=stream)
    torch.cuda.synchronize()
    got = {k: host(got_t[k], dt) for k, dt in UDT.items()}
    got["tx"] = got_t
    if not ref:
        return got, None, slab_t, want_slab
    want = R.ip4_output_ref(want_slab, n, tw, pcb, faddr, laddr, ports, length, mode=mode, stride=stride, offsets=offs,
                            data_off=data_off, sel=sel, n_bins=n_bins, stats=stats0, slab_len=slab_len)
    what = f"mode {mode} data_off {data_off}"
    for k in UDT:
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, (f"{what}: {k}: {len(bad)} differ, first at {bad[0]}: got {got[k][bad[0]]:#x} "
                               f"want {want[k][bad[0]]:#x}")
    got_slab = slab_t.cpu().numpy()
    bad = np.nonzero(got_slab != want_slab)[0]
    assert len(bad) == 0, (f"{what}: slab: {len(bad)} bytes differ, first at {bad[0]} (slab_len {slab_len}): "
                           f"got {got_slab[bad[0]]:#x} want {want_slab[bad[0]]:#x}")
    have = [T.ident_get(fwd, k) for k in range(256)]
    assert have == idents(tw), f"{what}: identification counters: {have[:6]} want {idents(tw)[:6]}"
    return got, want, slab_t, want_slab


def inputs(n, tw, seed, mode=R.TX_UDP, **kw):
    pcb, faddr, laddr, ports, length = R.make_inputs(n, tw, seed, **kw)
    if mode == R.TX_IP4:
        length = (length + 20).astype(np.uint16)    # the L4 header is counted
    return pcb, faddr, laddr, ports, length


def laid(kind, inp, data_off, seed=0, guard=64, cut=None):
    """The buffers for `inp`; lengths come back cut to what a slot holds."""
    lay = R.layout(kind, inp[4], data_off, seed=seed, guard=guard, cut=cut)
    return lay, inp[:4] + (lay[5],)


def set_idents(tabs, tw, ident0=0xFFF0):
    for nif in range(6):
        tw.ident[nif] = (ident0 + nif) & 0xFFFF
        assert T.ident_set(tabs[2], nif, tw.ident[nif]) == 0


@pytest.fixture(scope="module")
def cl(gpu):
    from cndp_amd.classify import Classifier
    c = Classifier(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worlds(gpu):
    """The standard world folded onto 1, 2 and 5 netifs, in the product's tables."""
    made = {}
    for k in (1, 2, 5):
        tw = R.standard_world(k)
        made[k] = (tw, R.make_tables(tw))
    yield made
    for tw, tabs in made.values():
        R.close_tables(*tabs)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(LAYOUTS))
@pytest.mark.parametrize("n", SIZES)
def test_sizes_layouts_selections(cl, worlds, gpu, n, kind):
    tw, tabs = worlds[5]
    set_idents(tabs, tw)        # 0xFFF0...: the counters wrap within a batch
    seen = np.zeros(6, np.uint64)
    for data_off in LAYOUTS[kind]:
        for sk in SELS:
            for mode in (R.TX_UDP, R.TX_IP4) if sk in ("all", "third") else (R.TX_UDP,):
                lay, inp = laid(kind, inputs(n, tw, n + data_off, mode), data_off, seed=n)
                sel = make_sel(sk, n)
                got, want, _, _ = run(cl, tabs, tw, lay, inp, gpu, mode=mode, sel=sel)
                if sel is not None:
                    assert (got["tx_edge"][sel == 0] == 0xFFFF).all()
                seen += want["stats"]
    if n >= 257:    # sent, arp_request, no route, protocol, checksummed all occur; never the headroom
        assert seen[[R.SENT, R.ARP_REQ, R.DROP_NOROUTE, R.DROP_PROTO, R.CKSUM]].all() and seen[R.DROP_HEADROOM] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("netifs", [1, 2])
def test_one_and_two_netifs(cl, worlds, gpu, netifs):
    """Every frame of the batch on one netif, and two netifs interleaved."""
    tw, tabs = worlds[netifs]
    set_idents(tabs, tw)
    for n in (65, 257, 1027):
        lay, inp = laid("imix", inputs(n, tw, 7 * n), 43, seed=n)
        got, want, _, _ = run(cl, tabs, tw, lay, inp, gpu)
        used = set(want["bin_of"][want["bin_of"] < 8].tolist())
        assert len(used) == netifs


@pytest.mark.gpu
def test_second_pass_of_every_block(cl, worlds, gpu):
    """One frame more than blocks launched x frames per block: the blocks'
    chunks double, so each block's running counters carry into a second pass and
    from block to block, for five interleaved netifs."""
    tw, tabs = worlds[5]
    set_idents(tabs, tw)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = cus * T.TX_BLOCKS_PER_CU * T.TX_BLOCK + 1
    assert n <= 1 << 18
    lay, inp = laid("slot64", inputs(n, tw, 99, lens=(0, 1, 2, 3, 17, 18, 22), odd_pcbs=False), 42, seed=5)
    sel = make_sel("eighth", n)
    sel[-1] = sel[T.TX_BLOCK] = sel[2 * T.TX_BLOCK - 1] = 1     # the last frame; a second pass's first and last lane
    got, want, _, _ = run(cl, tabs, tw, lay, inp, gpu, sel=sel)
    assert want["stats"][R.SENT] > n // 64


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [R.TX_UDP, R.TX_IP4])
def test_insufficient_headroom(cl, worlds, gpu, mode):
    tw, tabs = worlds[5]
    set_idents(tabs, tw)
    n = 67
    for headroom in (7, 8, 27, 28, 41, 42, 43, 256):
        kind = "umem" if headroom == 256 else ("packed", "imix")[headroom & 1]
        lay, inp = laid(kind, inputs(n, tw, headroom, mode), headroom, seed=headroom)
        before = idents(tw)
        got, want, _, _ = run(cl, tabs, tw, lay, inp, gpu, mode=mode)
        if headroom < (42 if mode == R.TX_UDP else 34):
            assert want["stats"][R.SENT] == 0 and want["stats"][R.DROP_HEADROOM] > 0 and idents(tw) == before
        else:
            assert want["stats"][R.SENT] > 0 and want["stats"][R.DROP_HEADROOM] == 0


@pytest.mark.gpu
def test_two_calls_and_ident_set(cl, worlds, gpu):
    """A second call continues from the first's counters (the device copy); an
    ident_set between two calls reaches the device and leaves the others alone;
    the counters accumulate in `stats`."""
    tw, tabs = worlds[5]
    set_idents(tabs, tw)
    n = 257
    lay, inp = laid("packed", inputs(n, tw, 3), 64, seed=3)
    got, want, slab_t, want_slab = run(cl, tabs, tw, lay, inp, gpu)
    assert idents(tw)[:6] != [0xFFF0 + k for k in range(6)]
    got, want, slab_t, want_slab = run(cl, tabs, tw, lay, inp, gpu, slab_t=slab_t, want_slab=want_slab, tx=got["tx"],
                                       stats0=want["stats"])
    keep = idents(tw)
    tw.ident[2] = 0x1234
    assert T.ident_set(tabs[2], 2, 0x1234) == 0
    assert [T.ident_get(tabs[2], k) for k in range(6)] == keep[:2] + [0x1234] + keep[3:6]
    got, want, _, _ = run(cl, tabs, tw, lay, inp, gpu, slab_t=slab_t, want_slab=want_slab, tx=got["tx"],
                          stats0=want["stats"])
    assert want["stats"][R.SENT] % 3 == 0 and want["stats"][R.SENT] > 0


@pytest.mark.gpu
def test_same_input_twice_is_identical(cl, worlds, gpu):
    tw, tabs = worlds[5]
    n = 1027
    lay, inp = laid("imix", inputs(n, tw, 41), 43, seed=41)
    slabs = []
    for _ in range(2):
        set_idents(tabs, tw, 0x8001)
        _, _, slab_t, _ = run(cl, tabs, tw, lay, inp, gpu, ref=False)
        slabs.append(slab_t.cpu().numpy())
    assert np.array_equal(slabs[0], slabs[1])


@pytest.mark.gpu
def test_slab_end(cl, worlds, gpu):
    """The last frame cut by slab_len inside its payload, its headers and before
    them: bytes past the end read as zero, nothing at or past it is written."""
    tw, tabs = worlds[5]
    set_idents(tabs, tw)
    n = 5
    for kind, data_off in (("packed", 64), ("imix", 43)):
        for cut in (-43, -42, -41, -36, -29, -28, -22, -9, -8, -7, -2, -1, 0, 1, 2, 5, 16, 17, 40):
            base = inputs(n, tw, 11, lens=(40,), pcb_pool=[1, 3, 8, 32], odd_pcbs=False)
            lay, inp = laid(kind, base, data_off, seed=cut + 50, guard=96, cut=cut)
            for mode in (R.TX_UDP, R.TX_IP4):
                got, want, slab_t, _ = run(cl, tabs, tw, lay, inp, gpu, mode=mode)
                assert (slab_t.cpu().numpy()[lay[1]:] == 0xA5).all()
                assert want["tx_edge"][n - 1] != 0xFFFF


@pytest.mark.gpu
def test_streams(cl, worlds, gpu):
    """Calls on non-default streams, alternating without a host wait: each starts
    from the counters and the slab the one before left."""
    tw, tabs = worlds[5]
    set_idents(tabs, tw)
    n = 1027
    lay, inp = laid("packed", inputs(n, tw, 23), 64, seed=23)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    _, _, slab_t, want_slab = run(cl, tabs, tw, lay, inp, gpu, stream=s1.cuda_stream)
    run(cl, tabs, tw, lay, inp, gpu, stream=s2.cuda_stream, slab_t=slab_t, want_slab=want_slab)
    buf, slab_len, stride, offs, data_off, _ = lay
    slab_t = torch.from_numpy(buf.copy()).to(gpu)
    fr = pktgen.Frames(slab_t[:slab_len], n, stride=stride, data_off=data_off)
    args = [dev32(a, gpu) for a in inp[:4]] + [torch.from_numpy(inp[4].view(np.int16)).to(gpu)]
    tx = alloc_tx_outputs(n, gpu)
    torch.cuda.synchronize()
    for s in (s1, s2, s1, s2):
        cl.ip4_output(fr, tabs[2], tabs[3], *args, n_bins=8, tx=tx, stream=s.cuda_stream)
    torch.cuda.synchronize()
    ref = buf.copy()
    for _ in range(4):
        want = R.ip4_output_ref(ref, n, tw, *inp, stride=stride, data_off=data_off, slab_len=slab_len)
    assert np.array_equal(slab_t.cpu().numpy(), ref)
    assert [T.ident_get(tabs[2], k) for k in range(256)] == idents(tw)
    assert np.array_equal(host(tx["stats"], np.uint64), want["stats"] * 4)


@pytest.mark.gpu
def test_zero_sum_goes_out_as_ffff(cl, worlds, gpu):
    """The reference's recorded zero-sum datagrams, sent: the addresses, ports
    and payloads of tests/golden/ip4_output_cksum_ref.npz through the stage give
    the recorded checksums, 0xFFFF where the complemented sum is 0."""
    tw, tabs = worlds[5]
    g = np.load(os.path.join(HERE, "golden", "ip4_output_cksum_ref.npz"))
    kinds = g["kind"].tolist()
    pick = [i for i in range(len(kinds)) if g["proto"][i] == 17 and g["off"][i + 1] - g["off"][i] - 28 <= 1472][:96]
    zs = [k for k, i in enumerate(pick) if kinds[i].startswith("zero-sum")]
    pick = pick + [i for i in range(len(kinds)) if kinds[i].startswith("zero-sum") and g["proto"][i] == 17]
    strs = [g["data"][g["off"][i]:g["off"][i + 1]] for i in pick]
    n = len(strs)
    laddr = np.array([int.from_bytes(bytes(s[12:16]), "little") for s in strs], np.uint32)
    faddr = np.array([int.from_bytes(bytes(s[16:20]), "little") for s in strs], np.uint32)
    ports = np.array([int.from_bytes(bytes(s[22:24]), "little") | int.from_bytes(bytes(s[20:22]), "little") << 16
                      for s in strs], np.uint32)
    length = np.array([len(s) - 28 for s in strs], np.uint16)
    # a world of its own: every source address routed, one PCB with the checksum flag
    w = F.World(4, 4)
    w.rt[1] = (0, 1)
    w.rt_fib.add(0, 1, 1)
    w.rt_fib.add(0x80000000, 1, 1)
    tw1 = R.TxWorld(w, [R.Pcb(cksum=True)])
    tabs1 = R.make_tables(tw1)
    try:
        lay = R.layout("umem", length, 256, seed=1, guard=64)
        for k, s in enumerate(strs):
            lay[0][k * 2048 + 256:k * 2048 + 256 + len(s) - 28] = s[28:]
        inp = (np.zeros(n, np.uint32), faddr, laddr, ports, lay[5])
        got, want, slab_t, _ = run(cl, tabs1, tw1, lay, inp, gpu, n_bins=2)
        rows = slab_t.cpu().numpy()[:n * 2048].reshape(n, 2048)
        sent = rows[:, 256 - 2].astype(np.uint16) | rows[:, 256 - 1].astype(np.uint16) << 8
        assert np.array_equal(sent, g["l4_cksum"][pick])
        assert len(pick) - 96 >= 8 and (sent[96:] == 0xFFFF).all() and (sent[zs] == 0xFFFF).all()
        assert want["stats"][R.CKSUM] == n
    finally:
        R.close_tables(*tabs1)


@pytest.mark.gpu
def test_arguments(cl, worlds, gpu):
    tw, tabs = worlds[5]
    _, _, fwd, pt = tabs
    n = 5
    lay, inp = laid("packed", inputs(n, tw, 1), 64)
    slab_t = torch.from_numpy(lay[0].copy()).to(gpu)
    fr = pktgen.Frames(slab_t[:lay[1]], n, stride=128, data_off=64)
    full = [dev32(a, gpu) for a in inp[:4]] + [torch.from_numpy(inp[4].view(np.int16)).to(gpu)]

    def refused(args=full, mode=R.TX_UDP, n_bins=8, tx=None):
        with pytest.raises(OSError) as e:
            cl.ip4_output(fr, fwd, pt, *args, mode=mode, n_bins=n_bins, tx=tx)
        return e.value.errno == 22

    for k in range(5):
        assert refused(args=full[:k] + [None] + full[k + 1:])
    assert refused(mode=2) and refused(n_bins=7) and refused(n_bins=65534)
    assert refused(tx=alloc_tx_outputs(n, gpu) | {"tx_edge": None})
    torch.cuda.synchronize()
    assert np.array_equal(slab_t.cpu().numpy(), lay[0])     # a refused call touches nothing
    cl.ip4_output(fr, fwd, pt, *(full[:3] + [None] + full[4:]), mode=R.TX_IP4, n_bins=8)    # no ports in IP4 mode
    cl.ip4_output(pktgen.Frames(slab_t, 0, stride=128, data_off=64), fwd, pt, *full, n_bins=8)  # an empty batch
    torch.cuda.synchronize()
    T.ident_get(fwd, 0)


@pytest.mark.gpu
def test_echo_end_to_end(gpu):
    """classify -> udp_input -> swap addresses and ports -> ip4_output ->
    classify the produced frames as the peer would -> udp_input with checksum
    verify on the mirrored PCB table: every datagram is received, so the
    generated checksums verify under the project's own kernel."""
    from cndp_amd.classify import Classifier
    from cndp_amd.fib import Fib, node_ip4_add_input
    from helpers import CNET_DEF, cnet_fibs
    fib, fib6, routes, _, _, _ = cnet_fibs()
    local = [ip for ip, d, _ in routes if d == 32][:4]
    foreign = [(0xC6120001, 9), (0xC6120002, 53), (0xC6120003, 5000)]
    ports_h = (7, 5000)
    peer = Fib("peer-fib", N.CNE_FIB_DIR24_8, default_nh=CNET_DEF, max_routes=64, nh_sz=N.CNE_FIB_DIR24_8_4B,
               num_tbl8=16)
    ours, theirs = PcbTable(16), PcbTable(16)
    w = F.World(8, 8)
    tabs = None
    cl = Classifier(0)
    try:
        for k, (a, _) in enumerate(foreign):
            assert node_ip4_add_input(peer, a, 32, k) == 0
            w.arp[k + 1] = (0, bytes([2, 0xAA, 0, 0, 0, k + 1]))
            w.arp_fib.add(a, 32, k + 1)
        for k, a in enumerate(local):
            w.rt[k + 1] = (0, k % 2)
            w.rt_fib.add(a, 32, k + 1)
            for p in ports_h:
                ours.add(laddr=a, lport=p, cksum=True)
        for a, p in foreign:
            theirs.add(laddr=a, lport=p, cksum=True)
        w.netif = {0: bytes([2, 0x11, 0, 0, 0, 0]), 1: bytes([2, 0x11, 0, 0, 0, 1])}
        arp, rt4, fwd = F.make_tables(w)
        tabs = (arp, rt4, fwd)

        n = 200
        rx = pktgen.udp_socket_frames(n, [(a, p) for a in local for p in ports_h], foreign, seed=5, device=gpu,
                                      payload_lens=(0, 1, 2, 3, 17, 18, 64), cksum=("ok",), layout="packed", slot=128)
        cl.set_fib(fib, fib6)
        cl.set_tuning(cnet_spec=256)
        out = cl.classify(rx, N.CNDP_MODE_CNET, out=cl.alloc_outputs(n, 64, device=gpu, meta=True))
        l4 = cl.udp_input(rx, out, ours)
        torch.cuda.synchronize()
        recv = N.CNDP_L4_EDGE(N.CNDP_L4_NODE_UDP_INPUT, N.CNDP_UDP_INPUT_CHNL_RECV)
        assert (l4["l4edge"] == recv).all()
        # the application: the payload into a transmit buffer, the addresses swapped
        rows = rx.slab.view(n, 128)
        plen = (rows[:, 38].to(torch.int32) << 8 | rows[:, 39].to(torch.int32)) - 8
        txs = torch.zeros(n, 256, dtype=torch.uint8, device=gpu)
        txs[:, 64:64 + 64] = rows[:, 42:42 + 64]
        src = rows[:, 26:30].contiguous().view(torch.int32).reshape(n)      # the frame's source: our foreign address
        dst = rows[:, 30:34].contiguous().view(torch.int32).reshape(n)
        fr = pktgen.Frames(txs.view(-1), n, stride=256, data_off=64)
        tx = cl.ip4_output(fr, fwd, ours, l4["pcb"], src, dst, l4["ports"], plen.to(torch.int16))
        torch.cuda.synchronize()
        assert (host(tx["tx_edge"], np.uint16) >= 2).all() and host(tx["stats"], np.uint64)[R.CKSUM] == n
        # the peer: the produced frames start 42 bytes before the payload
        back = pktgen.Frames(txs.view(-1), n, stride=256, data_off=22)
        cl.set_fib(peer, fib6)
        cl.set_tuning(cnet_spec=256)
        out2 = cl.classify(back, N.CNDP_MODE_CNET, out=cl.alloc_outputs(n, 64, device=gpu, meta=True))
        l4b = cl.udp_input(back, out2, theirs)
        torch.cuda.synchronize()
        st = host(l4b["stats"], np.uint64)
        assert (l4b["l4edge"] == recv).all() and st[N.CNDP_L4_STAT_RECV] == n and st[N.CNDP_L4_STAT_CKSUM] == 0
        # what came back is what went out: the ports swapped, the payload offset the same
        assert np.array_equal(host(l4b["ports"], np.uint32), np.bitwise_or(host(l4["ports"], np.uint32) >> 16,
                                                                            host(l4["ports"], np.uint32) << 16))
        assert (host(l4b["payload_off"], np.uint16) == 42).all()
    finally:
        cl.close()
        if tabs:
            F.close_tables(*tabs)
        ours.close()
        theirs.close()
        peer.close()
        fib.close()
        fib6.close()

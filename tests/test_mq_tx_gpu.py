"""cnet's udp_output + ip4_output nodes as a mode of the asynchronous mbuf queue
(cndp_gpu_mq_create_ip4_output, include/cndp_mqtx.h), zero-copy and staged, both
tx_modes, over pools of at most 1024 mbufs laid out like CNDP's.

Every expected value comes twice: from the Python restatement of the nodes over
mbufs (tests/mq_tx_ref.py, independent of the library) and from the host twin
(cndp_ip4_output_node_host) run burst by burst over a copy of the pool.  The
edges, the seven counters, the order of return, every netif's counter afterwards
and the WHOLE pool memory -- mbuf headers, metadata, headroom and frames -- are
compared exactly.  Every test asserts that the outcomes it is about occur in its
input."""
import ctypes

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd import tx as X
from cndp_amd.mbuf import FRAME, HDR, MbufQueue

import mq_tx_ref as M
import tx_ref as T

pytestmark = pytest.mark.gpu

KEYS = tuple(range(N.CNDP_MQ_STAT_TX_SENT, N.CNDP_MQ_STAT_TX_CKSUM + 1))
OTHER_KEYS = (N.CNDP_MQ_STAT_FORWARD, N.CNDP_MQ_STAT_ECHO, N.CNDP_MQ_STAT_ACL_PREFILTER, N.CNDP_MQ_STAT_ACL_DENY,
              N.CNDP_MQ_STAT_ACL_PERMIT, N.CNDP_MQ_STAT_FWD_DIRECT, N.CNDP_MQ_STAT_FWD_GATEWAY,
              N.CNDP_MQ_STAT_FWD_ARP_REQUEST)
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "staged"])
MODES = pytest.mark.parametrize("mode", [M.TX_UDP, M.TX_IP4], ids=["udp", "ip4"])
MIX_BURSTS = [256, 253, 3, 256, 232]


@pytest.fixture(scope="module")
def cl(gpu):
    from cndp_amd.classify import Classifier
    c = Classifier(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def std(gpu):
    w = M.standard_world()
    yield w
    w.close()


def own(e):
    return e & N.CNDP_MQ_EDGE_TX_MASK


class Queue:
    """An ip4_output queue over `pool`, registered first when zero-copy."""

    def __init__(self, cl, pool, world, mode, zero_copy, batch=256, depth=2, md_delta=None, md_null=None,
                 register=True, **kw):
        self.cl, self.pool, self.world = cl, pool, world
        self.reg = zero_copy and register
        self.seen = [0] * M.NSTAT
        hook = M._hook(pool.base, md_delta, md_null)
        if self.reg:
            cl.host_register(pool.mem)
        try:
            # a long max_delay_us: a batch goes out when no further full burst fits, half full with
            # the GPU idle, or flushed
            self.q = MbufQueue(cl, N.CNDP_MQ_IP4_OUTPUT, batch=batch, depth=depth,
                               umem=pool.base if zero_copy else None, fwd_tbl=world.fwd, pcb_tbl=world.pt,
                               tx_mode=mode, max_delay_us=1000000, metadata=hook, **kw)
        except Exception:
            if self.reg:
                cl.host_unregister(pool.mem)
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.q.close()
        if self.reg:
            self.cl.host_unregister(self.pool.mem)

    def drive(self, bursts, outside=None, flush_each=False):
        """Submit bursts of mbuf indices (None: the mbuf at address `outside`) as
        cnet-graph's node would, polling between them, until all are back:
        (addresses, edges) in completion order."""
        q = self.q
        got_a, got_e = [], []

        def take():
            a, e = q.poll()
            got_a.append(a)
            got_e.append(e)
            return a
        for b in bursts:
            ptrs = (ctypes.c_void_p * len(b))(*[outside if i is None else self.pool.addr(int(i)) for i in b])
            done = 0
            while done < len(b):
                k = q.submit(ctypes.addressof(ptrs) + done * ctypes.sizeof(ctypes.c_void_p), len(b) - done)
                done += k
                if flush_each:
                    q.flush()
                a = take()
                if k == 0 and a.size == 0:
                    q.wait()
        for _ in range(64):
            if not q.pending:
                break
            q.flush()
            q.wait()
            take()
        assert q.pending == 0
        return np.concatenate(got_a), np.concatenate(got_e)

    def check(self, bursts, want, outside=None, flush_each=False):
        """One pass of `bursts` through the queue against `want` (M.expect)."""
        addrs, edges = self.drive(bursts, outside, flush_each)
        sent = [outside if i is None else self.pool.addr(int(i)) for b in bursts for i in b]
        assert addrs.tolist() == sent, "mbufs came back out of submission order"
        bad = np.nonzero(edges != want["edges"])[0]
        assert len(bad) == 0, (f"edges: {len(bad)} differ, first at {bad[0]}: got {edges[bad[0]]:#x} "
                               f"want {want['edges'][bad[0]]:#x}")
        bad = np.nonzero(self.pool.mem != want["mem"])[0]
        assert len(bad) == 0, (f"pool memory: {len(bad)} bytes differ, first at mbuf {bad[0] // FRAME} + {bad[0] % FRAME}: "
                               f"got {self.pool.mem[bad[0]]:#x} want {want['mem'][bad[0]]:#x}")
        assert self.world.get_ident(want["ident1"]) == want["ident1"], "netif counters"
        self.seen = [a + b for a, b in zip(self.seen, want["stats"])]
        assert [self.q.stat(k) for k in KEYS] == self.seen
        assert all(self.q.stat(k) == 0 for k in OTHER_KEYS)         # other modes' families
        return edges


def occurs(want, *keys):
    assert all(want["stats"][k] > 0 for k in keys), want["stats"]


@MODES
@FORMS
def test_standard_mix(cl, std, mode, zero_copy):
    """1000 mbufs in bursts with tails over five netifs: every netif's counter
    crosses several batches and wraps."""
    pool = M.make_pool(1000)
    M.fill_mix(pool, std, mode)
    bursts = M.split(list(range(1000)), MIX_BURSTS)
    want = M.expect(pool, std, bursts, mode, zero_copy)
    occurs(want, M.SENT, M.ARP, M.HEADROOM, M.NOROUTE, M.PROTO, M.CKSUM)
    none = int((want["edges"] == M.EDGE_NONE).sum())
    assert none > 0 and sum(want["stats"][:6]) + none == 1000
    for lo in (0, 256, 512, 768):                              # every netif in every batch
        part = want["edges"][lo:lo + 232]
        assert {int(own(e)) - 2 for e in part if e != M.EDGE_NONE and own(e) >= 2} == {0, 1, 2, 3, 4}
    assert any(want["ident1"][k] < want["ident0"][k] for k in range(5))
    with Queue(cl, pool, std, mode, zero_copy) as q:
        q.check(bursts, want)
        assert q.q.stat(N.CNDP_MQ_STAT_MBUFS) == 1000 and q.q.stat(N.CNDP_MQ_STAT_BATCHES) >= 4


@FORMS
def test_one_burst_per_batch(cl, std, zero_copy):
    pool = M.make_pool(300)
    M.fill_mix(pool, std, M.TX_UDP, seed=9)
    bursts = M.split(list(range(300)), [1, 63, 64, 65, 107])
    want = M.expect(pool, std, bursts, M.TX_UDP, zero_copy)
    occurs(want, M.SENT, M.ARP, M.CKSUM)
    with Queue(cl, pool, std, M.TX_UDP, zero_copy, batch=512, depth=4) as q:
        q.check(bursts, want, flush_each=True)
        assert q.q.stat(N.CNDP_MQ_STAT_BATCHES) == 5


@FORMS
def test_uniform_batches(cl, std, zero_copy):
    """All drops, all not taken, all on one netif."""
    n = 300
    for kind in ("drops", "none", "one_netif"):
        pool = M.make_pool(n)
        for i in range(n):
            if kind == "drops":
                M.put(pool, std, i, (5, M.PCB_PROTO1, 1)[i % 3], length=i, data_off=(192, 192, 30)[i % 3])
            elif kind == "none":
                M.put(pool, std, i, 1, userptr=(M.PCB_DEAD, 1 << 40, 4000)[i % 3])
            else:
                M.put(pool, std, i, 1, faddr=T.ip_n("10.1.0.2"), length=i, data_off=192 + i % 16)
        bursts = M.split(list(range(n)), [256, 44])
        want = M.expect(pool, std, bursts, M.TX_UDP, zero_copy)
        if kind == "drops":
            occurs(want, M.NOROUTE, M.PROTO, M.HEADROOM)
            assert want["stats"][M.SENT] == want["stats"][M.ARP] == 0
        elif kind == "none":
            assert (want["edges"] == M.EDGE_NONE).all() and np.array_equal(want["mem"], pool.mem)
        else:
            assert want["stats"][M.SENT] == n and len({int(e) for e in want["edges"]}) == 1
        with Queue(cl, pool, std, M.TX_UDP, zero_copy) as q:
            q.check(bursts, want)


@MODES
@FORMS
def test_headrooms(cl, std, mode, zero_copy):
    """Headrooms 0-50: 41 / 42 / 43 and 33 / 34 / 35 around the boundary, and every earlier stopping point."""
    pool = M.make_pool(256)
    n = M.fill_headrooms(pool, std, mode)
    want = M.expect(pool, std, [list(range(n))], mode, zero_copy)
    need = 42 if mode == M.TX_UDP else 34
    for H in (need - 1, need, need + 1):
        assert (own(int(want["edges"][4 * H])) != 0) == (H >= need)
    occurs(want, M.SENT, M.ARP, M.HEADROOM, M.NOROUTE, M.PROTO, M.CKSUM)
    with Queue(cl, pool, std, mode, zero_copy) as q:
        q.check([list(range(n))], want)


@MODES
@FORMS
def test_payload_lengths_and_alignments(cl, std, mode, zero_copy):
    pool = M.make_pool(256)
    n = M.fill_lens(pool, std, mode)
    want = M.expect(pool, std, [list(range(n))], mode, zero_copy)
    assert want["stats"][M.CKSUM] == n
    with Queue(cl, pool, std, mode, zero_copy) as q:
        q.check([list(range(n))], want)


def test_checksum_zero_and_wrap(cl, std):
    pool = M.make_pool(64)
    for i in range(64):
        if i < 8:
            M.craft_zero(pool, std, i, 1, length=(2, 18, 333, 17)[i % 4], data_off=192 + i)
        else:
            M.put(pool, std, i, 0, length=18)
    want = M.expect(pool, std, [list(range(64))], M.TX_UDP, True)
    for i in range(8):
        o = i * FRAME + HDR + 192 + i
        assert bytes(want["mem"][o - 2:o]) == b"\xff\xff"
    with Queue(cl, pool, std, M.TX_UDP, True) as q:
        q.check([list(range(64))], want)


def _clip_pool(std):
    pool = M.make_pool(8)
    M.put(pool, std, 0, 1, length=333)
    M.put(pool, std, 1, 1, length=100, data_off=1984 - 10)                   # the buffer holds 10 bytes of it
    M.put(pool, std, 2, M.PCB_TCP, length=100, data_off=1984 - 12)           # TCP field at +16: past the buffer
    M.put(pool, std, 3, M.PCB_TCP, length=100, data_off=1984 - 17)           # ... its first byte inside
    M.put(pool, std, 4, 3, length=1472, data_off=200)
    for i in (5, 6):
        M.put(pool, std, i, 1, length=64)
    M.put(pool, std, 7, 1, length=400, data_off=1984 - 100)
    return pool


@MODES
def test_clipped_by_stage_max_and_buffer(cl, std, mode):
    pool = _clip_pool(std)
    full = M.expect(pool, std, [list(range(8))], mode, False)
    M.rewind(std, full)
    want = M.expect(pool, std, [list(range(8))], mode, False, stage_max=64)
    assert not np.array_equal(full["mem"], want["mem"]) and want["stats"][M.CKSUM] == 8
    with Queue(cl, pool, std, mode, False, stage_max=64) as q:
        q.check([list(range(8))], want)


@MODES
def test_clipped_by_region_end(cl, std, mode):
    pool = _clip_pool(std)
    pool.hdr["buf_len"][7] = 4000                                            # the buffer claims to pass the region's end
    want = M.expect(pool, std, [list(range(8))], mode, True)
    assert want["edges"][7] & M.CKBIT
    with Queue(cl, pool, std, mode, True) as q:
        q.check([list(range(8))], want)


def test_mbuf_outside_the_region(cl, std):
    pool, other = M.make_pool(8), M.make_pool(2)
    for i in range(8):
        M.put(pool, std, i, 1)
    M.put(other, std, 0, 1)
    before = other.mem.copy()
    bursts = [[0, 1, None, 2], [None, 3, 4, 5, 6, 7]]
    want = M.expect(pool, std, bursts, M.TX_UDP, True)
    assert (want["edges"][[2, 4]] == M.EDGE_NONE).all() and want["stats"][M.SENT] + want["stats"][M.ARP] == 8
    with Queue(cl, pool, std, M.TX_UDP, True) as q:
        q.check(bursts, want, outside=other.addr(0))
    assert np.array_equal(other.mem, before)


@FORMS
def test_changes_between_batches(cl, gpu, zero_copy):
    """ident_set, a route, an ARP entry and a PCB attribute changed between batches reach the next batch."""
    w = M.standard_world()
    try:
        pool = M.make_pool(512)
        for i in range(512):
            M.put(pool, w, i, (1, 3, 8)[i % 3], faddr=T.ip_n(("10.1.0.2", "10.1.0.5")[i % 2]), length=18 + i % 50)
        with Queue(cl, pool, w, M.TX_UDP, zero_copy) as q:
            b0 = [list(range(0, 256))]
            want = M.expect(pool, w, b0, M.TX_UDP, zero_copy)
            q.check(b0, want)
            # the counters, then the tables, in the restatement and in the product
            w.tw.ident[2] = 0x1234
            w.set_ident({2: 0x1234})
            w.tw.pcbs[1].ttl, w.tw.pcbs[1].tos, w.tw.pcbs[3].proto = 9, 0x20, 6
            assert X.pcb_tx_set(w.pt, 1, 0x20, 9, 17) == 0 and X.pcb_tx_set(w.pt, 3, 0, 64, 6) == 0
            w.tw.w.rt[1] = (w.tw.w.rt[1][0], 4)                      # 10.2/16 now leaves on netif 4
            assert w.fwd.rt_set(1, w.tw.w.rt[1][0], 4) == 0
            del w.tw.w.arp[2]                                        # 10.1.0.2: arp_request from now on
            assert w.fwd.arp_clear(2) == 0
            pool.mem[256 * FRAME:] = want["mem"][256 * FRAME:]       # (nothing of the second half has moved)
            b1 = [list(range(256, 512))]
            want1 = M.expect(pool, w, b1, M.TX_UDP, zero_copy)
            occurs(want1, M.SENT, M.ARP, M.CKSUM)
            assert want1["ident0"][2] == 0x1234
            q.check(b1, want1)
    finally:
        w.close()


def test_batch_stage_between_queue_batches(cl, gpu):
    """cndp_gpu_ip4_output on the same tables between two queue batches: the counters pass from one to the other."""
    import torch
    from cndp_amd import pktgen
    w = M.standard_world()
    try:
        pool = M.make_pool(512)
        for i in range(512):
            M.put(pool, w, i, M.ROUTED[i % len(M.ROUTED)], length=18 + i % 40)
        with Queue(cl, pool, w, M.TX_UDP, True) as q:
            b0, b1 = [list(range(256))], [list(range(256, 512))]
            q.check(b0, M.expect(pool, w, b0, M.TX_UDP, True))
            n = 300
            pcb, faddr, laddr, ports, length = T.make_inputs(n, w.tw, 77, pcb_pool=M.ROUTED)
            buf, slab_len, stride, offs, data_off, length = T.layout("packed", length, 64, seed=3)
            want_slab = buf.copy()
            ref = T.ip4_output_ref(want_slab, n, w.tw, pcb, faddr, laddr, ports, length, stride=stride,
                                   data_off=data_off, slab_len=slab_len)

            def dev32(a):
                return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(gpu)
            slab_t = torch.from_numpy(buf.copy()).to(gpu)
            fr = pktgen.Frames(slab_t[:slab_len], n, stride=stride, data_off=data_off)
            got = cl.ip4_output(fr, w.fwd, w.pt, dev32(pcb), dev32(faddr), dev32(laddr), dev32(ports),
                                torch.from_numpy(np.ascontiguousarray(length, np.uint16).view(np.int16)).to(gpu))
            torch.cuda.synchronize()
            assert np.array_equal(got["tx_edge"].cpu().numpy().view(np.uint16), ref["tx_edge"])
            assert np.array_equal(slab_t.cpu().numpy(), want_slab)
            assert w.get_ident(w.tw.ident) == w.tw.ident
            q.check(b1, M.expect(pool, w, b1, M.TX_UDP, True))
    finally:
        w.close()


def test_two_queues_one_table(cl, gpu):
    w = M.standard_world()
    try:
        pa, pb = M.make_pool(512), M.make_pool(512)
        for i in range(512):
            M.put(pa, w, i, M.ROUTED[i % len(M.ROUTED)], length=18 + i % 40)
            M.put(pb, w, i, M.ROUTED[(i + 5) % len(M.ROUTED)], length=30 + i % 64, data_off=200)
        with Queue(cl, pa, w, M.TX_UDP, True) as qa, Queue(cl, pb, w, M.TX_UDP, False) as qb:
            for r in range(2):
                b = [list(range(256 * r, 256 * r + 256))]
                wa = M.expect(pa, w, b, M.TX_UDP, True)
                if r:
                    pa.mem[:256 * FRAME] = wa["mem"][:256 * FRAME]
                qa.check(b, wa, flush_each=True)
                wb = M.expect(pb, w, b, M.TX_UDP, False)
                qb.check(b, wb, flush_each=True)
                occurs(wa, M.SENT, M.ARP, M.CKSUM)
    finally:
        w.close()


@FORMS
@pytest.mark.parametrize("hook", ["offset", "null"])
def test_metadata_hooks(cl, std, zero_copy, hook):
    pool = M.make_pool(64)
    for i in range(64):
        M.put(pool, std, i, M.ROUTED[i % len(M.ROUTED)], length=20 + i, md_at=1024 if hook == "offset" else 64)
    kw = {"md_delta": 1024} if hook == "offset" else {"md_null": lambda i: i % 3 == 0}
    want = M.expect(pool, std, [list(range(64))], M.TX_UDP, zero_copy, **kw)
    assert want["stats"][M.NOMD] == (22 if hook == "null" else 0)
    with Queue(cl, pool, std, M.TX_UDP, zero_copy, **kw) as q:
        q.check([list(range(64))], want)


def test_keys_and_arguments(cl, std):
    L = N.lib()
    pool = M.make_pool(4)

    def create(mode=N.CNDP_MQ_IP4_OUTPUT, flags=0, batch=256, depth=2, stage_max=0, umem=None, f=std.fwd.h,
               p=std.pt.h, tx_mode=0, fn=None):
        c, h = N.MqConf(), ctypes.c_void_p()
        c.mode, c.flags, c.batch, c.depth, c.stage_max, c.umem = mode, flags, batch, depth, stage_max, umem
        if fn == "plain":
            r = L.cndp_gpu_mq_create(cl.h, ctypes.byref(c), ctypes.byref(h))
        elif fn == "fwd":
            r = L.cndp_gpu_mq_create_fwd(cl.h, ctypes.byref(c), ctypes.byref(N.MqFwd()), ctypes.byref(h))
        elif fn == "ip4_forward":
            r = L.cndp_gpu_mq_create_ip4_forward(cl.h, ctypes.byref(c), f, ctypes.byref(h))
        elif fn == "udp_input":
            r = L.cndp_gpu_mq_create_udp_input(cl.h, ctypes.byref(c), p, ctypes.byref(h))
        elif fn == "tcp_input":
            r = L.cndp_gpu_mq_create_tcp_input(cl.h, ctypes.byref(c), p, ctypes.byref(h))
        else:
            r = L.cndp_gpu_mq_create_ip4_output(cl.h, ctypes.byref(c), f, p, tx_mode, ctypes.byref(h))
        if r == 0:
            L.cndp_gpu_mq_free(h)
        return r

    assert create() == 0 and create(tx_mode=1) == 0
    for fn in ("plain", "fwd", "ip4_forward", "udp_input", "tcp_input"):    # mode 10 needs its own call
        assert create(fn=fn) == -22, fn
    assert create(f=None) == -22 and create(p=None) == -22 and create(tx_mode=2) == -22
    c = N.MqConf()
    c.mode = N.CNDP_MQ_IP4_OUTPUT
    hh = ctypes.c_void_p()
    assert L.cndp_gpu_mq_create_ip4_output(cl.h, None, std.fwd.h, std.pt.h, 0, ctypes.byref(hh)) == -22
    assert L.cndp_gpu_mq_create_ip4_output(cl.h, ctypes.byref(c), std.fwd.h, std.pt.h, 0, None) == -22
    assert L.cndp_gpu_mq_create_ip4_output(None, ctypes.byref(c), std.fwd.h, std.pt.h, 0, ctypes.byref(hh)) == -22
    for mode in range(10):
        assert create(mode=mode) == -22
    assert create(mode=11) == -22
    for bit in range(32):
        assert create(flags=1 << bit) == -22
    assert create(batch=255) == -22 and create(batch=(1 << 24) + 1) == -22
    assert create(depth=1) == -22 and create(depth=17) == -22            # CNDP_MQ_DEPTH_MAX is 16
    assert create(stage_max=63) == -22 and create(stage_max=65536) == -22
    assert create(umem=pool.base) == -22                                        # not registered
    with Queue(cl, pool, std, M.TX_UDP, True) as q:
        assert all(q.q.stat(k) == 0 for k in KEYS) and L.cndp_gpu_mq_stat(q.q.h, 32) == -22
        assert all(L.cndp_gpu_mq_stat(q.q.h, k) == -22 for k in range(11, 25))    # the UDP and TCP modes' keys
        assert all(q.q.stat(k) == 0 for k in OTHER_KEYS)
        assert q.q.submit(None, 0) == 0
    others = [MbufQueue(cl, N.CNDP_MQ_MAC_SWAP, batch=256, depth=2),
              MbufQueue(cl, N.CNDP_MQ_IP4_FORWARD, batch=256, depth=2, fwd_tbl=std.fwd),
              MbufQueue(cl, N.CNDP_MQ_UDP_INPUT, batch=256, depth=2, pcb_tbl=std.pt),
              MbufQueue(cl, N.CNDP_MQ_TCP_INPUT, batch=256, depth=2, pcb_tbl=std.pt)]
    try:
        for o in others:                                         # the seven keys are this mode's alone
            assert all(L.cndp_gpu_mq_stat(o.h, k) == -22 for k in KEYS) and o.stat(N.CNDP_MQ_STAT_FORWARD) == 0
    finally:
        for o in others:
            o.close()


def test_table_bound_to_another_device(gpu):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU: tables bound to cuda:0 must refuse a queue on cuda:1")
    from cndp_amd.classify import Classifier
    w = M.standard_world()
    c0, c1 = Classifier(0), Classifier(1)
    try:
        pool = M.make_pool(4)
        for i in range(4):
            M.put(pool, w, i, 1)
        with Queue(c0, pool, w, M.TX_UDP, False) as q:       # its first batch binds the tables to cuda:0
            q.check([[0, 1, 2, 3]], M.expect(pool, w, [[0, 1, 2, 3]], M.TX_UDP, False))
        with pytest.raises(OSError) as e:
            MbufQueue(c1, N.CNDP_MQ_IP4_OUTPUT, batch=256, depth=2, fwd_tbl=w.fwd, pcb_tbl=w.pt)
        assert e.value.errno == 22
    finally:
        c0.close()
        c1.close()
        w.close()


@FORMS
def test_echo_loop(cl, gpu, zero_copy):
    """About 300 mbufs through a CNDP_MQ_UDP_INPUT queue and, untouched, through this
    one: every chnl_recv mbuf comes back a frame with addresses and ports swapped,
    both checksums verifying, and bytes equal to the twin chain's."""
    import mq_udp_ref as U
    import l4_ref as R
    w = M.standard_world()
    try:
        tw = w.tw
        uw = type("UdpWorld", (), {})()                          # the same PCB table as the UDP stage's tests see it
        uw.tbl, uw.users, uw.punt, uw.tcp = w.pt, list(range(len(tw.pcbs))), True, False
        uw.ent = np.zeros(len(tw.pcbs), R.ENTRY_DT)
        for k, p in enumerate(tw.pcbs):
            if not p.deleted:
                uw.ent[k] = (p.laddr, p.faddr, p.lport, p.fport, R.CHK if p.cksum else 0)
        n = 300
        pool = M.make_pool(n)
        for i in range(n):
            k = M.ROUTED[i % len(M.ROUTED)] if i % 10 else 4      # PCB 4: no route back; some datagrams match nothing
            U.put(pool, i, src=T.FOREIGN[i % 5], dst=T.LOCALS[k % 7] if k < 28 else "10.11.0.7",
                  sport=40000 + i, dport=(5000 + k if k < 28 else 6000 + k - 28) if i % 17 else 4999,
                  dgram=8 + (0, 1, 18, 333, 1400)[i % 5], data_off=192 + i % 16, cksum="good")
        bursts = M.split(list(range(n)), [256, 44])
        want_u = U.expect(pool, uw, bursts, zero_copy)
        recv = [i for i in range(n) if want_u["edges"][i] == U.UDP_RECV]
        assert len(recv) > 250 and want_u["stats"][U.NOMATCH] > 0
        mid = type("P", (), {})()                                # the pool as the UDP stage leaves it
        mid.mem, mid.base, mid.n = want_u["mem"], pool.base, pool.n
        tb = [recv[:200], recv[200:]]
        want = M.expect(mid, w, tb, M.TX_UDP, zero_copy)
        occurs(want, M.SENT, M.ARP, M.NOROUTE, M.CKSUM)
        if zero_copy:
            cl.host_register(pool.mem)
        try:
            uq = MbufQueue(cl, N.CNDP_MQ_UDP_INPUT, batch=256, depth=2, pcb_tbl=w.pt, max_delay_us=1000000,
                           umem=pool.base if zero_copy else None)
            try:
                addrs, edges = uq.run(pool, np.arange(n), [256, 44])
            finally:
                uq.close()
            assert np.array_equal(edges, want_u["edges"]) and np.array_equal(pool.mem, want_u["mem"])
            assert pool.index_of(addrs[edges == U.UDP_RECV]).tolist() == recv
            with Queue(cl, pool, w, M.TX_UDP, zero_copy, register=False) as q:
                q.check(tb, want)
        finally:
            if zero_copy:
                cl.host_unregister(pool.mem)
        # what came back: the frame that came in, turned round
        seen = 0
        for j, i in enumerate(recv):
            if own(int(want["edges"][j])) == 0:
                continue
            o = i * FRAME + HDR + 192 + i % 16 - 14
            fr = pool.mem[o:o + int(pool.hdr["data_len"][i])]
            assert int(pool.hdr["data_off"][i]) == 192 + i % 16 - 14 and bytes(fr[12:14]) == b"\x08\x00"
            k = M.ROUTED[i % len(M.ROUTED)]
            assert bytes(fr[26:30]) == U._ip(T.LOCALS[k % 7] if k < 28 else "10.11.0.7")
            assert bytes(fr[30:34]) == U._ip(T.FOREIGN[i % 5])
            assert int.from_bytes(bytes(fr[36:38]), "big") == 40000 + i
            assert T.raw_cksum(bytes(fr[14:34])) == 0xFFFF
            if want["edges"][j] & M.CKBIT:
                psd = bytes(fr[26:34]) + bytes([0, 17]) + bytes(fr[38:40])
                c = T.raw_cksum(bytes(fr[34:])) + T.raw_cksum(psd)
                assert ((c >> 16) + (c & 0xFFFF)) & 0xFFFF == 0xFFFF
                seen += 1
        assert seen > 50
    finally:
        w.close()

"""cnet's ip4_forward node as a mode of the asynchronous mbuf queue
(cndp_gpu_mq_create_ip4_forward, include/cndp_mqcnet.h), zero-copy and staged,
over pools of at most 1024 mbufs laid out like CNDP's (batch 256, depth 2).

Every expected value comes twice: from the Python restatement of the node over
mbufs (tests/mq_ip4fwd_ref.py, independent of the library) and from the host
twin (cndp_fwd_node_host) run burst by burst over a copy of the pool.  The
edges, the three counters and the WHOLE pool memory -- mbuf headers and the
bytes the node may not touch included -- are compared exactly."""
import ctypes

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.mbuf import FRAME, MbufQueue

import fwd_ref as R
import mq_ip4fwd_ref as M

pytestmark = pytest.mark.gpu

NONE = N.CNDP_MQ_EDGE_NONE
G = N.CNDP_MQ_EDGE_FWD_GATEWAY
KEYS = (N.CNDP_MQ_STAT_FWD_DIRECT, N.CNDP_MQ_STAT_FWD_GATEWAY, N.CNDP_MQ_STAT_FWD_ARP_REQUEST)
OTHER_KEYS = (N.CNDP_MQ_STAT_FORWARD, N.CNDP_MQ_STAT_ECHO, N.CNDP_MQ_STAT_ACL_PREFILTER, N.CNDP_MQ_STAT_ACL_DENY,
              N.CNDP_MQ_STAT_ACL_PERMIT)
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "staged"])


@pytest.fixture(scope="module")
def cl(gpu):
    from cndp_amd.classify import Classifier
    c = Classifier(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def std(gpu):
    w = R.standard_world()
    arp, rt4, tbl = R.make_tables(w)
    yield w, tbl
    R.close_tables(arp, rt4, tbl)


class Queue:
    """An ip4_forward queue over `pool`, registered first when zero-copy."""

    def __init__(self, cl, pool, tbl, zero_copy, batch=256, **kw):
        self.cl, self.pool, self.zc = cl, pool, zero_copy
        self.seen = [0, 0, 0]
        if zero_copy:
            cl.host_register(pool.mem)
        try:
            # a long max_delay_us: a batch goes out when no further full burst fits, half full with
            # the GPU idle, or flushed
            self.q = MbufQueue(cl, N.CNDP_MQ_IP4_FORWARD, batch=batch, depth=2, umem=pool.base if zero_copy else None,
                               fwd_tbl=tbl, max_delay_us=1000000, **kw)
        except Exception:
            if zero_copy:
                cl.host_unregister(pool.mem)
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.q.close()
        if self.zc:
            self.cl.host_unregister(self.pool.mem)

    def drive(self, bursts, outside=None):
        """Submit bursts of mbuf indices (None: the mbuf at address `outside`) as
        cnet-graph's node would, polling between them, until all are back:
        (addresses, edges) in completion order."""
        q = self.q
        got_a, got_e = [], []
        for b in bursts:
            ptrs = (ctypes.c_void_p * len(b))(*[outside if i is None else self.pool.addr(int(i)) for i in b])
            done = 0
            while done < len(b):
                k = q.submit(ctypes.addressof(ptrs) + done * ctypes.sizeof(ctypes.c_void_p), len(b) - done)
                done += k
                a, e = q.poll()
                got_a.append(a)
                got_e.append(e)
                if k == 0 and a.size == 0:
                    q.wait()
        for _ in range(64):
            if not q.pending:
                break
            q.flush()
            q.wait()
            a, e = q.poll()
            got_a.append(a)
            got_e.append(e)
        assert q.pending == 0
        return np.concatenate(got_a), np.concatenate(got_e)

    def check(self, bursts, want, outside=None):
        """One pass of `bursts` through the queue against `want` (M.expect)."""
        addrs, edges = self.drive(bursts, outside)
        sent = [outside if i is None else self.pool.addr(int(i)) for b in bursts for i in b]
        assert addrs.tolist() == sent, "mbufs came back out of submission order"
        bad = np.nonzero(edges != want["edges"])[0]
        assert len(bad) == 0, (f"edges: {len(bad)} differ, first at {bad[0]}: got {edges[bad[0]]:#x} "
                               f"want {want['edges'][bad[0]]:#x}")
        bad = np.nonzero(self.pool.mem != want["mem"])[0]
        assert len(bad) == 0, (f"pool memory: {len(bad)} bytes differ, first at mbuf {bad[0] // FRAME} + {bad[0] % FRAME}: "
                               f"got {self.pool.mem[bad[0]]:#x} want {want['mem'][bad[0]]:#x}")
        self.seen = [a + b for a, b in zip(self.seen, want["stats"])]
        assert [self.q.stat(k) for k in KEYS] == self.seen
        assert all(self.q.stat(k) == 0 for k in OTHER_KEYS)         # other modes' families
        return edges


@FORMS
@pytest.mark.parametrize("batch", [256, 512])
def test_burst_sizes(cl, std, zero_copy, batch):
    """Bursts of 1 ... 256 in one run: tails, groups at chunk ends (63, 65, 255),
    frames at all four alignments.  A batch is launched as soon as no further
    256-mbuf burst fits, so at batch 256 every burst is a batch of its own; at
    batch 512 several bursts share a batch (1 ... 65 make 222 mbufs, 255 more
    477) and a batch boundary falls between two bursts (255 | 256)."""
    w, tbl = std
    pool = M.make_pool(sum(M.BURST_SIZES))
    M.fill_random(pool, 3, data_offs=(214, 215, 216, 217))
    bursts = M.split(list(range(pool.n)), M.BURST_SIZES)
    want = M.expect(pool, w, tbl, bursts, zero_copy)
    assert all(want["stats"])
    with Queue(cl, pool, tbl, zero_copy, batch=batch) as q:
        q.check(bursts, want)
        assert q.q.stat(N.CNDP_MQ_STAT_MBUFS) == pool.n
        nb = q.q.stat(N.CNDP_MQ_STAT_BATCHES)
        assert nb == len(bursts) if batch == 256 else 2 <= nb < len(bursts)


@FORMS
def test_group_rules(cl, std, zero_copy):
    """test_group_rules of tests/test_fwd_gpu.py over mbufs, each group's outcome
    spelt out, and one group's four mbufs again as four bursts of one."""
    w, tbl = std
    pool = M.make_pool(40)
    bursts = M.fill_groups(pool)
    want = M.expect(pool, w, tbl, bursts, zero_copy)
    assert want["edges"].tolist() == [e for g in M.GROUP_EDGES for e in g]
    with Queue(cl, pool, tbl, zero_copy) as q:
        edges = q.check(bursts, want)
    assert edges[:4].tolist() != edges[-4:].tolist()                # where the reference differs
    # the quirk on the wire: lane 2 of C's first group carries gateway 0's MAC as d_addr
    f = pool.mem[bursts[2][2] * FRAME + 64 + 192:][:12]
    assert bytes(f[:6]) == w.arp[1][1] and bytes(f[6:]) == w.netif[4]


@FORMS
def test_l2_len_and_alignment(cl, std, zero_copy):
    """l2_len 0, 2, 14, 18, 22 at data_off 206 ... 209 (so the frames and their
    MAC bytes take every alignment, and for l2_len < 12 the MACs lie over the IP
    header), and l2_len above data_off."""
    w, tbl = std
    pool = M.make_pool(80)
    n = M.fill_l2(pool)
    bursts = M.split(list(range(n)), [16, 7, n - 23])
    want = M.expect(pool, w, tbl, bursts, zero_copy)
    assert all(want["stats"])
    with Queue(cl, pool, tbl, zero_copy) as q:
        q.check(bursts, want)
    i = n - 8       # l2_len 14 above data_off 10: edited and sent on, neither adjusted nor rewritten
    assert (int(pool.hdr["data_off"][i]), int(pool.hdr["data_len"][i])) == (10, 46) and want["edges"][i] == 1 + 2


@FORMS
def test_readable_end(cl, zero_copy):
    """x bytes of the last mbuf's IP header readable: the region ends there
    (zero-copy), or its buf_len does (staged).  0.0.0.0 -- what an unreadable
    destination reads as -- has an ARP entry, so MAC bytes cross the end too."""
    w = R.standard_world()
    w.arp[7] = (3, bytes([2, 0xEE, 0, 0, 0, 7]))
    w.arp_fib.add(0, 32, 7)
    arp, rt4, tbl = R.make_tables(w)
    try:
        pool = M.make_pool(8)
        with Queue(cl, pool, tbl, zero_copy) as q:
            for x, l2 in ((1, 14), (5, 0), (9, 2), (11, 0), (12, 14), (17, 14), (19, 18), (20, 22)):
                for i in range(8):
                    M.put(pool, i, M.D if i % 2 else M.G1, l2=l2)
                if zero_copy:
                    M.put(pool, 7, M.D, l2=l2, data_off=FRAME - 64 - x)
                else:
                    pool.hdr["buf_len"][7] = int(pool.hdr["data_off"][7]) + x
                bursts = [[0, 1, 2], [4, 5, 6, 7]]
                want = M.expect(pool, w, tbl, bursts, zero_copy)
                assert want["edges"][6] != NONE
                q.check(bursts, want)
    finally:
        R.close_tables(arp, rt4, tbl)


def test_mbuf_outside_region(cl, std):
    """Zero-copy: an mbuf of another, unregistered pool in the middle of a group
    and as a group's lane 0: EDGE_NONE, untouched, its neighbours as the group
    rules have them without it."""
    w, tbl = std
    pool, other = M.make_pool(12), M.make_pool(1, seed=5)
    for i, d in enumerate([M.G1, M.G2, M.G4, M.G6, M.G1, M.G2, M.G4, M.G6, M.D, M.G1, M.G2, M.G4]):
        M.put(pool, i, d)
    M.put(other, 0, M.D)
    before = other.mem.copy()
    bursts = [[0, None, 2, 3], [None, 5, 6, 7], [8, 9, None, 11, 1]]
    want = M.expect(pool, w, tbl, bursts, True)
    assert want["edges"].tolist() == [4 | G, NONE, 6 | G, 2 | G, NONE, 5 | G, 6 | G, 2 | G, 3, 1, NONE, 1, 5 | G]
    with Queue(cl, pool, tbl, True) as q:
        q.check(bursts, want, outside=other.addr(0))
    assert np.array_equal(other.mem, before)
    assert bytes(pool.mem[2 * FRAME + 256:][:6]) == w.arp[1][1]        # lane 0's gateway entry
    assert bytes(pool.mem[6 * FRAME + 256:][:6]) == w.arp[14][1]       # its own: lane 0 was not taken


@FORMS
def test_table_changes_between_batches(cl, zero_copy):
    """An ARP object set and cleared, a netif MAC and a route added to the rt4
    FIB, each followed by a batch that must see it."""
    w = R.standard_world()
    arp, rt4, tbl = R.make_tables(w)
    dsts = [M.D, "10.1.0.77", "10.2.200.9", M.G1, M.G2, M.NR, M.D]
    bursts = [[0, 1, 2], [3, 4, 5, 6]]
    try:
        pool = M.make_pool(7)
        with Queue(cl, pool, tbl, zero_copy) as q:
            def once():
                for i, d in enumerate(dsts):
                    M.put(pool, i, d, ttl=9 + i)
                want = M.expect(pool, w, tbl, bursts, zero_copy)
                return q.check(bursts, want)

            assert once().tolist() == [3, 1, 4 | G, 1, 1, 1, 3]
            ha = bytes([2, 0xDD, 1, 2, 3, 4])
            assert tbl.arp_set(2, 5, ha) == 0                       # an ARP object replaced ...
            w.arp[2] = (5, ha)
            assert once()[0] == 5 + 2 and bytes(pool.mem[256:262]) == ha
            assert tbl.arp_clear(2) == 0                            # ... and cleared
            del w.arp[2]
            assert once().tolist() == [1, 1, 4 | G, 4 | G, 5 | G, 1, 1]
            mac = bytes([2, 0x77, 0, 0, 0, 1])
            assert tbl.netif_set(2, mac) == 0                       # a netif's MAC
            w.netif[2] = mac
            once()
            assert bytes(pool.mem[2 * FRAME + 256 + 6:][:6]) == mac
            assert rt4.add(R.ip_h("10.2.200.0"), 24, 2) == 0        # a more specific route in the rt4 FIB
            w.rt_fib.add(R.ip_h("10.2.200.0"), 24, 2)
            assert once()[2] == 3 + 2 | G
            assert arp.add(R.ip_h("10.1.0.77"), 32, 6) == 0         # an ARP /32
            w.arp_fib.add(R.ip_h("10.1.0.77"), 32, 6)
            assert once()[1] == 5 + 2
    finally:
        R.close_tables(arp, rt4, tbl)


def test_batch_call_and_queue_share_the_mirror(cl, gpu):
    """cndp_gpu_ip4_forward on a batch, the queue, a table change, the queue and
    the batch call again, all on one table: each sees the table as it is."""
    import torch
    from cndp_amd import pktgen
    w = R.standard_world()
    arp, rt4, tbl = R.make_tables(w)
    dsts = [M.D, M.G1, M.G2, M.NR, M.D, M.D, M.G4]
    n = len(dsts)
    try:
        def batch_call():
            slab = np.concatenate([np.resize(R.ip4_frame(d), 64) for d in dsts])
            ref = slab.copy()
            slab_t = torch.from_numpy(slab.copy()).to(gpu)
            out = {"nh": torch.full((n,), 1 << 24, dtype=torch.int32, device=gpu),
                   "rxmeta": torch.full((n,), 14, dtype=torch.int32, device=gpu)}
            got = cl.ip4_forward(pktgen.Frames(slab_t, n, stride=64), out, tbl, burst=8,
                                 sel=torch.ones(n, dtype=torch.uint8, device=gpu))
            torch.cuda.synchronize()
            want = R.ip4_forward_ref(ref, n, np.full(n, 14, np.uint32), 8, w, sel=np.ones(n, np.uint8), stride=64)
            assert np.array_equal(got["fwd_edge"].cpu().numpy().view(np.uint16), want["fwd_edge"])
            assert np.array_equal(slab_t.cpu().numpy(), ref)
            return want["fwd_edge"]

        first = batch_call()
        pool = M.make_pool(n)
        with Queue(cl, pool, tbl, True) as q:
            def once():
                for i, d in enumerate(dsts):
                    M.put(pool, i, d)
                return q.check([list(range(n))], M.expect(pool, w, tbl, [list(range(n))], True))

            assert (once() & N.CNDP_MQ_EDGE_FWD_MASK).tolist() == first.tolist()
            assert tbl.arp_clear(2) == 0
            del w.arp[2]
            e = once()
            assert e[0] == 1 and e[6] == 4 + 2 | G
            assert (e & N.CNDP_MQ_EDGE_FWD_MASK).tolist() == batch_call().tolist()
            ha = bytes([2, 0xDD, 9, 9, 9, 9])
            assert tbl.arp_set(2, 4, ha) == 0
            w.arp[2] = (4, ha)
            assert batch_call()[0] == 4 + 2 and once()[0] == 4 + 2
    finally:
        R.close_tables(arp, rt4, tbl)


def test_arguments(cl, std):
    w, tbl = std
    L = N.lib()
    pool = M.make_pool(4)

    def create(mode=N.CNDP_MQ_IP4_FORWARD, flags=0, batch=256, depth=2, stage_max=0, umem=None, t=tbl.h, fn=None):
        c, h = N.MqConf(), ctypes.c_void_p()
        c.mode, c.flags, c.batch, c.depth, c.stage_max, c.umem = mode, flags, batch, depth, stage_max, umem
        if fn == "plain":
            r = L.cndp_gpu_mq_create(cl.h, ctypes.byref(c), ctypes.byref(h))
        elif fn == "fwd":
            r = L.cndp_gpu_mq_create_fwd(cl.h, ctypes.byref(c), ctypes.byref(N.MqFwd()), ctypes.byref(h))
        else:
            r = L.cndp_gpu_mq_create_ip4_forward(cl.h, ctypes.byref(c), t, ctypes.byref(h))
        if r == 0:
            L.cndp_gpu_mq_free(h)
        return r

    assert create() == 0
    assert create(fn="plain") == -22 and create(fn="fwd") == -22                # mode 7 needs its own create call
    assert create(t=None) == -22
    c = N.MqConf()
    c.mode = N.CNDP_MQ_IP4_FORWARD
    assert L.cndp_gpu_mq_create_ip4_forward(cl.h, None, tbl.h, ctypes.byref(ctypes.c_void_p())) == -22
    assert L.cndp_gpu_mq_create_ip4_forward(cl.h, ctypes.byref(c), tbl.h, None) == -22
    assert L.cndp_gpu_mq_create_ip4_forward(None, ctypes.byref(c), tbl.h, ctypes.byref(ctypes.c_void_p())) == -22
    for mode in (N.CNDP_MQ_IP4_LOOKUP, N.CNDP_MQ_CNET, N.CNDP_MQ_MAC_SWAP, N.CNDP_MQ_IP4_REWRITE, N.CNDP_MQ_CFWD_FWD,
                 N.CNDP_MQ_ACL_FWD, 8):
        assert create(mode=mode) == -22
    for bit in range(8):
        assert create(flags=1 << bit) == -22
    assert create(batch=255) == -22 and create(batch=(1 << 24) + 1) == -22
    assert create(depth=1) == -22 and create(depth=17) == -22            # CNDP_MQ_DEPTH_MAX is 16
    assert create(stage_max=63) == -22 and create(stage_max=65536) == -22
    assert create(umem=pool.base) == -22                                        # not registered
    with Queue(cl, pool, tbl, True) as q:
        assert q.q.stat(N.CNDP_MQ_STAT_FWD_DIRECT) == 0 and L.cndp_gpu_mq_stat(q.q.h, 11) == -22
        assert q.q.submit(None, 0) == 0


def test_table_bound_to_another_device(std, gpu):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU: a table bound to cuda:0 must refuse a queue on cuda:1")
    from cndp_amd.classify import Classifier
    w = R.standard_world()
    arp, rt4, tbl = R.make_tables(w)
    c0, c1 = Classifier(0), Classifier(1)
    try:
        pool = M.make_pool(4)
        for i in range(4):
            M.put(pool, i, M.D)
        with Queue(c0, pool, tbl, False) as q:     # its first batch binds the table to cuda:0
            q.check([[0, 1, 2, 3]], M.expect(pool, w, tbl, [[0, 1, 2, 3]], False))
        with pytest.raises(OSError) as e:
            MbufQueue(c1, N.CNDP_MQ_IP4_FORWARD, batch=256, depth=2, fwd_tbl=tbl)
        assert e.value.errno == 22
    finally:
        c0.close()
        c1.close()
        R.close_tables(arp, rt4, tbl)

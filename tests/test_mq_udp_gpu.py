"""cnet's ip4_proto + udp_input nodes as a mode of the asynchronous mbuf queue
(cndp_gpu_mq_create_udp_input, include/cndp_mql4.h), zero-copy and staged, over
pools of at most 1024 mbufs laid out like CNDP's.

Every expected value comes twice: from the Python restatement of the nodes over
mbufs (tests/mq_udp_ref.py, independent of the library) and from the host twin
(cndp_udp_input_node_host) run burst by burst over a copy of the pool.  The
edges, the six counters, the order of return and the WHOLE pool memory -- mbuf
headers, metadata and the frames, which the nodes never write -- are compared
exactly."""
import ctypes

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.mbuf import FRAME, MbufQueue

import l4_ref as R
import mq_udp_ref as M

pytestmark = pytest.mark.gpu

KEYS = (N.CNDP_MQ_STAT_L4_RECV, N.CNDP_MQ_STAT_L4_NOMATCH, N.CNDP_MQ_STAT_L4_CKSUM, N.CNDP_MQ_STAT_L4_PROTO_DROP,
        N.CNDP_MQ_STAT_L4_TCP, N.CNDP_MQ_STAT_L4_NOMD)
OTHER_KEYS = (N.CNDP_MQ_STAT_FORWARD, N.CNDP_MQ_STAT_ECHO, N.CNDP_MQ_STAT_ACL_PREFILTER, N.CNDP_MQ_STAT_ACL_DENY,
              N.CNDP_MQ_STAT_ACL_PERMIT, N.CNDP_MQ_STAT_FWD_DIRECT, N.CNDP_MQ_STAT_FWD_GATEWAY,
              N.CNDP_MQ_STAT_FWD_ARP_REQUEST)
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "staged"])


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


class Queue:
    """A udp_input queue over `pool`, registered first when zero-copy."""

    def __init__(self, cl, pool, world, zero_copy, batch=256, depth=2, md_delta=None, md_null=None, **kw):
        self.cl, self.pool, self.zc = cl, pool, zero_copy
        self.seen = [0] * 6
        hook = None
        if md_delta is not None or md_null is not None:
            def hook(m):
                if md_null is not None and md_null((m - pool.base) // FRAME):
                    return None
                return m + (64 if md_delta is None else md_delta)
        if zero_copy:
            cl.host_register(pool.mem)
        try:
            # a long max_delay_us: a batch goes out when no further full burst fits, half full with
            # the GPU idle, or flushed
            self.q = MbufQueue(cl, N.CNDP_MQ_UDP_INPUT, batch=batch, depth=depth, umem=pool.base if zero_copy else None,
                               pcb_tbl=world.tbl, max_delay_us=1000000, metadata=hook, **kw)
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

    def drive(self, bursts, outside=None, flush_each=False):
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
                if flush_each:
                    q.flush()
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
        self.seen = [a + b for a, b in zip(self.seen, want["stats"])]
        assert [self.q.stat(k) for k in KEYS] == self.seen
        assert all(self.q.stat(k) == 0 for k in OTHER_KEYS)         # other modes' families
        return edges


@FORMS
@pytest.mark.parametrize("batch,depth", [(256, 2), (512, 4)])
def test_batch_shapes(cl, std, zero_copy, batch, depth):
    """1, 63, 64, 65, 256, 257 and 600 mbufs in bursts with tails: waves with a
    tail, batches of one burst (batch 256) and of several, bursts split over
    submit calls (257, 600), more batches than the depth."""
    sizes = [1, 63, 64, 65, 256, 257, 600 - 6 - 300]
    pool = M.make_pool(1000)
    M.fill_mix(pool)
    bursts = M.split(list(range(1000)), sizes)
    want = M.expect(pool, std, bursts, zero_copy)
    assert all(want["stats"][k] for k in (M.RECV, M.NOMATCH, M.CKSUM, M.PDROP)) and sum(want["stats"]) == 1000
    with Queue(cl, pool, std, zero_copy, batch=batch, depth=depth) as q:
        q.check(bursts, want)
        assert q.q.stat(N.CNDP_MQ_STAT_MBUFS) == 1000 and q.q.stat(N.CNDP_MQ_STAT_BATCHES) >= 1000 // batch
    # 600 mbufs as one burst
    pool = M.make_pool(600)
    M.fill_mix(pool, seed=6)
    want = M.expect(pool, std, [list(range(600))], zero_copy)
    with Queue(cl, pool, std, zero_copy, batch=batch, depth=depth) as q:
        q.check([list(range(600))], want)


@FORMS
@pytest.mark.parametrize("punt,tcp", [(True, False), (False, True)])
def test_lookup_classes(cl, gpu, zero_copy, punt, tcp):
    w = M.standard_world()
    try:
        w.set_flags(punt, tcp)
        pool = M.make_pool(64)
        n = M.fill_lookup(pool)
        want = M.expect(pool, w, [list(range(n))], zero_copy)
        st = want["stats"]
        assert st[M.RECV] and st[M.NOMATCH] and st[M.CKSUM] and bool(st[M.TCP]) == tcp and st[M.PDROP]
        miss = M.UDP_PUNT if punt else M.UDP_DROP
        assert want["edges"][:14].tolist() == [M.UDP_RECV] * 6 + [miss, M.UDP_RECV, miss] + [M.UDP_RECV] * 3 + [miss, miss]
        with Queue(cl, pool, w, zero_copy) as q:
            q.check([list(range(n))], want)
        # all six counters' classes in one run: the same frames with a hook answering NULL for some
        pool = M.make_pool(64)
        M.fill_lookup(pool)
        want = M.expect(pool, w, [list(range(n))], zero_copy, md_null=lambda i: i % 7 == 2)
        assert all(want["stats"][k] for k in (M.RECV, M.NOMATCH, M.CKSUM, M.PDROP, M.NOMD)) and bool(want["stats"][M.TCP]) == tcp
        with Queue(cl, pool, w, zero_copy, md_null=lambda i: i % 7 == 2) as q:
            q.check([list(range(n))], want)
    finally:
        w.close()


@FORMS
def test_checksum(cl, std, zero_copy):
    """Every length of M.DGRAM_LENS (the last few beyond 255 readable bytes) at
    every mtod alignment, l3_len 20 / 24 / 60, good sums and corrupted first /
    last bytes; field 0; a sum of 0xFFFF; total_length below the IHL and above
    data_len."""
    pool = M.make_pool(512)
    n, sp = M.fill_cksum(pool)
    bursts = M.split(list(range(n)), [256, n - 256])
    want = M.expect(pool, std, bursts, zero_copy)
    assert (want["edges"][:sp // 2] == M.UDP_RECV).all() and (want["edges"][sp // 2:sp] == (M.UDP_DROP | M.CK)).all()
    assert want["stats"][M.CKSUM] and want["stats"][M.RECV]
    with Queue(cl, pool, std, zero_copy, batch=512) as q:
        q.check(bursts, want)


def test_checksum_stage_max(cl, std):
    """Staged, stage_max = 128: a 256-byte datagram is clipped."""
    pool = M.make_pool(512)
    n, sp = M.fill_cksum(pool)
    idx = list(range(sp, n))
    want = M.expect(pool, std, [idx], False, stage_max=128)
    assert want["edges"][7] == M.UDP_DROP | M.CK and want["edges"][1] == M.UDP_RECV
    with Queue(cl, pool, std, False, stage_max=128) as q:
        q.check([idx], want)


def test_checksum_region_end(cl, std):
    """Zero-copy: the pool's last mbuf with its datagram ending exactly at the
    region's end, and reaching past it."""
    for over, ck in ((0, "good"), (0, "last"), (2, "good"), (40, "good")):
        pool = M.make_pool(4)
        for i in range(4):
            M.put(pool, i, dport=5002, dgram=100, cksum=ck)
        M.put(pool, 3, dport=5002, dgram=100, l3=24, data_off=FRAME - 64 - 124 + over, cksum=ck)
        pool.hdr["buf_len"][3] = 4000
        want = M.expect(pool, std, [[0, 1], [2, 3]], True)
        assert want["edges"][3] == (M.UDP_RECV if over == 0 and ck == "good" else M.UDP_DROP | M.CK)
        with Queue(cl, pool, std, True) as q:
            q.check([[0, 1], [2, 3]], want)


@FORMS
def test_checksum_waves(cl, std, zero_copy):
    """Waves holding exactly 0, 1, 4, 5 and 64 lanes that need a verify."""
    pool = M.make_pool(320)
    n = M.fill_waves(pool)
    bursts = M.split(list(range(n)), [256, 64])
    want = M.expect(pool, std, bursts, zero_copy)
    assert want["stats"][M.CKSUM] == 25 and want["stats"][M.RECV] == 295
    # one batch (it stays below half of 1024 until the flush): wave k holds mbufs 64 k ... 64 k + 63
    with Queue(cl, pool, std, zero_copy, batch=1024) as q:
        q.check(bursts, want)
        assert q.q.stat(N.CNDP_MQ_STAT_BATCHES) == 1


@FORMS
def test_image_in_lds(cl, std, zero_copy):
    """CNDP_TUNE_MQ_PCB_LDS: the kernel variant that looks up in an LDS copy of the
    table image gives the same results (lookup classes, checksums, waves)."""
    cl.set_tuning(mq_pcb_lds=1)
    try:
        pool = M.make_pool(448)
        n = M.fill_lookup(pool)
        for i in range(n, 448):
            M.put(pool, i, dport=5002, dgram=8 + (i * 7) % 300, l3=M.L3_LENS[i % 3], data_off=192 + i % 16,
                  cksum="last" if i % 5 == 0 else "good")
        bursts = M.split(list(range(448)), [256, 192])
        want = M.expect(pool, std, bursts, zero_copy)
        assert all(want["stats"][k] for k in (M.RECV, M.NOMATCH, M.CKSUM, M.PDROP))
        with Queue(cl, pool, std, zero_copy, batch=512) as q:
            q.check(bursts, want)
    finally:
        cl.set_tuning(mq_pcb_lds=0)
    assert N.lib().cndp_gpu_set_tuning(cl.h, N.CNDP_TUNE_MQ_PCB_LDS, 2) == -22


@FORMS
def test_adj_offset_refuses(cl, std, zero_copy):
    pool = M.make_pool(8)
    n = M.fill_adj(pool)
    want = M.expect(pool, std, [list(range(n))], zero_copy)
    assert (want["edges"] == M.UDP_RECV).all()
    with Queue(cl, pool, std, zero_copy) as q:
        q.check([list(range(n))], want)
    assert (int(pool.hdr["data_off"][1]), int(pool.hdr["data_len"][1])) == (192, 120)
    assert (int(pool.hdr["data_off"][3]), int(pool.hdr["data_len"][3])) == (192, 60)


@FORMS
@pytest.mark.parametrize("hook", ["default", "offset", "null"])
def test_metadata_hooks(cl, std, zero_copy, hook):
    pool = M.make_pool(48)
    M.fill_mix(pool, seed=9)
    kw = {"default": {}, "offset": {"md_delta": 128}, "null": {"md_delta": 128, "md_null": lambda i: i % 3 == 0}}[hook]
    bursts = [list(range(20)), list(range(20, 48))]
    want = M.expect(pool, std, bursts, zero_copy, **kw)
    assert bool(want["stats"][M.NOMD]) == (hook == "null") and want["stats"][M.RECV]
    with Queue(cl, pool, std, zero_copy, **kw) as q:
        q.check(bursts, want)


@FORMS
def test_table_changes_between_batches(cl, gpu, zero_copy):
    """Add, delete, flags, user value; a flush between the changes; batches of a
    queue of depth 4 still in flight when the table changes."""
    w = M.standard_world()
    try:
        pool = M.make_pool(256)
        idx = list(range(64))
        with Queue(cl, pool, w, zero_copy, depth=4) as q:
            def once():
                M.fill_mix(pool, seed=21)
                for i in range(0, 64, 8):
                    M.put(pool, i, dport=7000, dst=M.OTHER)
                    M.put(pool, i + 1, proto=6)
                want = M.expect(pool, w, [idx[:40], idx[40:]], zero_copy)
                return q.check([idx[:40], idx[40:]], want, flush_each=True)

            e = once()
            assert e[0] == M.UDP_PUNT and e[1] == M.PROTO_DROP
            new = w.add(lport=7000, user=0x5555000012345678)          # a PCB added
            e = once()
            assert e[0] == M.UDP_RECV and int(pool.hdr["udata64"][0]) == 0x5555000012345678
            w.user_set(new, 42)                                        # its user value changed
            once()
            assert int(pool.hdr["udata64"][8]) == 42
            w.set_flags(False, True)                                   # punt off, TCP on
            w.delete(new)                                              # and the PCB deleted
            e = once()
            assert e[0] == M.UDP_DROP and e[1] == M.PROTO_TCP
            # changes while batches are in flight reach the batches launched after them
            M.fill_mix(pool, seed=22)
            for i in range(256):
                M.put(pool, i, dport=7001)
            ptrs = pool.ptrs(np.arange(256))
            mem0 = pool.mem.copy()
            assert q.q.submit(ptrs, 128) == 128
            q.q.flush()
            ent0, users0 = w.ent.copy(), list(w.users)                 # the table as the first batch saw it
            w.add(lport=7001)
            w.set_flags(True, True)
            assert q.q.submit(ctypes.addressof(ptrs) + 128 * 8, 128) == 128
            q.q.flush()
            got_e = []
            while q.q.pending:
                q.q.wait()
                got_e.append(q.q.poll()[1])
            e = np.concatenate(got_e)
            assert (e[:128] == M.UDP_DROP).all() and (e[128:] == M.UDP_RECV).all()
            mem = mem0.copy()
            e1, _ = M.node_ref(mem, pool.base, ent0, users0, [i * FRAME for i in range(128)], zero_copy, 2048,
                               False, True)
            e2, _ = M.node_ref(mem, pool.base, w.ent, w.users, [i * FRAME for i in range(128, 256)], zero_copy, 2048,
                               True, True)
            assert np.array_equal(e, np.concatenate([e1, e2])) and np.array_equal(pool.mem, mem)
    finally:
        w.close()


def test_one_table_two_readers(cl, gpu):
    """cndp_gpu_udp_input on another stream against the same table while queue
    batches are in flight; both results are right."""
    import torch
    from cndp_amd import pktgen
    w = M.standard_world()
    try:
        pool = M.make_pool(512)
        M.fill_mix(pool, seed=31)
        n = 512
        rows = pool.mem.reshape(n, FRAME)
        slab = np.zeros((n, 512), np.uint8)
        for i in range(n):
            o = 64 + int(pool.hdr["data_off"][i])
            slab[i] = rows[i, o:o + 512]
        l3 = ((pool.hdr["tx_offload"] >> 7) & 0x1FF).astype(np.uint32)
        rxmeta = (l3 << 7 | 8 << 16).astype(np.uint32)
        slab_t = torch.from_numpy(slab.reshape(-1).copy()).to(gpu)
        out = {"nh": torch.full((n,), 2 << 24, dtype=torch.int32, device=gpu),
               "rxmeta": torch.from_numpy(rxmeta.view(np.int32).copy()).to(gpu)}
        sel = torch.ones(n, dtype=torch.uint8, device=gpu)
        want_b = R.udp_input_ref(slab.reshape(-1), n, np.full(n, 2 << 24, np.uint32), rxmeta, w.ent, sel=np.ones(n, np.uint8),
                                 stride=512, punt=True, tcp=False)
        bursts = M.split(list(range(n)), [256, 256])
        want = M.expect(pool, w, bursts, True)
        side = torch.cuda.Stream(device=gpu)
        with Queue(cl, pool, w, True, depth=4) as q:
            ptrs = pool.ptrs(np.arange(n))
            assert q.q.submit(ptrs, 256) == 256                       # a batch of its own, launched at once
            with torch.cuda.stream(side):
                l4 = cl.udp_input(pktgen.Frames(slab_t, n, stride=512), out, w.tbl, sel=sel, stream=side.cuda_stream)
            assert q.q.submit(ctypes.addressof(ptrs) + 256 * 8, 256) == 256
            with torch.cuda.stream(side):
                l4b = cl.udp_input(pktgen.Frames(slab_t, n, stride=512), out, w.tbl, sel=sel, stream=side.cuda_stream)
            got_a, got_e = [], []
            while q.q.pending:
                q.q.wait()
                a, e = q.q.poll()
                got_a.append(a)
                got_e.append(e)
            side.synchronize()
            assert np.concatenate(got_a).tolist() == [pool.addr(i) for i in range(n)]
            assert np.array_equal(np.concatenate(got_e), want["edges"]) and np.array_equal(pool.mem, want["mem"])
            assert [q.q.stat(k) for k in KEYS] == want["stats"]
        for r in (l4, l4b):
            assert np.array_equal(r["l4edge"].cpu().numpy(), want_b["l4edge"])
            assert np.array_equal(r["pcb"].cpu().numpy().view(np.uint32), want_b["pcb"])
            assert np.array_equal(r["stats"].cpu().numpy().astype(np.uint64), want_b["stats"])
    finally:
        w.close()


def test_zero_copy_out_of_region(cl, std):
    """mbufs outside every registered region: CNDP_MQ_EDGE_NONE, untouched, counted
    nowhere; a frame outside (buf_addr elsewhere) likewise; the others unaffected."""
    pool = M.make_pool(8)
    other = M.make_pool(2, seed=3)
    for i in range(8):
        M.put(pool, i, dport=5000 + i % 3)
    M.put(other, 0, dport=5000)
    keep = other.mem.copy()
    bursts = [[0, None, 2, 3], [None, 5, 6, 7]]
    want = M.expect(pool, std, bursts, True)
    with Queue(cl, pool, std, True) as q:
        e = q.check(bursts, want, outside=other.addr(0))
        assert e[1] == N.CNDP_MQ_EDGE_NONE and e[4] == N.CNDP_MQ_EDGE_NONE and np.array_equal(other.mem, keep)
        assert sum(q.q.stat(k) for k in KEYS) == 6
        # an mbuf of the pool whose buffer lies outside it
        for i in range(8):
            M.put(pool, i, dport=5000)
        pool.hdr["buf_addr"][5] = other.addr(0) + 64
        before = pool.mem.copy()
        addrs, e = q.drive([list(range(8))])
        assert e[5] == N.CNDP_MQ_EDGE_NONE and (np.delete(e, 5) == M.UDP_RECV).all()
        assert np.array_equal(pool.mem[5 * FRAME:6 * FRAME], before[5 * FRAME:6 * FRAME]) and np.array_equal(other.mem, keep)
        assert sum(q.q.stat(k) for k in KEYS) == 6 + 7


def test_arguments(cl, std):
    L = N.lib()
    pool = M.make_pool(4)
    tbl = std.tbl

    def create(mode=N.CNDP_MQ_UDP_INPUT, flags=0, batch=256, depth=2, stage_max=0, umem=None, t=tbl.h, fn=None):
        c, h = N.MqConf(), ctypes.c_void_p()
        c.mode, c.flags, c.batch, c.depth, c.stage_max, c.umem = mode, flags, batch, depth, stage_max, umem
        if fn == "plain":
            r = L.cndp_gpu_mq_create(cl.h, ctypes.byref(c), ctypes.byref(h))
        elif fn == "fwd":
            r = L.cndp_gpu_mq_create_fwd(cl.h, ctypes.byref(c), ctypes.byref(N.MqFwd()), ctypes.byref(h))
        elif fn == "ip4_forward":
            import fwd_ref
            arp, rt4, ft = fwd_ref.make_tables(fwd_ref.standard_world())
            r = L.cndp_gpu_mq_create_ip4_forward(cl.h, ctypes.byref(c), ft.h, ctypes.byref(h))
            if r == 0:
                L.cndp_gpu_mq_free(h)
            fwd_ref.close_tables(arp, rt4, ft)
            return r
        else:
            r = L.cndp_gpu_mq_create_udp_input(cl.h, ctypes.byref(c), t, ctypes.byref(h))
        if r == 0:
            L.cndp_gpu_mq_free(h)
        return r

    assert create() == 0
    assert create(fn="plain") == -22 and create(fn="fwd") == -22 and create(fn="ip4_forward") == -22   # mode 8 needs its own call
    assert create(t=None) == -22
    c = N.MqConf()
    c.mode = N.CNDP_MQ_UDP_INPUT
    assert L.cndp_gpu_mq_create_udp_input(cl.h, None, tbl.h, ctypes.byref(ctypes.c_void_p())) == -22
    assert L.cndp_gpu_mq_create_udp_input(cl.h, ctypes.byref(c), tbl.h, None) == -22
    assert L.cndp_gpu_mq_create_udp_input(None, ctypes.byref(c), tbl.h, ctypes.byref(ctypes.c_void_p())) == -22
    for mode in (N.CNDP_MQ_IP4_LOOKUP, N.CNDP_MQ_CNET, N.CNDP_MQ_MAC_SWAP, N.CNDP_MQ_IP4_REWRITE, N.CNDP_MQ_CFWD_FWD,
                 N.CNDP_MQ_ACL_FWD, N.CNDP_MQ_IP4_FORWARD, 9):
        assert create(mode=mode) == -22
    for bit in range(8):
        assert create(flags=1 << bit) == -22
    assert create(batch=255) == -22 and create(batch=(1 << 24) + 1) == -22
    assert create(depth=1) == -22 and create(depth=17) == -22            # CNDP_MQ_DEPTH_MAX is 16
    assert create(stage_max=63) == -22 and create(stage_max=65536) == -22
    assert create(umem=pool.base) == -22                                        # not registered
    with Queue(cl, pool, std, True) as q:
        assert all(q.q.stat(k) == 0 for k in KEYS) and L.cndp_gpu_mq_stat(q.q.h, 17) == -22
        assert q.q.submit(None, 0) == 0
    other = MbufQueue(cl, N.CNDP_MQ_MAC_SWAP, batch=256, depth=2)      # the six keys are this mode's alone
    try:
        assert all(L.cndp_gpu_mq_stat(other.h, k) == -22 for k in KEYS) and other.stat(N.CNDP_MQ_STAT_FORWARD) == 0
    finally:
        other.close()


def test_table_bound_to_another_device(gpu):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU: a table bound to cuda:0 must refuse a queue on cuda:1")
    from cndp_amd.classify import Classifier
    w = M.standard_world()
    c0, c1 = Classifier(0), Classifier(1)
    try:
        pool = M.make_pool(4)
        for i in range(4):
            M.put(pool, i, dport=5000)
        with Queue(c0, pool, w, False) as q:       # its first batch binds the table to cuda:0
            q.check([[0, 1, 2, 3]], M.expect(pool, w, [[0, 1, 2, 3]], False))
        with pytest.raises(OSError) as e:
            MbufQueue(c1, N.CNDP_MQ_UDP_INPUT, batch=256, depth=2, pcb_tbl=w.tbl)
        assert e.value.errno == 22
    finally:
        c0.close()
        c1.close()
        w.close()

"""cnet's tcp_input node as a mode of the asynchronous mbuf queue
(cndp_gpu_mq_create_tcp_input, include/cndp_mqtcp.h), zero-copy and staged, over
pools of at most 1024 mbufs laid out like CNDP's.

Every expected value comes twice: from the Python restatement of the node over
mbufs (tests/mq_tcp_ref.py, independent of the library) and from the host twin
(cndp_tcp_input_node_host) run burst by burst over a copy of the pool.  The
edges, the segment records, the eight counters, the order of return and the
WHOLE pool memory -- mbuf headers, metadata and the frames, which the node never
writes -- are compared exactly.  Every test asserts that the outcomes it is
about occur in its input."""
import ctypes

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.mbuf import FRAME, MbufQueue

import mq_tcp_ref as M

pytestmark = pytest.mark.gpu

KEYS = tuple(range(N.CNDP_MQ_STAT_TCP_SEGMENT, N.CNDP_MQ_STAT_TCP_IPOPT + 1))
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
    """A tcp_input queue over `pool`, registered first when zero-copy."""

    def __init__(self, cl, pool, world, zero_copy, batch=256, depth=2, md_delta=None, md_null=None,
                 mode=N.CNDP_MQ_TCP_INPUT, **kw):
        self.cl, self.pool, self.zc = cl, pool, zero_copy
        self.seen = [0] * M.NSTAT
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
            self.q = MbufQueue(cl, mode, batch=batch, depth=depth, umem=pool.base if zero_copy else None,
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

    def poll(self, plain=False):
        """poll_tcp, or plain poll with no records (None)"""
        if plain:
            a, e = self.q.poll()
            return a, e, None
        return self.q.poll_tcp()

    def drive(self, bursts, outside=None, flush_each=False, interleave=False):
        """Submit bursts of mbuf indices (None: the mbuf at address `outside`) as
        cnet-graph's node would, polling between them, until all are back:
        (addresses, edges, records or None per poll) in completion order.
        interleave: every other poll is plain cndp_gpu_mq_poll."""
        q = self.q
        got_a, got_e, got_s = [], [], []
        turn = [0]

        def take():
            turn[0] += 1
            a, e, s = self.poll(plain=interleave and turn[0] % 2 == 0)
            got_a.append(a)
            got_e.append(e)
            got_s.append((len(a), s))
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
        return np.concatenate(got_a), np.concatenate(got_e), got_s

    def check(self, bursts, want, outside=None, flush_each=False, interleave=False):
        """One pass of `bursts` through the queue against `want` (M.expect)."""
        addrs, edges, segs = self.drive(bursts, outside, flush_each, interleave)
        sent = [outside if i is None else self.pool.addr(int(i)) for b in bursts for i in b]
        assert addrs.tolist() == sent, "mbufs came back out of submission order"
        bad = np.nonzero(edges != want["edges"])[0]
        assert len(bad) == 0, (f"edges: {len(bad)} differ, first at {bad[0]}: got {edges[bad[0]]:#x} "
                               f"want {want['edges'][bad[0]]:#x}")
        pos, n_rec = 0, 0
        for k, s in segs:                                    # the records of the polls that asked for them
            if s is not None:
                assert len(s) == k
                w = want["segs"][pos:pos + k]
                assert s.tobytes() == w.tobytes(), f"records differ in the poll that returned mbufs {pos} ..."
                n_rec += k
            pos += k
        assert 0 < n_rec < len(sent) if interleave else n_rec == len(sent)
        bad = np.nonzero(self.pool.mem != want["mem"])[0]
        assert len(bad) == 0, (f"pool memory: {len(bad)} bytes differ, first at mbuf {bad[0] // FRAME} + {bad[0] % FRAME}: "
                               f"got {self.pool.mem[bad[0]]:#x} want {want['mem'][bad[0]]:#x}")
        self.seen = [a + b for a, b in zip(self.seen, want["stats"])]
        assert [self.q.stat(k) for k in KEYS] == self.seen
        assert all(self.q.stat(k) == 0 for k in OTHER_KEYS)         # other modes' families
        return edges


def occurs(want, *keys):
    assert all(want["stats"][k] > 0 for k in keys), want["stats"]


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
    occurs(want, M.SEGMENT, M.NOMATCH, M.CKSUM, M.ADJUST, M.SHORT, M.BADOFF, M.OPT)
    assert sum(want["stats"]) == 1000
    with Queue(cl, pool, std, zero_copy, batch=batch, depth=depth) as q:
        q.check(bursts, want)
        assert q.q.stat(N.CNDP_MQ_STAT_MBUFS) == 1000 and q.q.stat(N.CNDP_MQ_STAT_BATCHES) >= 1000 // batch
    pool = M.make_pool(600)                                  # 600 mbufs as one burst
    M.fill_mix(pool, seed=6)
    want = M.expect(pool, std, [list(range(600))], zero_copy)
    occurs(want, M.SEGMENT, M.NOMATCH, M.CKSUM)
    with Queue(cl, pool, std, zero_copy, batch=batch, depth=depth) as q:
        q.check([list(range(600))], want)


@FORMS
@pytest.mark.parametrize("punt", [True, False])
def test_lookup_classes(cl, gpu, zero_copy, punt):
    """NCONN connections behind a wildcard and a bound listener, keys only a
    listener answers, a deleted entry, tuples that collide in the exact hash,
    no match with the punt flag on and off, user values."""
    w = M.standard_world()
    try:
        w.set_flags(punt, False)
        pool = M.make_pool(64)
        n = M.fill_lookup(pool)
        want = M.expect(pool, w, [list(range(n))], zero_copy)
        occurs(want, M.SEGMENT, M.NOMATCH)
        miss = M.TCP_PUNT if punt else M.TCP_DROP
        assert want["edges"][:11].tolist() == [M.TCP_SEG] * 8 + [miss, miss, M.TCP_SEG]
        with Queue(cl, pool, w, zero_copy) as q:
            q.check([list(range(n))], want)
        assert int(pool.hdr["udata64"][0]) == w.users[2] != 2 and int(pool.hdr["udata64"][8]) == 0xABABABABABABABAB
    finally:
        w.close()


@FORMS
def test_table_of_4096(cl, gpu, zero_copy):
    w = M.big_world()
    try:
        pool = M.make_pool(256)
        M.fill_big(pool)
        want = M.expect(pool, w, [list(range(256))], zero_copy)
        occurs(want, M.SEGMENT, M.NOMATCH)
        hdr = want["mem"].reshape(pool.n, FRAME)[:, :64].view(pool.hdr.dtype)[:, 0]
        users = set(int(x) for x in hdr["udata64"])
        assert 0x7F00DEAD0000 in users and 1 in users and len(users) > 200   # the last entry; a deleted one's listener
        with Queue(cl, pool, w, zero_copy) as q:
            q.check([list(range(256))], want)
    finally:
        w.close()


@FORMS
def test_checksum(cl, std, zero_copy):
    """Every length of M.SEG_LENS at odd, 4-byte-misaligned and aligned mtod, good
    sums and corrupted first / last bytes; a zero field that fails and one that is
    right; 0xFFFF for 0x0000; total_length below the IHL and beyond the readable
    bytes; one flipped bit in the last byte of 1460."""
    pool = M.make_pool(512)
    n, sp = M.fill_cksum(pool)
    bursts = M.split(list(range(n)), [256, n - 256])
    want = M.expect(pool, std, bursts, zero_copy)
    assert (want["edges"][:sp // 2] == M.TCP_SEG).all() and (want["edges"][sp // 2:sp] == (M.TCP_DROP | M.CK)).all()
    bad, ok = M.TCP_DROP | M.CK, M.TCP_SEG
    assert want["edges"][sp:sp + 12].tolist() == [bad, ok, ok, ok, bad, bad, bad, bad, bad, ok, bad, ok]
    occurs(want, M.CKSUM, M.SEGMENT)
    with Queue(cl, pool, std, zero_copy, batch=512) as q:
        q.check(bursts, want)


def test_checksum_stage_max(cl, std):
    """Staged, stage_max = 128: a 256-byte segment is clipped."""
    pool = M.make_pool(512)
    n, sp = M.fill_cksum(pool)
    idx = list(range(sp, n))
    want = M.expect(pool, std, [idx], False, stage_max=128)
    assert want["edges"][9] == M.TCP_DROP | M.CK and want["edges"][1] == M.TCP_SEG
    occurs(want, M.CKSUM, M.SEGMENT)
    with Queue(cl, pool, std, False, stage_max=128) as q:
        q.check([idx], want)


def test_checksum_region_end(cl, std):
    """Zero-copy: the pool's last mbuf with its segment ending exactly at the
    region's end, and reaching past it."""
    for over, ck in ((0, "good"), (0, "last"), (2, "good"), (40, "good")):
        pool = M.make_pool(4)
        for i in range(4):
            M.put(pool, i, seglen=100, cksum=ck)
        M.put(pool, 3, seglen=100, data_off=FRAME - 64 - 120 + over, cksum=ck)
        pool.hdr["buf_len"][3] = 4000
        want = M.expect(pool, std, [[0, 1], [2, 3]], True)
        assert want["edges"][3] == (M.TCP_SEG if over == 0 and ck == "good" else M.TCP_DROP | M.CK)
        occurs(want, M.SEGMENT if ck == "good" else M.CKSUM)
        with Queue(cl, pool, std, True) as q:
            q.check([[0, 1], [2, 3]], want)


@FORMS
def test_checksum_waves(cl, std, zero_copy):
    """Waves holding exactly 0, 1, 4, 5 and 64 lanes that hit: the lanes that
    missed join the cooperative sums."""
    pool = M.make_pool(320)
    n = M.fill_waves(pool)
    bursts = M.split(list(range(n)), [256, 64])
    want = M.expect(pool, std, bursts, zero_copy)
    assert want["stats"][M.CKSUM] == 25 and want["stats"][M.SEGMENT] == 49 and want["stats"][M.NOMATCH] == 246
    # one batch (it stays below half of 1024 until the flush): wave k holds mbufs 64 k ... 64 k + 63
    with Queue(cl, pool, std, zero_copy, batch=1024) as q:
        q.check(bursts, want)
        assert q.q.stat(N.CNDP_MQ_STAT_BATCHES) == 1


@FORMS
def test_header_steps(cl, std, zero_copy):
    """IPOPT, pktmbuf_adjust failing both ways, rx_short at 19 and not at 20,
    offset nibbles 4 and 15, offset above total_length and above data_len, len
    wrapping, SYN / FIN counts."""
    pool = M.make_pool(16)
    n = M.fill_steps(pool)
    want = M.expect(pool, std, [list(range(n))], zero_copy)
    S, D, O = M.TCP_SEG, M.TCP_DROP, M.TCP_SEG | M.IPOPT
    assert want["edges"].tolist() == [O, O, D, D, D, S, D, S, S, D, S, S, S, S]
    occurs(want, M.OPT, M.ADJUST, M.SHORT, M.BADOFF, M.SEGMENT)
    with Queue(cl, pool, std, zero_copy) as q:
        q.check([list(range(n))], want)
    assert (int(pool.hdr["data_off"][8]), int(pool.hdr["data_len"][8])) == (212, 40)
    assert (int(pool.hdr["data_off"][0]), int(pool.hdr["data_len"][0])) == (192, 64)


@FORMS
@pytest.mark.parametrize("hook", ["default", "offset", "null"])
def test_metadata_hooks(cl, std, zero_copy, hook):
    pool = M.make_pool(48)
    M.fill_mix(pool, seed=9)
    kw = {"default": {}, "offset": {"md_delta": 128}, "null": {"md_delta": 128, "md_null": lambda i: i % 3 == 0}}[hook]
    bursts = [list(range(20)), list(range(20, 48))]
    want = M.expect(pool, std, bursts, zero_copy, **kw)
    assert (want["stats"][M.NOMD] > 0) == (hook == "null")
    occurs(want, M.SEGMENT)
    with Queue(cl, pool, std, zero_copy, **kw) as q:
        q.check(bursts, want)


@FORMS
def test_table_changes_between_batches(cl, gpu, zero_copy):
    """A connection added, one deleted, a user value and the punt flag changed
    between two batches of one queue."""
    w = M.standard_world()
    try:
        pool = M.make_pool(64)
        idx = list(range(64))
        with Queue(cl, pool, w, zero_copy, depth=4) as q:
            def once():
                M.fill_mix(pool, seed=21)
                for i in range(0, 64, 8):
                    M.put(pool, i, src=M.PEER2, sport=41000, dst=M.OTHER)   # the wildcard listener until a connection is added
                    M.put(pool, i + 1, dport=7000)
                want = M.expect(pool, w, [idx[:40], idx[40:]], zero_copy)
                occurs(want, M.SEGMENT)
                return q.check([idx[:40], idx[40:]], want, flush_each=True)

            e = once()
            assert e[0] == M.TCP_SEG and e[1] == M.TCP_PUNT and int(pool.hdr["udata64"][0]) == 0
            new = w.add(laddr=M.OTHER, lport=5000, faddr=M.PEER2, fport=41000, user=0x5555000012345678)
            once()
            assert int(pool.hdr["udata64"][0]) == 0x5555000012345678
            w.user_set(new, 42)
            lis = w.add(lport=7000)
            e = once()
            assert int(pool.hdr["udata64"][8]) == 42 and e[1] == M.TCP_SEG
            w.delete(new)
            w.delete(lis)
            w.set_flags(False, False)
            e = once()
            assert e[0] == M.TCP_SEG and int(pool.hdr["udata64"][0]) == 0 and e[1] == M.TCP_DROP
    finally:
        w.close()


def test_one_table_two_readers(cl, gpu):
    """cndp_gpu_tcp_input on another stream against the same table while queue
    batches are in flight: the queue's results are right and the batch stage's
    are what it gives alone."""
    import torch
    from cndp_amd import pktgen
    import tcp_ref
    w = M.standard_world()
    try:
        n = 512
        pool = M.make_pool(n)
        M.fill_mix(pool, seed=31)
        rows = pool.mem.reshape(n, FRAME)
        slab = np.zeros((n, 512), np.uint8)
        for i in range(n):
            o = 64 + int(pool.hdr["data_off"][i])
            slab[i] = rows[i, o:o + 512]
        l3 = ((pool.hdr["tx_offload"] >> 7) & 0x1FF).astype(np.uint32)
        rxmeta = (l3 << 7 | 20 << 16).astype(np.uint32)
        slab_t = torch.from_numpy(slab.reshape(-1).copy()).to(gpu)
        out = {"rxmeta": torch.from_numpy(rxmeta.view(np.int32).copy()).to(gpu)}
        sel = torch.ones(n, dtype=torch.uint8, device=gpu)
        want_b = tcp_ref.tcp_input_ref(slab.reshape(-1), n, rxmeta, w.ent, sel=np.ones(n, np.uint8), stride=512, punt=True)
        bursts = M.split(list(range(n)), [256, 256])
        want = M.expect(pool, w, bursts, True)
        occurs(want, M.SEGMENT, M.NOMATCH, M.CKSUM)
        side = torch.cuda.Stream(device=gpu)
        with Queue(cl, pool, w, True, depth=4) as q:
            ptrs = pool.ptrs(np.arange(n))
            assert q.q.submit(ptrs, 256) == 256                       # a batch of its own, launched at once
            with torch.cuda.stream(side):
                r1 = cl.tcp_input(pktgen.Frames(slab_t, n, stride=512), out, w.tbl, sel=sel, stream=side.cuda_stream)
            assert q.q.submit(ctypes.addressof(ptrs) + 256 * 8, 256) == 256
            with torch.cuda.stream(side):
                r2 = cl.tcp_input(pktgen.Frames(slab_t, n, stride=512), out, w.tbl, sel=sel, stream=side.cuda_stream)
            got_a, got_e = [], []
            while q.q.pending:
                q.q.wait()
                a, e, _ = q.q.poll_tcp()
                got_a.append(a)
                got_e.append(e)
            side.synchronize()
            assert np.concatenate(got_a).tolist() == [pool.addr(i) for i in range(n)]
            assert np.array_equal(np.concatenate(got_e), want["edges"]) and np.array_equal(pool.mem, want["mem"])
            assert [q.q.stat(k) for k in KEYS] == want["stats"]
        for r in (r1, r2):
            assert np.array_equal(r["l4edge"].cpu().numpy(), want_b["l4edge"])
            assert np.array_equal(r["pcb"].cpu().numpy().view(np.uint32), want_b["pcb"])
    finally:
        w.close()


def test_zero_copy_out_of_region(cl, std):
    """mbufs outside every registered region: CNDP_MQ_EDGE_NONE, untouched, counted
    nowhere, a zero record; a frame outside (buf_addr elsewhere) likewise."""
    pool = M.make_pool(8)
    other = M.make_pool(2, seed=3)
    for i in range(8):
        M.put(pool, i, sport=40000 + i)
    M.put(other, 0)
    keep = other.mem.copy()
    bursts = [[0, None, 2, 3], [None, 5, 6, 7]]
    want = M.expect(pool, std, bursts, True)
    occurs(want, M.SEGMENT)
    with Queue(cl, pool, std, True) as q:
        e = q.check(bursts, want, outside=other.addr(0))
        assert e[1] == N.CNDP_MQ_EDGE_NONE and e[4] == N.CNDP_MQ_EDGE_NONE and np.array_equal(other.mem, keep)
        assert sum(q.q.stat(k) for k in KEYS) == 6
        for i in range(8):
            M.put(pool, i)
        pool.hdr["buf_addr"][5] = other.addr(0) + 64          # an mbuf of the pool whose buffer lies outside it
        before = pool.mem.copy()
        addrs, e, segs = q.drive([list(range(8))])
        s = np.concatenate([x for _, x in segs])
        assert e[5] == N.CNDP_MQ_EDGE_NONE and (np.delete(e, 5) == M.TCP_SEG).all()
        assert not s[5].tobytes().strip(b"\0") and (np.delete(s["offset"], 5) == 20).all()
        assert np.array_equal(pool.mem[5 * FRAME:6 * FRAME], before[5 * FRAME:6 * FRAME]) and np.array_equal(other.mem, keep)
        assert sum(q.q.stat(k) for k in KEYS) == 6 + 7


@FORMS
def test_poll_and_poll_tcp_interleaved(cl, std, zero_copy):
    """Plain poll works on this mode and drops the records; poll_tcp's records
    stay those of the mbufs it returns."""
    pool = M.make_pool(600)
    M.fill_mix(pool, seed=41)
    bursts = M.split(list(range(600)), [100] * 6)
    want = M.expect(pool, std, bursts, zero_copy)
    occurs(want, M.SEGMENT, M.CKSUM, M.NOMATCH)
    with Queue(cl, pool, std, zero_copy, batch=256, depth=4) as q:
        q.check(bursts, want, interleave=True)
        # a partial poll_tcp: max below what is ready
        for i in range(8):
            M.put(pool, i, sport=40000 + i, flags=0x02)
        want = M.expect(pool, std, [list(range(8))], zero_copy)
        q.q.submit(pool.ptrs(np.arange(8)), 8)
        q.q.flush()
        q.q.wait()
        a1, e1, s1 = q.q.poll_tcp(3)
        a2, e2 = q.q.poll(2)
        a3, e3, s3 = q.q.poll_tcp(16)
        assert (len(a1), len(a2), len(a3)) == (3, 2, 3)
        assert s1.tobytes() == want["segs"][:3].tobytes() and s3.tobytes() == want["segs"][5:].tobytes()
        assert (s3["len"] == 13).all() and np.array_equal(pool.mem, want["mem"])
        # segs may be NULL
        out, ed = (ctypes.c_void_p * 4)(), np.zeros(4, np.uint16)
        assert N.lib().cndp_gpu_mq_poll_tcp(q.q.h, out, ed.ctypes.data, None, 4) == 0


def test_chain_behind_udp_input(cl, gpu):
    """One pool through a CNDP_MQ_UDP_INPUT queue; the mbufs that come back on
    ip4_proto's tcp_input edge go through the TCP queue.  The final pool equals
    the two twins run in the same order."""
    import mq_udp_ref as U
    uw, tw = U.standard_world(), M.standard_world()
    try:
        uw.set_flags(True, True)
        n = 512
        pool = M.make_pool(n)
        M.fill_mix(pool, seed=51)
        for i in range(0, n, 3):                               # a third of it UDP traffic
            U.put(pool, i, dport=[5000, 5002, 4999][(i // 3) % 3], dgram=26 + i % 200,
                  cksum=["good", "last"][(i // 3) % 2], data_off=192 + i % 16)
        bursts = M.split(list(range(n)), [256, 256])
        want_u = U.expect(pool, uw, bursts, False)
        assert want_u["stats"][U.TCP] > 0 and want_u["stats"][U.RECV] > 0
        on = [i for i in range(n) if want_u["edges"][i] == U.PROTO_TCP]
        tb = [on[:200], on[200:]]
        mid = type("P", (), {})()                              # the pool as the UDP stage leaves it
        mid.mem, mid.base, mid.n = want_u["mem"], pool.base, pool.n
        want_t = M.expect(mid, tw, tb, False)
        occurs(want_t, M.SEGMENT, M.NOMATCH, M.CKSUM, M.OPT)
        uq = MbufQueue(cl, N.CNDP_MQ_UDP_INPUT, batch=256, depth=2, pcb_tbl=uw.tbl, max_delay_us=1000000)
        try:
            addrs, edges = uq.run(pool, np.arange(n), [256, 256])
        finally:
            uq.close()
        assert np.array_equal(edges, want_u["edges"]) and np.array_equal(pool.mem, want_u["mem"])
        got = pool.index_of(addrs[edges == U.PROTO_TCP]).tolist()
        assert got == on
        with Queue(cl, pool, tw, False) as q:
            q.check(tb, want_t)
        assert np.array_equal(pool.mem, want_t["mem"])
    finally:
        uw.close()
        tw.close()


def test_arguments(cl, std):
    L = N.lib()
    pool = M.make_pool(4)
    tbl = std.tbl

    def create(mode=N.CNDP_MQ_TCP_INPUT, flags=0, batch=256, depth=2, stage_max=0, umem=None, t=tbl.h, fn=None):
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
        elif fn == "udp_input":
            r = L.cndp_gpu_mq_create_udp_input(cl.h, ctypes.byref(c), t, ctypes.byref(h))
        else:
            r = L.cndp_gpu_mq_create_tcp_input(cl.h, ctypes.byref(c), t, ctypes.byref(h))
        if r == 0:
            L.cndp_gpu_mq_free(h)
        return r

    assert create() == 0
    for fn in ("plain", "fwd", "ip4_forward", "udp_input"):    # mode 9 needs its own call
        assert create(fn=fn) == -22, fn
    assert create(t=None) == -22
    c = N.MqConf()
    c.mode = N.CNDP_MQ_TCP_INPUT
    assert L.cndp_gpu_mq_create_tcp_input(cl.h, None, tbl.h, ctypes.byref(ctypes.c_void_p())) == -22
    assert L.cndp_gpu_mq_create_tcp_input(cl.h, ctypes.byref(c), tbl.h, None) == -22
    assert L.cndp_gpu_mq_create_tcp_input(None, ctypes.byref(c), tbl.h, ctypes.byref(ctypes.c_void_p())) == -22
    for mode in (N.CNDP_MQ_IP4_LOOKUP, N.CNDP_MQ_CNET, N.CNDP_MQ_MAC_SWAP, N.CNDP_MQ_IP4_REWRITE, N.CNDP_MQ_CFWD_FWD,
                 N.CNDP_MQ_CFWD_L3FWD, N.CNDP_MQ_ACL_FWD, N.CNDP_MQ_IP4_FORWARD, N.CNDP_MQ_UDP_INPUT, 10):
        assert create(mode=mode) == -22
    for bit in range(32):
        assert create(flags=1 << bit) == -22
    assert create(batch=255) == -22 and create(batch=(1 << 24) + 1) == -22
    assert create(depth=1) == -22 and create(depth=17) == -22            # CNDP_MQ_DEPTH_MAX is 16
    assert create(stage_max=63) == -22 and create(stage_max=65536) == -22
    assert create(umem=pool.base) == -22                                        # not registered
    with Queue(cl, pool, std, True) as q:
        assert all(q.q.stat(k) == 0 for k in KEYS) and L.cndp_gpu_mq_stat(q.q.h, 25) == -22
        assert all(L.cndp_gpu_mq_stat(q.q.h, k) == -22 for k in range(11, 17))    # the UDP mode's keys
        assert q.q.submit(None, 0) == 0
    out, ed, sg = (ctypes.c_void_p * 4)(), np.zeros(4, np.uint16), np.zeros(4, M.SEG_DT)
    other = MbufQueue(cl, N.CNDP_MQ_MAC_SWAP, batch=256, depth=2)      # the eight keys are this mode's alone
    try:
        assert all(L.cndp_gpu_mq_stat(other.h, k) == -22 for k in KEYS) and other.stat(N.CNDP_MQ_STAT_FORWARD) == 0
        assert L.cndp_gpu_mq_poll_tcp(other.h, out, ed.ctypes.data, sg.ctypes.data, 4) == -22
    finally:
        other.close()
    import mq_udp_ref as U
    uw = U.standard_world()
    try:
        uq = MbufQueue(cl, N.CNDP_MQ_UDP_INPUT, batch=256, depth=2, pcb_tbl=uw.tbl)
        try:
            assert L.cndp_gpu_mq_poll_tcp(uq.h, out, ed.ctypes.data, sg.ctypes.data, 4) == -22
            assert all(L.cndp_gpu_mq_stat(uq.h, k) == -22 for k in KEYS)
        finally:
            uq.close()
    finally:
        uw.close()


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
            M.put(pool, i)
        with Queue(c0, pool, w, False) as q:       # its first batch binds the table to cuda:0
            q.check([[0, 1, 2, 3]], M.expect(pool, w, [[0, 1, 2, 3]], False))
        with pytest.raises(OSError) as e:
            MbufQueue(c1, N.CNDP_MQ_TCP_INPUT, batch=256, depth=2, pcb_tbl=w.tbl)
        assert e.value.errno == 22
    finally:
        c0.close()
        c1.close()
        w.close()

"""cndp_gpu_mq_poll with a small max: a finished slot handed back in ranges.

mq_writeback works on a range [i0, i1) of a slot, but the other queue tests
always poll whole slots (MbufQueue.poll asks for 65536).  Here every mode of
the queue, in each of its forms (zero-copy, staged, host writeback, device
headers), gets the same input twice: through a queue polled with max 7 until it
is empty, and through a queue polled in one call.  Everything observable must
be equal.  Pools and frames are those of each mode's own test."""
import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd import pktgen
from cndp_amd.mbuf import HDR, MbufPool, MbufQueue

import test_gpu_mq as Q

pytestmark = pytest.mark.gpu

l3, cn = Q.l3, Q.cn     # the module fixtures of test_gpu_mq.py: a Classifier with the l3fwd FIB / cnet's two


PIECE_BURSTS = (69, 5)      # 69 = 64 + 5: two chunks of ip4_forward; 5: a 4-wide group and a 1-wide tail
PIECE_N = sum(PIECE_BURSTS)
PIECE_BATCH = pytest.mark.parametrize("batch", [256, 512], ids=["batch256", "batch512"])


def _poll_in_pieces(cl, zero_copy, build, open_queue, before=None):
    """The same input through two queues: one polled with max 7 until empty, one
    polled in one call.  build() makes a pool of PIECE_N mbufs, open_queue(pool,
    umem) its queue; both runs submit bursts of 69 and 5 and flush.  The order of
    return, the edges, the whole pool memory (every mbuf header byte -- buf_addr
    relative to the pool --, the frames, the metadata at m + 64) and the answer
    of cndp_gpu_mq_stat to every key from 0 to 19 must be equal.  batch 256: each
    burst is a batch of its own (a poll crosses from one slot to the next);
    batch 512: both share one slot."""
    runs = []
    for piece in (7, 1 << 16):
        pool = build()
        assert pool.n == PIECE_N
        if before:
            before()
        if zero_copy:
            cl.host_register(pool.mem)
        try:
            q = open_queue(pool, pool.base if zero_copy else None)
            try:
                pos = 0
                for b in PIECE_BURSTS:
                    assert q.submit(pool.ptrs(np.arange(pos, pos + b))) == b
                    pos += b
                q.flush()
                q.wait()
                got_a, got_e, calls = [], [], 0
                while q.pending:
                    a, e = q.poll(piece)
                    assert a.size <= piece
                    if a.size == 0:
                        q.wait()    # the second batch is still in flight
                        continue
                    got_a.append(a)
                    got_e.append(e)
                    calls += 1
                assert calls >= (PIECE_N + piece - 1) // piece
                stats = [int(q._L.cndp_gpu_mq_stat(q.h, k)) for k in range(20)]
            finally:
                q.close()
        finally:
            if zero_copy:
                cl.host_unregister(pool.mem)
        mem = pool.mem.copy()
        mem.reshape(pool.n, -1)[:, :HDR].view(pool.hdr.dtype)[:, 0]["buf_addr"] -= np.uint64(pool.base)
        runs.append((pool.index_of(np.concatenate(got_a)), np.concatenate(got_e), mem, stats))
    (ia, ea, ma, sa), (ib, eb, mb, sb) = runs
    assert np.array_equal(ia, np.arange(PIECE_N)) and np.array_equal(ib, ia), "order of return"
    assert np.array_equal(ea, eb), f"edges differ at {np.nonzero(ea != eb)[0][:8]}"
    bad = np.nonzero(ma != mb)[0]
    assert bad.size == 0, f"pool memory: {bad.size} bytes differ, first at mbuf {bad[0] // 2048} + {bad[0] % 2048}"
    assert sa == sb, f"cndp_gpu_mq_stat: {sa} != {sb}"
    assert sa[N.CNDP_MQ_STAT_MBUFS] == PIECE_N
    return eb, sb


WB, DH, RXP, RWF = (N.CNDP_MQ_F_HOST_WRITEBACK, N.CNDP_MQ_F_DEVICE_HEADERS, N.CNDP_MQ_F_RX_PARSE, N.CNDP_MQ_F_REWRITE)


@PIECE_BATCH
@pytest.mark.parametrize("zero_copy,flags", [(True, 0), (False, 0), (True, WB), (True, DH), (True, DH | WB), (False, RXP),
                                             (True, RXP | WB), (True, RXP | RWF), (True, RWF | WB)],
                         ids=["zero_copy", "staged", "host_writeback", "device_headers", "device_headers_host_writeback",
                              "staged_rx_parse", "rx_parse_host_writeback", "fused", "fused_host_writeback"])
def test_mq_poll_in_pieces_ip4_lookup(l3, gpu, zero_copy, flags, batch):
    cl, fib, t4 = l3
    Q._rewrite_setup(cl, 41)
    fr = Q._mixed_l3_frames(PIECE_N, seed=61)

    def build():
        pool = MbufPool(PIECE_N)
        pool.hdr["data_off"] = 256 + np.arange(PIECE_N) % 61
        pool.fill(fr)
        pool.hdr["udata64"] = 0xABABABABABABABAB
        pool.hdr["packet_type"] = 0x77
        return pool

    edges, _ = _poll_in_pieces(cl, zero_copy, build, lambda pool, umem: MbufQueue(
        cl, N.CNDP_MQ_IP4_LOOKUP, flags=flags, batch=batch, depth=2, umem=umem, max_delay_us=1000000))
    assert len(set(edges.tolist())) > 1


@PIECE_BATCH
@pytest.mark.parametrize("zero_copy,flags", [(True, 0), (False, 0), (True, WB), (True, DH), (True, N.CNDP_MQ_F_HASH),
                                             (False, N.CNDP_MQ_F_NO_METADATA)],
                         ids=["zero_copy", "staged", "host_writeback", "device_headers", "zero_copy_hash",
                              "staged_no_metadata"])
def test_mq_poll_in_pieces_cnet(cn, gpu, zero_copy, flags, batch):
    """The pool is built as for zero-copy in both forms: a frame that reaches past
    its buffer finds the same staged bytes there in both runs."""
    cl, routes, v6, t4, t6 = cn

    edges, _ = _poll_in_pieces(cl, zero_copy, lambda: Q.cnet_pool(PIECE_N, routes, v6, True, shift=True)[0],
                               lambda pool, umem: MbufQueue(cl, N.CNDP_MQ_CNET, flags=flags, batch=batch, depth=2,
                                                            umem=umem, lport=7, max_delay_us=1000000),
                               before=lambda: cl.set_tuning(cnet_spec=256))     # fresh ptype node state
    assert {0, 1, 2} <= set((edges >> 8).tolist())


@PIECE_BATCH
@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "staged"])
def test_mq_poll_in_pieces_mac_swap(l3, gpu, zero_copy, batch):
    cl, fib, t4 = l3
    fr = pktgen.cndpfwd_udp(PIECE_N)

    def build():
        pool = MbufPool(PIECE_N)
        pool.fill(fr)
        return pool

    _poll_in_pieces(cl, zero_copy, build, lambda pool, umem: MbufQueue(cl, N.CNDP_MQ_MAC_SWAP, batch=batch, depth=2,
                                                                        umem=umem, max_delay_us=1000000))


@PIECE_BATCH
@pytest.mark.parametrize("zero_copy,flags", [(True, 0), (False, 0), (True, DH)], ids=["zero_copy", "staged", "device_headers"])
def test_mq_poll_in_pieces_ip4_rewrite(l3, gpu, zero_copy, flags, batch):
    cl, fib, t4 = l3
    Q._rewrite_setup(cl, 3)
    fr = Q._mixed_l3_frames(PIECE_N, seed=62)
    rng = np.random.default_rng(63)
    ck = rng.integers(0, 1 << 16, PIECE_N, dtype=np.uint64)
    ck[::7] = 0xFFFF
    ck[3::7] = 0xFFFE
    priv = rng.integers(0, 70, PIECE_N, dtype=np.uint64) | (rng.integers(0, 256, PIECE_N, dtype=np.uint64) << 16) | (ck << 32)

    def build():
        pool = MbufPool(PIECE_N)
        pool.hdr["data_off"] = 256 + np.arange(PIECE_N) % 61
        pool.fill(fr)
        pool.hdr["udata64"] = priv
        return pool

    edges, _ = _poll_in_pieces(cl, zero_copy, build, lambda pool, umem: MbufQueue(
        cl, N.CNDP_MQ_IP4_REWRITE, flags=flags, batch=batch, depth=2, umem=umem, max_delay_us=1000000))
    assert len(set(edges.tolist())) > 2


@PIECE_BATCH
@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "staged"])
@pytest.mark.parametrize("kind", ["fwd", "l3fwd", "acl"])
def test_mq_poll_in_pieces_cndpfwd(l3, gpu, kind, zero_copy, batch):
    import test_mq_cndpfwd_gpu as F
    cl = l3[0]
    n, lports = PIECE_N, (1, 2, 3, 70)
    fib = acl = None
    if kind == "fwd":
        rows = F.C.frames(np.arange(n, dtype=np.uint32), dmac5=np.array([1, 70, 200, 9, 3, 255, 64, 0])[np.arange(n) % 8], seed=5)
        build, mode, keys = (lambda: F.make_pool(n, rows)), N.CNDP_MQ_CFWD_FWD, F.FWD_KEYS
    elif kind == "l3fwd":
        fib, _ = F.l3_tables(name=f"mq-pieces-{int(zero_copy)}-{batch}")
        build, mode, keys = (lambda: F.make_pool(n, F.l3_rows(n))), N.CNDP_MQ_CFWD_L3FWD, F.FWD_KEYS
    else:
        acl = F.acl_table(F.SMALL)
        build, mode, keys = (lambda: F.acl_small_pool(n)[0]), N.CNDP_MQ_ACL_FWD, F.ACL_KEYS
    try:
        edges, st = _poll_in_pieces(cl, zero_copy, build, lambda pool, umem: MbufQueue(
            cl, mode, batch=batch, depth=2, umem=umem, lport=3, lports=lports, fib=fib, acl=acl,
            acl_mode=N.CNDP_ACL_STRICT, acl_flags=N.CNDP_ACL_F_MAC_SWAP, max_delay_us=1000000))
    finally:
        for t in (fib, acl):
            if t is not None:
                t.close()
    assert sum(st[k] for k in keys) == n and all(st[k] > 0 for k in keys[:2])


@PIECE_BATCH
@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "staged"])
def test_mq_poll_in_pieces_ip4_forward(l3, gpu, zero_copy, batch):
    import fwd_ref as R
    import mq_ip4fwd_ref as M
    cl = l3[0]
    arp, rt4, tbl = R.make_tables(R.standard_world())

    def build():
        pool = M.make_pool(PIECE_N)
        M.fill_random(pool, 3, data_offs=(214, 215, 216, 217))
        return pool

    try:
        _, st = _poll_in_pieces(cl, zero_copy, build, lambda pool, umem: MbufQueue(
            cl, N.CNDP_MQ_IP4_FORWARD, batch=batch, depth=2, umem=umem, fwd_tbl=tbl, max_delay_us=1000000))
    finally:
        R.close_tables(arp, rt4, tbl)
    keys = (N.CNDP_MQ_STAT_FWD_DIRECT, N.CNDP_MQ_STAT_FWD_GATEWAY, N.CNDP_MQ_STAT_FWD_ARP_REQUEST)
    assert sum(st[k] for k in keys) == PIECE_N and all(st[k] > 0 for k in keys)


@PIECE_BATCH
@pytest.mark.parametrize("zero_copy,md_null", [(True, False), (False, False), (True, True), (False, True)],
                         ids=["zero_copy", "staged", "zero_copy_null_metadata", "staged_null_metadata"])
def test_mq_poll_in_pieces_udp_input(l3, gpu, zero_copy, md_null, batch):
    """null_metadata: a hook that answers NULL for every 7th mbuf (the outcome
    poll decides and counts as CNDP_MQ_STAT_L4_NOMD)."""
    import mq_udp_ref as M
    cl = l3[0]
    w = M.standard_world()

    def build():
        pool = M.make_pool(PIECE_N)
        M.fill_mix(pool)
        return pool

    def open_queue(pool, umem):
        hook = (lambda m: None if ((m - pool.base) // 2048) % 7 == 2 else m + 64) if md_null else None
        return MbufQueue(cl, N.CNDP_MQ_UDP_INPUT, batch=batch, depth=2, umem=umem, pcb_tbl=w.tbl, metadata=hook,
                         max_delay_us=1000000)

    try:
        _, st = _poll_in_pieces(cl, zero_copy, build, open_queue)
    finally:
        w.close()
    keys = range(N.CNDP_MQ_STAT_L4_RECV, N.CNDP_MQ_STAT_L4_NOMD + 1)
    assert sum(st[k] for k in keys) == PIECE_N and (st[N.CNDP_MQ_STAT_L4_NOMD] > 0) == md_null

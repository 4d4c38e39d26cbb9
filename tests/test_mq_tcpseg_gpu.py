"""cnet's tcp_input, tcp_do_options and the header-prediction triage as one mode
of the asynchronous mbuf queue (cndp_gpu_mq_create_tcp_segment,
include/cndp_mqtcb.h), zero-copy and staged, over pools of at most 1500 mbufs
laid out like CNDP's.

Every expected value comes from the Python reference (tests/mq_tcpseg_ref.py:
tests/mq_tcp_ref.py's node and tests/tcpseg_ref.py's segment rule, composed,
independent of the library), and for batches of at most 256 mbufs also from the
host twin (cndp_tcp_segment_node_host) run over a copy of the pool.  The tests
decide the batch boundaries -- a batch is filled exactly or flushed before the
first poll -- and hand the composition to the reference, which computes FIRST
over it.  Edges, segment records, opts, verdicts, both counter families, the
order of return and the WHOLE pool memory are compared exactly."""
import ctypes

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.mbuf import FRAME, MbufQueue

import mq_tcp_ref as M
import mq_tcpseg_ref as T
import tcp_golden as TG
import tcpseg_ref as S

pytestmark = pytest.mark.gpu

KEYS = tuple(range(N.CNDP_MQ_STAT_TCP_SEGMENT, N.CNDP_MQ_STAT_TCP_IPOPT + 1))
TKEYS = tuple(range(N.CNDP_MQ_STAT_TSEG_RESET, N.CNDP_MQ_STAT_TSEG_PRED_NONE + 1))
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "staged"])


@pytest.fixture(scope="module")
def cl(gpu):
    from cndp_amd.classify import Classifier
    c = Classifier(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def std(gpu):
    tw = T.standard_tworld()
    yield tw
    tw.close()


class Queue:
    """A tcp_segment queue over `pool`, registered first when zero-copy."""

    def __init__(self, cl, pool, tw, zero_copy, batch=256, depth=2, md_delta=None, md_null=None, **kw):
        self.cl, self.pool, self.zc, self.batch = cl, pool, zero_copy, batch
        self.seen, self.tseen = [0] * M.NSTAT, [0] * T.NVERD
        self.got = [[], [], [], [], []]                        # addresses, edges, segs, opts, verdicts per poll
        self.turn = 0
        hook = None
        if md_delta is not None or md_null is not None:
            def hook(m):
                if md_null is not None and md_null((m - pool.base) // FRAME):
                    return None
                return m + (64 if md_delta is None else md_delta)
        if zero_copy:
            cl.host_register(pool.mem)
        try:
            # a long max_delay_us: a batch goes out full or flushed, or half full at a poll with the GPU idle --
            # and run() does not poll inside a batch
            self.q = MbufQueue(cl, N.CNDP_MQ_TCP_SEGMENT, batch=batch, depth=depth, umem=pool.base if zero_copy else None,
                               pcb_tbl=tw.tbl, tcb=tw.tcb_tbl, max_delay_us=1000000, metadata=hook, **kw)
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

    def take(self, variants=False):
        """One poll; with variants every second one is cndp_gpu_mq_poll_tcp and every third plain poll."""
        self.turn += 1
        kind = self.turn % 3 if variants else 0
        if kind == 1:
            a, e, s = self.q.poll_tcp()
            o = v = None
        elif kind == 2:
            a, e = self.q.poll()
            s = o = v = None
        else:
            a, e, s, o, v = self.q.poll_tcpseg()
        for g, x in zip(self.got, (a, e, s, o, v)):
            g.append(x)
        return len(a)

    def launch(self, b, pattern=(256,), outside=None, variants=False):
        """Submit the mbufs of one batch as bursts of the pattern's sizes without
        polling between them, then flush: `b` is what CNDP_MQ_STAT_BATCHES counts once."""
        assert 0 < len(b) <= self.batch
        q = self.q
        before = q.stat(N.CNDP_MQ_STAT_BATCHES)
        ptrs = (ctypes.c_void_p * len(b))(*[outside if i is None else self.pool.addr(int(i)) for i in b])
        done, k = 0, 0
        while done < len(b):
            size = min(pattern[k % len(pattern)], len(b) - done)
            got = q.submit(ctypes.addressof(ptrs) + done * ctypes.sizeof(ctypes.c_void_p), size)
            if got == 0:                                         # every slot is busy: only before the batch's first burst
                assert done == 0
                q.wait()
                self.take(variants)
                continue
            assert got == size
            done += size
            k += 1
        q.flush()
        assert q.stat(N.CNDP_MQ_STAT_BATCHES) == before + 1

    def drain(self, variants=False):
        for _ in range(64):
            if not self.q.pending:
                break
            self.q.wait()
            self.take(variants)
        assert self.q.pending == 0

    def check(self, batches, want, outside=None, variants=False):
        """What came back since the last check against `want` (T.expect over the same batches)."""
        got, self.got = self.got, [[], [], [], [], []]
        addrs, edges = np.concatenate(got[0]), np.concatenate(got[1])
        sent = [outside if i is None else self.pool.addr(int(i)) for b in batches for i in b]
        assert addrs.tolist() == sent, "mbufs came back out of submission order"
        bad = np.nonzero(edges != want["edges"])[0]
        assert len(bad) == 0, f"edges: {len(bad)} differ, first at {bad[0]}: got {edges[bad[0]]:#x} want {want['edges'][bad[0]]:#x}"
        pos, n_full = 0, 0
        for a, s, o, v in zip(got[0], got[2], got[3], got[4]):
            k = len(a)
            if s is not None:
                assert s.tobytes() == want["segs"][pos:pos + k].tobytes(), f"records differ in the poll of mbufs {pos} ..."
            if v is not None:
                bad = np.nonzero(v != want["verdicts"][pos:pos + k])[0]
                assert len(bad) == 0, (f"verdicts: {len(bad)} differ, first at mbuf {pos + bad[0]}: got {v[bad[0]]:#x} "
                                       f"want {want['verdicts'][pos + bad[0]]:#x}")
                assert o.tobytes() == want["opts"][pos:pos + k].tobytes(), f"opts differ in the poll of mbufs {pos} ..."
                n_full += k
            pos += k
        assert 0 < n_full < len(sent) if variants else n_full == len(sent)
        bad = np.nonzero(self.pool.mem != want["mem"])[0]
        assert len(bad) == 0, (f"pool memory: {len(bad)} bytes differ, first at mbuf {bad[0] // FRAME} + {bad[0] % FRAME}: "
                               f"got {self.pool.mem[bad[0]]:#x} want {want['mem'][bad[0]]:#x}")
        self.seen = [a + b for a, b in zip(self.seen, want["stats"])]
        self.tseen = [a + b for a, b in zip(self.tseen, want["tstats"])]
        assert [self.q.stat(k) for k in KEYS] == self.seen
        assert [self.q.stat(k) for k in TKEYS] == self.tseen
        L = N.lib()
        assert all(L.cndp_gpu_mq_stat(self.q.h, k) == -22 for k in range(25, 32))     # the transmit mode's keys
        assert all(L.cndp_gpu_mq_stat(self.q.h, k) == -22 for k in range(11, 17))     # the UDP mode's
        return edges

    def run(self, batches, want, pattern=(256,), outside=None, variants=False):
        for b in batches:
            self.launch(b, pattern, outside, variants)
        self.drain(variants)
        return self.check(batches, want, outside, variants)


def firsts(want):
    return np.nonzero(want["verdicts"] & S.FIRST)[0].tolist()


# (mbufs, burst sizes) per batch.  A batch is launched once no further full burst fits, so with
# batch 256 every burst is a batch of its own, and with 512 a batch may collect bursts up to 256 mbufs
# before its last one.
SHAPES = {256: [(1, (1,)), (63, (63,)), (64, (64,)), (65, (65,)), (256, (256,)), (256, (256,)), (256, (256,)), (39, (39,))],
          512: [(1, (1,)), (63, (63,)), (64, (64,)), (65, (65,)), (256, (256,)), (449, (1, 63, 64, 65, 256)),
                (102, (40, 62))]}


@FORMS
@pytest.mark.parametrize("batch,depth", [(256, 2), (512, 4)])
def test_batch_shapes(cl, std, zero_copy, batch, depth):
    """A mixed fill in batches of 1, 63, 64, 65 and 256 mbufs and in batches made
    of such bursts: one block and several (MQ_TPB is 64), waves with a tail, more
    batches than the depth.  Everything equals the reference."""
    pool = M.make_pool(1000)
    T.fill_mix(pool, std)
    shapes = SHAPES[batch]
    batches = M.split(list(range(1000)), [k for k, _ in shapes])
    assert sum(len(b) for b in batches) == 1000 and len(batches) == len(shapes)
    want = T.expect(pool, std, batches, zero_copy, now=T.NOW)
    st = want["stats"]
    assert all(st[k] > 0 for k in (M.SEGMENT, M.NOMATCH, M.CKSUM, M.ADJUST, M.SHORT, M.BADOFF, M.OPT))
    assert all(x > 0 for x in want["tstats"])
    with Queue(cl, pool, std, zero_copy, batch=batch, depth=depth) as q:
        q.q.set_now(T.NOW)
        for b, (_, pattern) in zip(batches, shapes):
            q.launch(b, pattern)
        q.drain()
        q.check(batches, want)
        assert q.q.stat(N.CNDP_MQ_STAT_MBUFS) == 1000 and q.q.stat(N.CNDP_MQ_STAT_BATCHES) == len(batches)


CAUSES = ["cksum", "nomd", "adjust", "short", "badoff", "outside"]


@pytest.mark.parametrize("zero_copy,cause", [(zc, c) for zc in (True, False) for c in CAUSES if zc or c != "outside"],
                         ids=lambda x: x if isinstance(x, str) else ("zero_copy" if x else "staged"))
def test_first_across_waves_and_blocks(cl, std, zero_copy, cause):
    """One PCB's segments at batch indices 0, 63, 64, 255, 256 and 511 of a
    512-batch, the earliest two dropped for `cause` ("outside": outside every
    registered region, which exists for zero-copy queues only -- the fill refuses
    the address on the host): FIRST sits on the first survivor, in another wave
    of another block; a second batch gets its own."""
    pool = M.make_pool(1024)
    other = M.make_pool(2, seed=3)
    t = std.tcbs[2]
    mine = dict(pair=T.pair_of(std.w, 2), seq=t["rcv_nxt"], ack=600, wnd=t["snd_wnd"] >> t["snd_scale"], flags=S.ACK)
    where = (0, 63, 64, 255, 256, 511)
    for i in range(1024):
        if i % 512 in where:
            T.put_spec(pool, i, mine, data_off=192 + i % 16)
        else:                                                     # other connections, each once a batch at most
            c = 4 + 2 * ((i % 512) % 30)
            T.put_spec(pool, i, dict(mine, pair=T.pair_of(std.w, c), seq=std.tcbs[c]["rcv_nxt"]), data_off=192 + i % 16)
    batches = [list(range(512)), list(range(512, 1024))]
    null = None
    for i in (0, 63):
        if cause == "cksum":
            T.put_spec(pool, i, dict(mine, bad_cksum=True))
        elif cause == "nomd":
            null = lambda k: k in (0, 63)                         # noqa: E731
        elif cause == "adjust":
            M.put(pool, i, seglen=40, data_len=19, clip=19, fix=12)
        elif cause == "short":
            M.put(pool, i, seglen=20, data_len=39, clip=39)
        elif cause == "badoff":
            M.put(pool, i, seglen=40, nib=4)
        else:
            batches[0][i] = None
    want = T.expect(pool, std, batches, zero_copy, now=T.NOW, md_null=null)
    f = [k for k in firsts(want) if k % 512 in where]
    assert f == [64, 512], f
    assert not want["verdicts"][[0, 63]].any() and (want["verdicts"][[64, 255, 256, 511]] & S.VMASK == S.PRED_ACK).all()
    with Queue(cl, pool, std, zero_copy, batch=512, depth=2, md_null=null) as q:
        q.q.set_now(T.NOW)
        q.run(batches, want, outside=other.addr(0))


@pytest.mark.parametrize("how", ["data_len", "stage_max", "region"])
def test_option_bytes_at_the_readable_edge(cl, std, how):
    """The TCP header ends exactly at data_len, at stage_max (staged) and at the
    registered region's end (zero-copy), or is cut there: a 32-byte header (the
    4-word read) and a 60-byte one (the 11-word read); what lies behind reads as
    zero, the length byte at the edge included."""
    for opts, ihl, clip, verdict, ts_val in T.EDGE_CASES_64:
        pool, batches, zc, sm = T.edge_case(std, opts, clip, how, ihl=ihl)
        want = T.expect(pool, std, batches, zc, now=T.NOW, stage_max=sm)
        assert int(want["verdicts"][0]) == verdict | S.FIRST and int(want["opts"]["ts_val"][0]) == ts_val
        with Queue(cl, pool, std, zc, stage_max=sm) as q:
            q.q.set_now(T.NOW)
            q.run(batches, want)


@FORMS
def test_reference_vectors(cl, gpu, zero_copy):
    """tests/golden/tcp_options_ref.npz through the queue: BADOPT exactly where the
    compiled tcp_do_options returned -1, its fields where it returned 0, and the
    branch tcp_header_prediction took, as test_tcp_reference_golden.py expects."""
    G = TG.load()
    seen_p = seen_h = 0
    for k, now in enumerate(G["nows"].tolist()):
        for cases_of, check in ((TG.parse_cases, TG.parse_check), (TG.pred_cases, TG.pred_check)):
            idx, cases = cases_of(G, k)
            if not len(idx):
                continue
            tw = T.TWorld(M.World(len(cases)))
            try:
                pool = M.make_pool(len(cases))
                for i, (tcb, spec) in enumerate(cases):
                    c = tw.w.add(laddr=M.LADDR, lport=5000, faddr=M.PEER, fport=1024 + i)
                    tw.set(c, tcb)
                    T.put_spec(pool, i, dict(spec, pair=T.pair_of(tw.w, c)), data_off=192 + i % 16)
                batches = [list(range(lo, min(lo + 512, len(cases)))) for lo in range(0, len(cases), 512)]
                with Queue(cl, pool, tw, zero_copy, batch=512, depth=4) as q:
                    q.q.set_now(now)
                    for b in batches:
                        q.launch(b)
                    q.drain()
                    e, o, v = (np.concatenate(q.got[j]) for j in (1, 3, 4))
                assert (e == M.TCP_SEG).all() and ((v & S.FIRST) != 0).all()
                check(G, idx, v, o, f"queue, now {now:#x}")
                if cases_of is TG.parse_cases:
                    seen_p += len(idx)
                else:
                    seen_h += len(idx)
            finally:
                tw.close()
    assert seen_p == len(G["p_tail"]) and seen_h == len(G["h_branch"])


@FORMS
def test_tcb_changes_between_batches(cl, gpu, zero_copy):
    """cndp_tcb_set, cndp_tcb_clear and cndp_pcb_del between batches, three
    batches in flight at once (depth 4): each is judged against the tables as
    they stood at its launch."""
    tw = T.standard_tworld()
    try:
        n = 768
        pool = M.make_pool(n)
        for i in range(n):
            c = 2 + (i % 256) % 40
            t = tw.tcbs.get(c) or T.EST
            T.put_spec(pool, i, dict(pair=T.pair_of(tw.w, c), seq=1000 + (c - 2), ack=600, wnd=t["snd_wnd"] >> t["snd_scale"],
                                     flags=S.ACK, opts=T.TS12 if i % 3 else b""), data_off=192 + i % 16)
        batches = M.split(list(range(n)), [256, 256, 256])
        wants = []
        with Queue(cl, pool, tw, zero_copy, batch=256, depth=4) as q:
            q.q.set_now(T.NOW)
            for bi, b in enumerate(batches):
                if bi == 1:
                    tw.set(2, dict(T.EST, rcv_nxt=5))              # changed: SLOW now
                    tw.set(3, dict(T.EST, rcv_nxt=1001))           # new: was none
                    tw.set(4, None)                                # cleared: RESET now
                elif bi == 2:
                    tw.delete(6)                                   # the listener answers, which is LISTEN: SLOW
                    tw.set(2, dict(T.EST, rcv_nxt=1000))
                wants.append(T.expect(pool, tw, [b], zero_copy, now=T.NOW))     # the twin too, against the tables now
                q.launch(b)
            assert q.q.pending == n                                # nothing polled: three batches were in flight
            q.drain()
            want = {k: np.concatenate([w[k] for w in wants]) for k in ("edges", "segs", "opts", "verdicts")}
            want["stats"] = [sum(x) for x in zip(*[w["stats"] for w in wants])]
            want["tstats"] = [sum(x) for x in zip(*[w["tstats"] for w in wants])]
            want["mem"] = wants[0]["mem"].copy()
            for bi, b in enumerate(batches):                      # each batch's mbufs as its own reference left them
                lo, hi = b[0] * FRAME, (b[-1] + 1) * FRAME
                want["mem"][lo:hi] = wants[bi]["mem"][lo:hi]
            q.check(batches, want)
        V = [w["verdicts"] for w in wants]
        assert V[0][0] & S.VMASK == S.PRED_ACK and V[1][0] & S.VMASK == S.SLOW and V[2][0] & S.VMASK == S.PRED_ACK
        assert V[0][1] & S.VMASK == S.CLOSED and V[1][1] & S.VMASK == S.PRED_ACK
        assert V[0][2] & S.VMASK != S.RESET and V[1][2] & S.VMASK == S.RESET
        assert V[1][4] & S.VMASK == S.PRED_ACK and V[2][4] & S.VMASK == S.SLOW
    finally:
        tw.close()


@FORMS
def test_now(cl, std, zero_copy):
    """An echoed timestamp ahead of `now` is zeroed; `now` changed between batches
    reaches the later batch only."""
    pool = M.make_pool(4)
    t = std.tcbs[2]
    spec = dict(pair=T.pair_of(std.w, 2), seq=t["rcv_nxt"], ack=600, wnd=t["snd_wnd"] >> t["snd_scale"], flags=S.ACK,
                opts=bytes([1, 1]) + S.ts_opt(95, 5000))
    for i in range(4):
        T.put_spec(pool, i, spec)
    w0 = T.expect(pool, std, [[0, 1]], zero_copy, now=0)           # 0 until set: 5000 is ahead of it
    w1 = T.expect(pool, std, [[2, 3]], zero_copy, now=5000)
    assert w0["opts"]["ts_ecr"].tolist() == [0, 0] and w1["opts"]["ts_ecr"].tolist() == [5000, 5000]
    with Queue(cl, pool, std, zero_copy, depth=4) as q:
        q.launch([0, 1])
        q.q.set_now(5000)
        q.launch([2, 3])
        q.drain()
        o = np.concatenate(q.got[3])
        assert o["ts_ecr"].tolist() == [0, 0, 5000, 5000] and o["ts_val"].tolist() == [95] * 4


@FORMS
def test_table_of_4096(cl, gpu, zero_copy):
    """A full table with a TCB on every PCB: indices above 255 and index 4095."""
    tw = T.TWorld(M.big_world())
    try:
        for i in range(4096):
            if tw.w.ent[i]["lport"]:
                tw.set(i, dict(T.EST, rcv_nxt=i, snd_scale=i % 5, state=S.ESTABLISHED if i % 11 else S.CLOSED_STATE))
        pool = M.make_pool(512)
        for i in range(512):
            k = (i * 4093 // 511) if i % 9 else 50 + 97 * (i // 9)
            T.put_spec(pool, i, dict(pair=((0x0A040007, 5000), (0xC6120001 if k & 1 else 0xC6120002, 10000 + k)),
                                     seq=2 + k, ack=600, wnd=512 >> ((2 + k) % 5), flags=S.ACK, opts=T.TS12 if i % 2 else b""),
                       data_off=192 + i % 16)
        batches = [list(range(512))]
        want = T.expect(pool, tw, batches, zero_copy, now=T.NOW)
        ts = want["tstats"]
        assert ts[S.PRED_ACK - 1] > 300 and ts[S.CLOSED - 1] > 0 and ts[S.SLOW - 1] > 0     # deleted entries: the listener
        with Queue(cl, pool, tw, zero_copy, batch=512, depth=2) as q:
            q.q.set_now(T.NOW)
            q.run(batches, want)
        last = want["mem"].reshape(pool.n, FRAME)[:, :64].view(pool.hdr.dtype)[:, 0]["udata64"][511]
        assert int(last) == 0x7F00DEAD0000 and want["verdicts"][511] & S.VMASK == S.PRED_ACK     # index 4095
    finally:
        tw.close()


def batch_stage(cl, gpu, mem, hdr, idx, tw, now, stream=None):
    """The same frames as a device slab through cndp_gpu_tcp_input + cndp_gpu_tcp_segment
    (every frame selected): (l4edge, opt records, verdicts) once `stream` is synchronised."""
    import torch
    from cndp_amd import pktgen
    offs = np.array([int(i) * FRAME + 64 + int(hdr["data_off"][i]) for i in idx], np.int64)
    l3 = ((hdr["tx_offload"][idx] >> 7) & 0x1FF).astype(np.uint32)
    slab_t = torch.from_numpy(mem.copy()).to(gpu)
    out = {"rxmeta": torch.from_numpy((l3 << 7).astype(np.uint32).view(np.int32).copy()).to(gpu)}
    fr = pktgen.Frames(slab_t, len(idx), stride=0, offsets=torch.from_numpy(offs).to(gpu))
    sel = torch.ones(len(idx), dtype=torch.uint8, device=gpu)
    kw = {} if stream is None else {"stream": stream.cuda_stream}
    tcp = cl.tcp_input(fr, out, tw.tbl, sel=sel, **kw)
    seg = cl.tcp_segment(fr, out, tw.tcb_tbl, tcp, now=now, **kw)
    return fr, tcp, seg


def stage_results(tcp, seg):
    from cndp_amd.l4 import opt_records
    return tcp["l4edge"].cpu().numpy(), opt_records(seg["opt"]), seg["verdict"].cpu().numpy().view(np.uint8)


def plain_fill(pool, tw, seed):
    """Segments with and without options on connections with TCBs, a tenth with a
    bad sum: nothing the batch stage leaves to the host (no ADJUST / SHORT).  The
    pool is zeroed first: the batch stage reads the parser's byte at opt_end from
    the slab whatever lies there, the queue reads zero past data_len, and the two
    can only agree on a segment without payload where that byte is zero."""
    rng = np.random.default_rng(seed)
    pool.mem.reshape(pool.n, FRAME)[:, 64:] = 0
    for i in range(pool.n):
        c = 2 + 2 * int(rng.integers(0, M.NCONN // 2))
        t = tw.tcbs[c]
        _, spec = S.random_case(rng, T.NOW)
        if rng.random() < 0.6:
            spec.update(seq=t["rcv_nxt"], ack=t["snd_una"] + (int(rng.choice([0, 100])) if not spec["payload"] else 0),
                        wnd=t["snd_wnd"] >> (t["snd_scale"] & 31))
        spec["pair"] = T.pair_of(tw.w, c)
        if rng.random() < 0.1:
            spec["bad_cksum"] = True
        T.put_spec(pool, i, spec, data_off=192 + int(rng.integers(0, 16)))


def test_parity_with_the_batch_stages(cl, gpu, std):
    """One batch = one call: opt and verdict (FIRST included) of the queue equal
    cndp_gpu_tcp_input + cndp_gpu_tcp_segment's over the same frames."""
    import torch
    pool = M.make_pool(512)
    plain_fill(pool, std, 77)
    mem0, hdr0 = pool.mem.copy(), pool.hdr.copy()
    batches = [list(range(512))]
    want = T.expect(pool, std, batches, True, now=T.NOW)
    assert want["stats"][M.CKSUM] > 0 and sum(1 for x in want["tstats"] if x) >= 5
    _, tcp, seg = batch_stage(cl, gpu, mem0, hdr0, np.arange(512), std, T.NOW)
    torch.cuda.synchronize()
    l4edge, opt, verdict = stage_results(tcp, seg)
    with Queue(cl, pool, std, True, batch=512, depth=2) as q:
        q.q.set_now(T.NOW)
        e = q.run(batches, want)
    on = e == M.TCP_SEG
    assert on.sum() > 300 and ((l4edge == N.CNDP_L4_EDGE(N.CNDP_L4_NODE_TCP_INPUT, N.CNDP_TCP_INPUT_SEGMENT)) == on).all()
    assert np.array_equal(verdict[on], want["verdicts"][on]) and opt[on].tobytes() == want["opts"][on].tobytes()
    assert not verdict[~on].any()


def test_one_table_two_readers(cl, gpu, std):
    """cndp_gpu_tcp_segment on another stream and the queue on one TCB table,
    interleaved, a TCB changed between the rounds: both are right both times."""
    import torch
    tw = T.standard_tworld()
    try:
        pool = M.make_pool(512)
        plain_fill(pool, tw, 78)
        mem0, hdr0 = pool.mem.copy(), pool.hdr.copy()
        side = torch.cuda.Stream(device=gpu)
        batches = M.split(list(range(512)), [256, 256])
        wants, stage = [], []
        with Queue(cl, pool, tw, True, batch=256, depth=4) as q:
            q.q.set_now(T.NOW)
            for bi, b in enumerate(batches):
                if bi == 1:
                    for c in range(2, 2 + M.NCONN, 2):
                        tw.set(c, dict(tw.tcbs[c], snd_una=tw.tcbs[c]["snd_una"] + 100))
                wants.append(T.expect(pool, tw, [b], True, now=T.NOW))
                q.launch(b)
                with torch.cuda.stream(side):
                    stage.append(batch_stage(cl, gpu, mem0, hdr0, np.array(b), tw, T.NOW, stream=side))
            q.drain()
            side.synchronize()
            e, v, o = (np.concatenate(q.got[j]) for j in (1, 4, 3))
        for bi, b in enumerate(batches):
            w = wants[bi]
            lo = bi * 256
            assert np.array_equal(e[lo:lo + 256], w["edges"]) and np.array_equal(v[lo:lo + 256], w["verdicts"])
            assert o[lo:lo + 256].tobytes() == w["opts"].tobytes()
            _, sopt, sverdict = stage_results(stage[bi][1], stage[bi][2])
            on = w["edges"] == M.TCP_SEG
            assert on.sum() > 100 and np.array_equal(sverdict[on], w["verdicts"][on])
            assert sopt[on].tobytes() == w["opts"][on].tobytes()
        assert not np.array_equal(wants[0]["verdicts"] & S.VMASK, wants[1]["verdicts"] & S.VMASK)
    finally:
        tw.close()


@FORMS
def test_poll_variants_interleaved(cl, std, zero_copy):
    """cndp_gpu_mq_poll, _poll_tcp and _poll_tcpseg taken in turn: every mbuf is
    edited and counted whichever poll returned it."""
    pool = M.make_pool(700)
    T.fill_mix(pool, std, seed=21)
    batches = [b for b in M.split(list(range(700)), [256, 100, 256, 88]) if b]
    want = T.expect(pool, std, batches, zero_copy, now=T.NOW)
    with Queue(cl, pool, std, zero_copy, batch=256, depth=2) as q:
        q.q.set_now(T.NOW)
        q.run(batches, want, variants=True)


def test_chain_behind_udp_input(cl, gpu):
    """One pool through a CNDP_MQ_UDP_INPUT queue; the mbufs that come back on
    ip4_proto's tcp_input edge go through the tcp_segment queue."""
    import mq_udp_ref as U
    uw, tw = U.standard_world(), T.standard_tworld()
    try:
        uw.set_flags(True, True)
        n = 512
        pool = M.make_pool(n)
        T.fill_mix(pool, tw, seed=51)
        for i in range(1, n, 3):                               # a third of it UDP traffic
            U.put(pool, i, dport=[5000, 5002, 4999][(i // 3) % 3], dgram=26 + i % 200,
                  cksum=["good", "last"][(i // 3) % 2], data_off=192 + i % 16)
        want_u = U.expect(pool, uw, M.split(list(range(n)), [256, 256]), False)
        on = [i for i in range(n) if want_u["edges"][i] == U.PROTO_TCP]
        tb = [on[:200], on[200:]]
        assert 200 < len(on) <= 456
        mid = type("P", (), {})()                              # the pool as the UDP stage leaves it
        mid.mem, mid.base, mid.n = want_u["mem"], pool.base, pool.n
        want_t = T.expect(mid, tw, tb, False, now=T.NOW)
        assert want_t["stats"][M.SEGMENT] > 0 and sum(1 for x in want_t["tstats"] if x) >= 5
        uq = MbufQueue(cl, N.CNDP_MQ_UDP_INPUT, batch=256, depth=2, pcb_tbl=uw.tbl, max_delay_us=1000000)
        try:
            addrs, edges = uq.run(pool, np.arange(n), [256, 256])
        finally:
            uq.close()
        assert np.array_equal(edges, want_u["edges"]) and np.array_equal(pool.mem, want_u["mem"])
        assert pool.index_of(addrs[edges == U.PROTO_TCP]).tolist() == on
        with Queue(cl, pool, tw, False) as q:
            q.q.set_now(T.NOW)
            q.run(tb, want_t)
    finally:
        uw.close()
        tw.close()


def test_arguments(cl, std):
    from cndp_amd.l4 import PcbTable, TcbTable
    L = N.lib()
    pool = M.make_pool(4)
    tbl, tcbs = std.tbl, std.tcb_tbl

    def create(mode=N.CNDP_MQ_TCP_SEGMENT, flags=0, batch=256, depth=2, stage_max=0, umem=None, t=tbl.h, tc=tcbs.h, fn=None):
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
        elif fn == "tcp_input":
            r = L.cndp_gpu_mq_create_tcp_input(cl.h, ctypes.byref(c), t, ctypes.byref(h))
        else:
            r = L.cndp_gpu_mq_create_tcp_segment(cl.h, ctypes.byref(c), t, tc, ctypes.byref(h))
        if r == 0:
            L.cndp_gpu_mq_free(h)
        return r

    assert create() == 0
    for fn in ("plain", "fwd", "ip4_forward", "udp_input", "tcp_input"):     # mode 11 needs its own call
        assert create(fn=fn) == -22, fn
    assert create(t=None) == -22 and create(tc=None) == -22
    other = PcbTable(8)
    tcb_other = TcbTable(other)
    try:                                                                     # a TCB table over another PCB table
        assert create(tc=tcb_other.h) == -22 and create(t=other.h) == -22
    finally:
        tcb_other.close()
        other.close()
    c = N.MqConf()
    c.mode = N.CNDP_MQ_TCP_SEGMENT
    assert L.cndp_gpu_mq_create_tcp_segment(cl.h, None, tbl.h, tcbs.h, ctypes.byref(ctypes.c_void_p())) == -22
    assert L.cndp_gpu_mq_create_tcp_segment(cl.h, ctypes.byref(c), tbl.h, tcbs.h, None) == -22
    assert L.cndp_gpu_mq_create_tcp_segment(None, ctypes.byref(c), tbl.h, tcbs.h, ctypes.byref(ctypes.c_void_p())) == -22
    for mode in range(0, 11):
        assert create(mode=mode) == -22
    assert create(mode=12) == -22
    for bit in range(32):
        assert create(flags=1 << bit) == -22
    assert create(batch=255) == -22 and create(batch=(1 << 24) + 1) == -22
    assert create(depth=1) == -22 and create(depth=17) == -22
    assert create(stage_max=63) == -22 and create(stage_max=65536) == -22
    assert create(umem=pool.base) == -22                                        # not registered
    out, ed, sg = (ctypes.c_void_p * 4)(), np.zeros(4, np.uint16), np.zeros(4, M.SEG_DT)
    op, vd = np.zeros(4, T.OPT_DT), np.zeros(4, np.uint8)
    with Queue(cl, pool, std, True) as q:
        assert all(q.q.stat(k) == 0 for k in KEYS + TKEYS) and L.cndp_gpu_mq_stat(q.q.h, 39) == -22
        assert q.q.submit(None, 0) == 0
        assert L.cndp_gpu_mq_poll_tcpseg(q.q.h, out, ed.ctypes.data, None, None, None, 4) == 0    # any of them may be NULL
        assert L.cndp_gpu_mq_poll_tcpseg(q.q.h, None, ed.ctypes.data, None, None, None, 4) == -22
    for mode, kw in ((N.CNDP_MQ_MAC_SWAP, {}), (N.CNDP_MQ_TCP_INPUT, {"pcb_tbl": tbl})):      # the calls and keys are this mode's alone
        o = MbufQueue(cl, mode, batch=256, depth=2, **kw)
        try:
            assert all(L.cndp_gpu_mq_stat(o.h, k) == -22 for k in TKEYS)
            assert L.cndp_gpu_mq_poll_tcpseg(o.h, out, ed.ctypes.data, sg.ctypes.data, op.ctypes.data, vd.ctypes.data, 4) == -22
            assert L.cndp_gpu_mq_tcp_now(o.h, 7) == -22
        finally:
            o.close()


def test_table_bound_to_another_device(gpu):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU: tables bound to cuda:0 must refuse a queue on cuda:1")
    from cndp_amd.classify import Classifier
    tw = T.standard_tworld()
    c0, c1 = Classifier(0), Classifier(1)
    try:
        pool = M.make_pool(4)
        for i in range(4):
            M.put(pool, i)
        with Queue(c0, pool, tw, False) as q:       # its first batch binds both tables to cuda:0
            q.run([[0, 1, 2, 3]], T.expect(pool, tw, [[0, 1, 2, 3]], False))
        with pytest.raises(OSError) as e:
            MbufQueue(c1, N.CNDP_MQ_TCP_SEGMENT, batch=256, depth=2, pcb_tbl=tw.tbl, tcb=tw.tcb_tbl)
        assert e.value.errno == 22
    finally:
        c0.close()
        c1.close()
        tw.close()

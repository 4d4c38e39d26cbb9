"""cndpfwd's fwd, l3fwd and ACL modes as modes of the asynchronous mbuf queue
(cndp_gpu_mq_create_fwd, include/cndp_mqfwd.h), zero-copy and staged, over
pools of at most 1024 mbufs laid out like CNDP's (batch 256, depth 2).

Every expected value comes twice: from the numpy restatements of the reference
loops (tests/cfwd_ref.py, tests/acl_ref.py, independent of the library) and from
the host twins (cndp_cfwd_host, cndp_acl_classify_host) run over a copy of the
pool.  The edges, the counters and the WHOLE pool memory -- mbuf headers and the
bytes no mode may touch included -- are compared exactly.

A frame's readable length is what the queue defines: zero-copy, up to the end of
the registered region; staged, buf_len - data_off.  Bytes past it read as zero
and are never written; the restatements and the twins get the same bound as
slab_len."""
import ctypes
import errno

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.acl import AclTable
from cndp_amd.cfwd import cfwd_host, l3fwd_fib, route_add
from cndp_amd.fib import Fib
from cndp_amd.mbuf import FRAME, MbufPool, MbufQueue

import acl_ref as A
import cfwd_ref as C

pytestmark = pytest.mark.gpu

NONE = N.CNDP_MQ_EDGE_NONE
FWD_KEYS = (N.CNDP_MQ_STAT_FORWARD, N.CNDP_MQ_STAT_ECHO)
ACL_KEYS = (N.CNDP_MQ_STAT_ACL_PREFILTER, N.CNDP_MQ_STAT_ACL_DENY, N.CNDP_MQ_STAT_ACL_PERMIT)
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "staged"])
MACS = {1: "02:aa:00:00:00:01", 2: "02:bb:00:00:00:02", 70: "02:cc:00:00:00:46", 9: "02:dd:00:00:00:09"}


@pytest.fixture(scope="module")
def cl(gpu):
    from cndp_amd.classify import Classifier
    c = Classifier(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------
# pools, the queue driver, the two references
# ---------------------------------------------------------------------------
def make_pool(n, rows, seed=11, data_len=None):
    """n mbufs, every byte behind the headers random, frame i = rows[i] at its mtod."""
    pool = MbufPool(n)
    rng = np.random.default_rng(seed)
    pool.mem.reshape(n, FRAME)[:, 64:] = rng.integers(0, 256, (n, FRAME - 64), dtype=np.uint8)
    place(pool, rows)
    pool.hdr["data_len"] = rows.shape[1] if data_len is None else data_len
    pool.hdr["udata64"] = 0xABABABABABABABAB
    return pool


def place(pool, rows, idx=None):
    """rows[k] to the mtod of mbuf idx[k], the part of it that fits the mbuf's 2 KiB."""
    idx = np.arange(len(rows)) if idx is None else np.asarray(idx)
    d = pool.data_pos().astype(np.int64)
    for k, i in enumerate(idx):
        m = min(rows.shape[1], (int(i) + 1) * FRAME - int(d[i]))     # never into the next mbuf
        pool.mem[d[i]:d[i] + m] = rows[k, :m]


def readable(pool, zero_copy):
    """Bytes of each frame the queue may read (see the module docstring)."""
    d = pool.data_pos().astype(np.int64)
    if zero_copy:
        return pool.mem.size - d
    return np.maximum(pool.hdr["buf_len"].astype(np.int64) - pool.hdr["data_off"].astype(np.int64), 0)


class Queue:
    """A cndpfwd-mode queue over `pool`, registered first when zero-copy."""

    def __init__(self, cl, pool, mode, zero_copy, **kw):
        self.cl, self.pool, self.zc = cl, pool, zero_copy
        if zero_copy:
            cl.host_register(pool.mem)
        try:
            self.q = MbufQueue(cl, mode, batch=256, depth=2, umem=pool.base if zero_copy else None, **kw)
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

    def drive(self, addrs, bursts):
        """Submit the mbufs at `addrs` as bursts, polling as cndpfwd's loop would,
        until all are back: (addresses, edges) in completion order."""
        q = self.q
        addrs = [int(a) for a in addrs]
        assert sum(bursts) == len(addrs)
        got_a, got_e, pos = [], [], 0
        for b in bursts:
            ptrs = (ctypes.c_void_p * b)(*addrs[pos:pos + b])
            done = 0
            while done < b:
                k = q.submit(ctypes.addressof(ptrs) + done * ctypes.sizeof(ctypes.c_void_p), b - done)
                done += k
                a, e = q.poll()
                got_a.append(a)
                got_e.append(e)
                if k == 0 and a.size == 0:
                    q.wait()
            pos += b
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

    def stats(self):
        return {k: self.q.stat(k) for k in FWD_KEYS + ACL_KEYS}


def groups(n, rd, skip):
    """(sel, slab_len) runs for the references: every frame whose 34 bytes are
    readable in one run over the whole memory, each shorter one alone, bounded."""
    full = (rd >= 34) & ~skip
    out = [(full, None)] if full.any() else []
    for i in np.nonzero((rd < 34) & ~skip)[0]:
        s = np.zeros(n, bool)
        s[i] = True
        out.append((s, int(i)))
    return out


def expect(kind, pool, zero_copy, P, skip=None, twin=True):
    """Edges and pool memory after one pass of mode `kind` ('fwd', 'l3', 'acl')
    over every mbuf of the pool, from the restatement; with twin the host twin
    is run the same way and must agree with it byte for byte."""
    n = pool.n
    skip = np.zeros(n, bool) if skip is None else skip
    start = pool.data_pos().astype(np.int64)
    rd = readable(pool, zero_copy)
    dlen = pool.hdr["data_len"].copy()
    want = {"edges": np.full(n, NONE, np.uint16)}
    mem_ref, mem_twin = pool.mem.copy(), pool.mem.copy()
    for sel, one in groups(n, rd, skip):
        slab_len = pool.mem.size if one is None else int(start[one] + rd[one])
        s8 = sel.astype(np.uint8)
        if kind == "acl":
            kw = dict(mode=P["acl_mode"], swap=P["swap"], in_lport=P["in_lport"], lports=P["lports"], sel=s8, length=dlen,
                      offsets=start.astype(np.uint64), slab_len=slab_len)
            r = A.acl_fwd_ref(mem_ref, n, P["rules"], **kw)
            e = np.where(r["verdict"] == A.FORWARD, r["tx_lport"].astype(np.uint16),
                         np.where(r["verdict"] == A.DENIED, N.CNDP_MQ_EDGE_ACL_DENY, N.CNDP_MQ_EDGE_ACL_PREFILTER))
            if twin:
                t = P["acl"].classify_host(mem_twin, n, **kw)
                assert np.array_equal(t["verdict"], r["verdict"]) and np.array_equal(t["tx_lport"], r["tx_lport"])
        else:
            mode = C.FWD if kind == "fwd" else C.L3FWD
            kw = dict(in_lport=P["in_lport"], lports=P["lports"], sel=s8, offsets=start.astype(np.uint64), slab_len=slab_len)
            r = C.cfwd_ref(mem_ref, n, mode, routes=P.get("routes"), **kw)
            e = r["tx_lport"] | (r["echoed"].astype(np.uint16) << 8)
            if twin:
                t = cfwd_host(mem_twin, n, mode, fib=P.get("fib"), **kw)
                assert np.array_equal(t["tx_lport"], r["tx_lport"]) and np.array_equal(t["echoed"], r["echoed"])
        want["edges"][sel] = e[sel].astype(np.uint16)
        mem_ref = r["slab"]
        if twin:
            assert np.array_equal(mem_twin, mem_ref), "the host twin and the restatement disagree"
    want["mem"] = mem_ref
    return want


def check(pool, addrs, edges, want, order=None):
    order = np.arange(pool.n) if order is None else order
    assert np.array_equal(pool.index_of(addrs), order), "mbufs came back out of submission order"
    bad = np.nonzero(edges != want["edges"][order])[0]
    assert len(bad) == 0, f"edges: {len(bad)} differ, first at {bad[0]}: got {edges[bad[0]]:#x} want {want['edges'][order][bad[0]]:#x}"
    bad = np.nonzero(pool.mem != want["mem"])[0]
    assert len(bad) == 0, f"pool memory: {len(bad)} bytes differ, first at mbuf {bad[0] // FRAME} + {bad[0] % FRAME}"


def acl_counts(edges):
    e = edges[edges != NONE]
    return {N.CNDP_MQ_STAT_ACL_PREFILTER: int((e == N.CNDP_MQ_EDGE_ACL_PREFILTER).sum()),
            N.CNDP_MQ_STAT_ACL_DENY: int((e == N.CNDP_MQ_EDGE_ACL_DENY).sum()),
            N.CNDP_MQ_STAT_ACL_PERMIT: int((e < 256).sum())}


# ---------------------------------------------------------------------------
# fwd
# ---------------------------------------------------------------------------
@FORMS
def test_fwd(cl, zero_copy):
    """_fwd_test over 512 mbufs in bursts [256, 255, 1]: p[5] names known ports
    (one above 63, one above 191), unknown ones (echo) and in_lport itself."""
    n, in_lport, lports = 512, 3, (1, 3, 70, 200)
    dmac5 = np.array([1, 70, 200, 9, 3, 255, 64, 0])[np.arange(n) % 8]
    rows = C.frames(np.arange(n, dtype=np.uint32), dmac5=dmac5, seed=5)
    pool = make_pool(n, rows)
    P = dict(in_lport=in_lport, lports=lports)
    want = expect("fwd", pool, zero_copy, P)
    with Queue(cl, pool, N.CNDP_MQ_CFWD_FWD, zero_copy, lport=in_lport, lports=lports) as q:
        addrs, edges = q.drive(pool.base + np.arange(n) * FRAME, [256, 255, 1])
        st = q.stats()
    check(pool, addrs, edges, want)
    assert set(np.unique(edges).tolist()) == {1, 3, 70, 200, 3 | N.CNDP_MQ_EDGE_ECHO}
    assert st[N.CNDP_MQ_STAT_FORWARD] + st[N.CNDP_MQ_STAT_ECHO] == 512
    assert st[N.CNDP_MQ_STAT_ECHO] == int((edges & N.CNDP_MQ_EDGE_ECHO != 0).sum()) == 512 // 2
    assert all(st[k] == 0 for k in ACL_KEYS)                  # another mode's family
    assert q.q._L.cndp_gpu_mq_stat(None, N.CNDP_MQ_STAT_ECHO) == -22


# ---------------------------------------------------------------------------
# l3fwd
# ---------------------------------------------------------------------------
ROUTES = [(0x0A020000, 16, 1), (0x0A010200, 24, 2), (0x0A010300, 24, 70), (0x0A010210, 28, 1), (0x0A010281, 32, 70),
          (0x0B000000, 8, 9)]                                 # port 9 is in no mask: echo
DSTS = np.array([0x0A010205, 0x0A010211, 0x0A01021F, 0x0A010220, 0x0A010281, 0x0A010282, 0x0A020304, 0x0A010309,
                 0x0B010101, 0x0C000001, 0xC0A80001], np.uint32)   # the last two miss: port 0, broadcast


def mac(port) -> bytes:
    return bytes(int(x, 16) for x in MACS[port].split(":"))


def l3_tables(routes=ROUTES, name="mq-l3fwd"):
    fib = l3fwd_fib(name)
    table = {}
    for ip, depth, port in routes:
        route_add(fib, ip, depth, MACS[port], port)
        table[(ip & C.mask(depth), depth)] = C.nexthop(mac(port), port)
    return fib, table


def l3_rows(n, seed=7):
    ck = np.array([0x0000, 0xFFFF, 0xFEFF, 0xFF00, 0x00FF, 0x1234, 0xB1E6], np.uint16)[np.arange(n) % 7]
    ttl = np.array([0, 1, 64, 255, 2])[np.arange(n) % 5]
    rows = C.frames(DSTS[np.arange(n) % len(DSTS)], ttl=ttl, ck=ck, seed=seed)
    rows[5::13, 12:14] = (0x08, 0x06)                         # not IPv4: edited all the same
    return rows


@FORMS
@pytest.mark.parametrize("port0", [True, False], ids=["port0_known", "port0_unknown"])
def test_l3fwd(cl, zero_copy, port0):
    """_l3fwd_test over 768 mbufs in bursts [3, 256, 61, 256, 192]: a /16, /24s, a
    /28 and a /32 behind a /24 (tbl8), misses (port 0, broadcast MAC; echoed when
    port 0 does not exist), a route to a port that is in no mask (echoed, TTL and
    checksum edited all the same), the checksum's carry cases, TTL 0 and 1."""
    n, in_lport = 768, 5
    lports = (0, 1, 2, 5, 70) if port0 else (1, 2, 5, 70)
    fib, table = l3_tables()
    pool = make_pool(n, l3_rows(n))
    P = dict(in_lport=in_lport, lports=lports, routes=table, fib=fib)
    want = expect("l3", pool, zero_copy, P)
    with Queue(cl, pool, N.CNDP_MQ_CFWD_L3FWD, zero_copy, lport=in_lport, lports=lports, fib=fib) as q:
        addrs, edges = q.drive(pool.base + np.arange(n) * FRAME, [3, 256, 61, 256, 192])
        st = q.stats()
    fib.close()
    check(pool, addrs, edges, want)
    seen = set(np.unique(edges).tolist())
    assert {1, 2, 70, in_lport | N.CNDP_MQ_EDGE_ECHO} <= seen and (0 in seen) == port0
    echo = int((edges & N.CNDP_MQ_EDGE_ECHO != 0).sum())
    assert (st[N.CNDP_MQ_STAT_FORWARD], st[N.CNDP_MQ_STAT_ECHO]) == (n - echo, echo)
    d = pool.data_pos().astype(np.int64)
    assert np.array_equal(pool.mem[d + 22], (l3_rows(n)[:, 22].astype(np.int64) - 1) & 0xFF)


@FORMS
def test_l3fwd_route_churn(cl, zero_copy):
    """Routes added and deleted between batches reach the next batch."""
    n, in_lport, lports = 256, 0, (0, 1, 2, 70)
    fib, table = l3_tables(name="mq-l3fwd-churn")
    pool = make_pool(n, l3_rows(n, seed=9))
    P = dict(in_lport=in_lport, lports=lports, routes=table, fib=fib)
    addr = pool.base + np.arange(n) * FRAME
    with Queue(cl, pool, N.CNDP_MQ_CFWD_L3FWD, zero_copy, lport=in_lport, lports=lports, fib=fib) as q:
        want = expect("l3", pool, zero_copy, P)
        a, e1 = q.drive(addr, [256])
        check(pool, a, e1, want)
        route_add(fib, 0x0C000000, 8, MACS[70], 70)           # 12/8 missed before
        table[(0x0C000000, 8)] = C.nexthop(mac(70), 70)
        assert fib.delete(0x0A010210, 28) == 0                # 10.1.2.17 falls back to the /24
        del table[(0x0A010210, 28)]
        want = expect("l3", pool, zero_copy, P)
        a, e2 = q.drive(addr, [256])
        check(pool, a, e2, want)
        assert q.stats()[N.CNDP_MQ_STAT_FORWARD] + q.stats()[N.CNDP_MQ_STAT_ECHO] == 2 * n
    fib.close()
    k = np.arange(n) % len(DSTS)
    assert np.all(e1[k == 9] == 0) and np.all(e2[k == 9] == 70)
    assert np.all(e1[k == 1] == 1) and np.all(e2[k == 1] == 2)


# ---------------------------------------------------------------------------
# acl
# ---------------------------------------------------------------------------
SMALL = [(0, 0, 0x64010200, 24, 1), (0x0C000000, 8, 0, 0, 1), (0xD2000001, 32, 0x6E000001, 32, 0)]
ANY = (0, 0, 0, 0, 0)
PAIRS = {"permit": (0xD2000001, 0x6E000001), "deny_dst": (0x01020304, 0x64010263), "deny_src": (0x0C222222, 0x05050505),
         "none": (0x01010101, 0x02020202)}


def acl_table(rows):
    t = AclTable()
    for s, sm, d, dm, deny in rows:
        t.add(s, sm, d, dm, bool(deny))
    t.build()
    return t


def acl_small_pool(n, seed=3):
    """Ten kinds of frame by i % 10, dmac5 by i % 3 (a known port, an unknown one, one above 63)."""
    kind = np.arange(n) % 10
    pair = [PAIRS["permit"], PAIRS["deny_dst"], PAIRS["deny_src"], PAIRS["none"]] + [PAIRS["permit"]] * 6
    src = np.array([pair[k][0] for k in kind], np.uint32)
    dst = np.array([pair[k][1] for k in kind], np.uint32)
    rows = A.frames(src, dst, dmac5=np.array([1, 9, 70])[np.arange(n) % 3], seed=seed)
    rows[kind == 4, 14] = 0x65                                # not version 4
    rows[kind == 5, 14] = 0x44                                # IHL 4
    rows[kind == 6, 16], rows[kind == 6, 17] = 0, 19          # total length 19
    rows[kind == 9, 14] = 0x46                                # IP options: the fields stay at fixed offsets
    dlen = np.full(n, 64, np.uint16)
    dlen[kind == 7], dlen[kind == 8] = 19, 20
    return make_pool(n, rows, data_len=dlen), kind


@FORMS
@pytest.mark.parametrize("any_last", [False, True], ids=["no_any_rule", "any_rule_last"])
@pytest.mark.parametrize("swap", [False, True], ids=["no_swap", "mac_swap"])
@pytest.mark.parametrize("acl_mode", [N.CNDP_ACL_STRICT, N.CNDP_ACL_PERMISSIVE], ids=["strict", "permissive"])
def test_acl_small_table(cl, zero_copy, acl_mode, swap, any_last):
    """acl_fwd_test over 512 mbufs in bursts [256, 7, 249] on a four-group table."""
    n, in_lport, lports = 512, 2, (1, 2, 70)
    rows = SMALL + ([ANY] if any_last else [])
    t = acl_table(rows)
    pool, kind = acl_small_pool(n)
    before = pool.mem.copy()
    P = dict(in_lport=in_lport, lports=lports, rules=A.rules_of(rows), acl=t, acl_mode=acl_mode, swap=swap)
    want = expect("acl", pool, zero_copy, P)
    with Queue(cl, pool, N.CNDP_MQ_ACL_FWD, zero_copy, lport=in_lport, lports=lports, acl=t, acl_mode=acl_mode,
               acl_flags=N.CNDP_ACL_F_MAC_SWAP if swap else 0) as q:
        addrs, edges = q.drive(pool.base + np.arange(n) * FRAME, [256, 7, 249])
        st = q.stats()
    t.close()
    check(pool, addrs, edges, want)
    assert {k: st[k] for k in ACL_KEYS} == acl_counts(edges) and sum(st[k] for k in ACL_KEYS) == n
    assert st[N.CNDP_MQ_STAT_FORWARD] == st[N.CNDP_MQ_STAT_ECHO] == 0
    if not swap:
        assert np.array_equal(pool.mem, before)
    for k in (4, 5, 6, 7):
        assert np.all(edges[kind == k] == N.CNDP_MQ_EDGE_ACL_PREFILTER)
    assert np.all(edges[(kind == 1) | (kind == 2)] == N.CNDP_MQ_EDGE_ACL_DENY)
    for k in (0, 8, 9):
        assert set(edges[kind == k].tolist()) == {1, 2, 70}    # the unknown port 9 goes back to in_lport, no echo bit
    fwd_none = any_last or acl_mode == N.CNDP_ACL_PERMISSIVE
    assert np.all((edges[kind == 3] < 256) == fwd_none)


@FORMS
def test_acl_default_rules(cl, zero_copy):
    """cndp_acl_add_init_rules (4226 rules, four groups): 512 frames that hit each
    of its four families and that miss."""
    n, in_lport, lports = 512, 0, (0, 1)
    rules = A.golden("a")["rules"]
    assert len(rules["src_addr"]) == N.CNDP_ACL_INIT_RULES
    t = AclTable()
    t.add_init_rules()
    t.build()
    rng = np.random.default_rng(21)
    fam, j = np.arange(n) % 5, np.arange(n) // 5
    rnd = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    src = np.select([fam == 1, fam == 2, fam == 3], [((10 + j % 15) << 24) | (rnd & 0xFFFFFF), 0x65000000 | ((j % 15) << 8) | (rnd & 0xFF),
                                                      0xD2000000 | (j * 41 % 4096)], 0x01010101).astype(np.uint32)
    dst = np.select([fam == 0, fam == 3], [0x64000000 | ((j % 100) << 16) | (rnd & 0xFF), 0x6E000000 | (j * 41 % 4096)],
                    0x02020202).astype(np.uint32)
    pool = make_pool(n, A.frames(src, dst, dmac5=np.arange(n) % 3, seed=8))
    P = dict(in_lport=in_lport, lports=lports, rules=rules, acl=t, acl_mode=N.CNDP_ACL_STRICT, swap=True)
    want = expect("acl", pool, zero_copy, P)
    res = A.classify(rules, src, dst)
    idx = res & 0x0FFFFFFF
    deny = (res & A.DENY) != 0
    assert (deny & (idx < 100)).any() and (deny & (idx >= 100) & (idx < 115)).any() and (deny & (idx >= 115)).any()
    assert (~deny & (res != 0)).any() and (res == 0).any()
    with Queue(cl, pool, N.CNDP_MQ_ACL_FWD, zero_copy, lport=in_lport, lports=lports, acl=t, acl_mode=N.CNDP_ACL_STRICT,
               acl_flags=N.CNDP_ACL_F_MAC_SWAP) as q:
        addrs, edges = q.drive(pool.base + np.arange(n) * FRAME, [256, 256])
        st = q.stats()
    t.close()
    check(pool, addrs, edges, want)
    assert {k: st[k] for k in ACL_KEYS} == acl_counts(edges)
    assert np.all(edges[fam == 3] < 256) and np.all(edges[fam != 3] == N.CNDP_MQ_EDGE_ACL_DENY)


@FORMS
def test_acl_rebuild_between_batches(cl, zero_copy):
    """A batch, then cndp_acl_clear + new rules + cndp_acl_build: the next batch
    follows the new image.  Then a build on zero rules leaves no image: the next
    batch comes back all CNDP_MQ_EDGE_NONE with the frames untouched and the
    following submit returns -ENOENT; after a good build the queue works again."""
    n, in_lport, lports = 256, 2, (1, 2, 70)
    t = acl_table(SMALL)
    pool, kind = acl_small_pool(n, seed=4)
    addr = pool.base + np.arange(n) * FRAME
    P = dict(in_lport=in_lport, lports=lports, rules=A.rules_of(SMALL), acl=t, acl_mode=N.CNDP_ACL_STRICT, swap=True)
    with Queue(cl, pool, N.CNDP_MQ_ACL_FWD, zero_copy, lport=in_lport, lports=lports, acl=t, acl_mode=N.CNDP_ACL_STRICT,
               acl_flags=N.CNDP_ACL_F_MAC_SWAP) as q:
        want = expect("acl", pool, zero_copy, P)
        a, e1 = q.drive(addr, [256])
        check(pool, a, e1, want)
        flipped = [(0xD2000001, 32, 0x6E000001, 32, 1), (0, 0, 0x64010200, 24, 0)]    # permit <-> deny
        t.clear()
        for s, sm, d, dm, deny in flipped:
            t.add(s, sm, d, dm, bool(deny))
        t.build()
        P["rules"] = A.rules_of(flipped)
        want = expect("acl", pool, zero_copy, P)
        a, e2 = q.drive(addr, [256])
        check(pool, a, e2, want)
        assert np.all(e1[kind == 0] < 256) and np.all(e2[kind == 0] == N.CNDP_MQ_EDGE_ACL_DENY)
        assert np.all(e1[kind == 1] == N.CNDP_MQ_EDGE_ACL_DENY) and np.all(e2[kind == 1] < 256)

        t.clear()
        assert t.build_raw() == -errno.EINVAL                  # no rules: no image
        before, counted = pool.mem.copy(), q.stats()
        ptrs = pool.ptrs(np.arange(n))
        assert q.q.submit(ptrs, n) == n                        # accepted; the launch fails behind it
        a, e3 = q.q.poll()
        assert np.array_equal(pool.index_of(a), np.arange(n)) and np.all(e3 == NONE)
        assert np.array_equal(pool.mem, before) and q.stats() == counted and q.q.pending == 0
        with pytest.raises(OSError) as ex:
            q.q.submit(ptrs, n)
        assert ex.value.errno == errno.ENOENT

        for s, sm, d, dm, deny in SMALL:
            t.add(s, sm, d, dm, bool(deny))
        t.build()
        P["rules"] = A.rules_of(SMALL)
        want = expect("acl", pool, zero_copy, P)
        a, e4 = q.drive(addr, [256])
        check(pool, a, e4, want)
        assert np.all(e4[kind == 0] < 256)
    t.close()


# ---------------------------------------------------------------------------
# frame placement
# ---------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("kind", ["l3", "acl"])
def test_frame_placement(cl, zero_copy, kind):
    """Odd data_off and data_off = 2 (mod 4) (the byte paths); mbufs whose buffer
    ends 20 and 0 bytes behind data_off; the pool's last mbuf with fewer than 34
    bytes before the end of the region; zero-copy, an mbuf of a pool that is not
    registered.  Every result equals the references given the same readable length."""
    n, in_lport, lports = 96, 0, (0, 1, 2, 70)
    fib, table = l3_tables(name="mq-l3fwd-place")
    t = acl_table(SMALL + [ANY])
    if kind == "l3":
        rows = l3_rows(n, seed=13)
    else:
        src = np.array([PAIRS[k][0] for k in ("permit", "deny_dst", "none")], np.uint32)[np.arange(n) % 3]
        dst = np.array([PAIRS[k][1] for k in ("permit", "deny_dst", "none")], np.uint32)[np.arange(n) % 3]
        rows = A.frames(src, dst, dmac5=np.array([1, 9, 70, 2])[np.arange(n) % 4], seed=13)
    pool = make_pool(n, rows)
    h = pool.hdr
    h["data_off"][0:48] = 192 + np.arange(48) % 4 + 4 * (np.arange(48) % 5)     # every alignment
    h["data_off"][60], h["buf_len"][60] = 300, 320                              # 20 bytes of buffer left
    h["data_off"][61], h["buf_len"][61] = 300, 300                              # none
    h["data_off"][62], h["buf_len"][62] = 301, 334                              # 33, unaligned
    h["data_off"][n - 1] = FRAME - 64 - 20                                      # 20 bytes before the pool's end
    h["data_off"][n - 2] = FRAME - 64 - 33                                      # 33 readable staged; zero-copy reads on
    place(pool, rows)                                                           # ... into the next mbuf's header
    other = make_pool(2, rows[:2], seed=17)
    P = dict(in_lport=in_lport, lports=lports, routes=table, fib=fib, rules=A.rules_of(SMALL + [ANY]), acl=t,
             acl_mode=N.CNDP_ACL_STRICT, swap=True)
    rd = readable(pool, zero_copy)
    assert rd[n - 1] == 20 and (zero_copy or (rd[60], rd[61], rd[62], rd[n - 2]) == (20, 0, 33, 33))
    want = expect(kind, pool, zero_copy, P)
    addr = (pool.base + np.arange(n) * FRAME).tolist()
    order = np.arange(n)
    if zero_copy:                                             # two strangers in the middle of the burst
        addr[40:40] = [other.addr(0), other.addr(1)]
    other_before = other.mem.copy()
    kw = dict(fib=fib) if kind == "l3" else dict(acl=t, acl_mode=N.CNDP_ACL_STRICT, acl_flags=N.CNDP_ACL_F_MAC_SWAP)
    with Queue(cl, pool, N.CNDP_MQ_CFWD_L3FWD if kind == "l3" else N.CNDP_MQ_ACL_FWD, zero_copy, lport=in_lport,
               lports=lports, **kw) as q:
        addrs, edges = q.drive(addr, [len(addr)])
        st = q.stats()
    fib.close()
    t.close()
    assert addrs.tolist() == addr
    if zero_copy:
        assert np.all(edges[40:42] == NONE) and np.array_equal(other.mem, other_before)
        addrs, edges = np.delete(addrs, [40, 41]), np.delete(edges, [40, 41])
    check(pool, addrs, edges, want, order)
    keys = FWD_KEYS if kind == "l3" else ACL_KEYS
    assert sum(st[k] for k in keys) == n                      # CNDP_MQ_EDGE_NONE mbufs count nowhere
    if kind == "acl" and not zero_copy:
        assert edges[61] == N.CNDP_MQ_EDGE_ACL_PREFILTER      # no readable byte: version 0


# ---------------------------------------------------------------------------
# argument rules
# ---------------------------------------------------------------------------
def test_argument_rules(cl):
    L = N.lib()
    fib, _ = l3_tables(name="mq-l3fwd-args")
    fib4 = Fib("mq-args-4b", N.CNE_FIB_DIR24_8, default_nh=0, max_routes=16, nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=16)
    built, empty = acl_table(SMALL), AclTable()

    def create(mode, fwd=True, **kw):
        c, w, h = N.MqConf(), N.MqFwd(), ctypes.c_void_p()
        c.mode, c.batch, c.depth = mode, 256, 2
        for k in ("flags", "lport", "batch", "depth", "stage_max"):
            if k in kw:
                setattr(c, k, kw[k])
        f, a = kw.get("fib"), kw.get("acl")
        w.fib, w.acl = f.h if f else None, a.h if a else None
        w.acl_mode, w.acl_flags = kw.get("acl_mode", 0), kw.get("acl_flags", 0)
        w.lport_mask[0] = 3
        rc = L.cndp_gpu_mq_create_fwd(cl.h, ctypes.byref(c), ctypes.byref(w) if fwd else None, ctypes.byref(h))
        if rc == 0:
            L.cndp_gpu_mq_free(h)
        else:
            assert not h.value
        return rc

    FWD, L3, ACL = N.CNDP_MQ_CFWD_FWD, N.CNDP_MQ_CFWD_L3FWD, N.CNDP_MQ_ACL_FWD
    assert create(FWD) == 0 and create(L3, fib=fib) == 0 and create(ACL, acl=built) == 0
    assert create(ACL, acl=built, acl_mode=N.CNDP_ACL_PERMISSIVE, acl_flags=N.CNDP_ACL_F_MAC_SWAP, lport=255) == 0
    assert create(FWD, fwd=False) == -22                                     # a NULL argument
    for mode in (0, 1, 2, 3, 7, 8, 0xFFFFFFFF):                              # a mode outside 4-6
        assert create(mode, fib=fib, acl=built) == -22
    for mode, kw in ((FWD, {}), (L3, dict(fib=fib)), (ACL, dict(acl=built))):
        for flag in (N.CNDP_MQ_F_HASH, N.CNDP_MQ_F_DEVICE_HEADERS, N.CNDP_MQ_F_HOST_WRITEBACK, 1 << 31):
            assert create(mode, flags=flag, **kw) == -22                     # the new modes take no flag
        assert create(mode, lport=256, **kw) == -22
        assert create(mode, batch=255, **kw) == -22 and create(mode, depth=1, **kw) == -22     # the existing rules
        assert create(mode, depth=17, **kw) == -22 and create(mode, stage_max=63, **kw) == -22
    assert create(L3) == -22 and create(L3, fib=fib4) == -22                 # no FIB, another entry width
    assert create(ACL) == -22                                                # no table
    assert create(ACL, acl=built, acl_mode=2) == -22 and create(ACL, acl=built, acl_flags=2) == -22
    assert create(ACL, acl=empty) == -errno.ENOENT                           # a table without an image
    # an unregistered umem, as for every mode
    c, w, h = N.MqConf(), N.MqFwd(), ctypes.c_void_p()
    c.mode, c.batch, c.depth, c.umem = FWD, 256, 2, 4096
    assert L.cndp_gpu_mq_create_fwd(cl.h, ctypes.byref(c), ctypes.byref(w), ctypes.byref(h)) == -22
    # cndp_gpu_mq_create has no tables to use
    for mode in (FWD, L3, ACL, 7):
        c.mode, c.umem = mode, None
        assert L.cndp_gpu_mq_create(cl.h, ctypes.byref(c), ctypes.byref(h)) == -22
    for x in (fib, fib4, built, empty):
        x.close()


# ---------------------------------------------------------------------------
# the queue and cndp_gpu_acl_fwd on one table
# ---------------------------------------------------------------------------
def test_acl_queue_and_batch_call_share_a_table(cl):
    """A CNDP_MQ_ACL_FWD queue (its own stream) and cndp_gpu_acl_fwd on another
    stream alternate on one table, with a rebuild in between: two rounds, both
    give the restatement's answers (the mirror's event ordering)."""
    import torch
    from cndp_amd import pktgen
    n, in_lport, lports = 256, 2, (1, 2, 70)
    t = acl_table(SMALL)
    pool, kind = acl_small_pool(n, seed=6)
    addr = pool.base + np.arange(n) * FRAME
    side = torch.cuda.Stream()
    rule_sets = [SMALL, [(0xD2000001, 32, 0x6E000001, 32, 1), ANY]]
    P = dict(in_lport=in_lport, lports=lports, acl=t, acl_mode=N.CNDP_ACL_PERMISSIVE, swap=False)
    d = pool.data_pos().astype(np.int64)
    with Queue(cl, pool, N.CNDP_MQ_ACL_FWD, False, lport=in_lport, lports=lports, acl=t,
               acl_mode=N.CNDP_ACL_PERMISSIVE) as q:
        for rnd, rows in enumerate(rule_sets):
            if rnd:
                t.clear()
                for s, sm, dd, dm, deny in rows:
                    t.add(s, sm, dd, dm, bool(deny))
                t.build()
            P["rules"] = A.rules_of(rows)
            want = expect("acl", pool, False, P)
            # the batch call first mirrors the new image on its stream, the queue follows on its own
            packed = np.ascontiguousarray(pool.mem[d[:, None] + np.arange(64)])
            fr = pktgen.Frames(torch.from_numpy(packed.reshape(-1)).to("cuda:0"), n, stride=64)
            ln = torch.from_numpy(pool.hdr["data_len"].astype(np.int16)).to("cuda:0")
            torch.cuda.synchronize()
            r = cl.acl_fwd(fr, t, mode=N.CNDP_ACL_PERMISSIVE, swap=False, in_lport=in_lport, lports=lports, length=ln,
                           stream=side.cuda_stream)
            a, e = q.drive(addr, [256])
            r2 = cl.acl_fwd(fr, t, mode=N.CNDP_ACL_PERMISSIVE, swap=False, in_lport=in_lport, lports=lports, length=ln,
                            stream=side.cuda_stream)
            side.synchronize()
            check(pool, a, e, want)
            ref = A.acl_fwd_ref(packed.reshape(-1), n, P["rules"], mode=A.PERMISSIVE, in_lport=in_lport, lports=lports,
                                length=pool.hdr["data_len"], stride=64)
            for res in (r, r2):
                assert np.array_equal(res["verdict"].cpu().numpy(), ref["verdict"])
                assert np.array_equal(res["tx_lport"].cpu().numpy(), ref["tx_lport"])
            assert np.all((e[kind == 0] < 256) == (rnd == 0))
    cl.stream_release(side.cuda_stream)
    t.close()

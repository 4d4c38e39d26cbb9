"""Host side of the ip4_forward queue mode (include/cndp_mqcnet.h): the node on
the calling thread (cndp_fwd_node_host, cndp_amd/csrc/fwd.c) against the Python
restatement over mbufs (tests/mq_ip4fwd_ref.py) -- bursts with tails, the group
rules, every l2_len, unaligned frames, frames across the readable end, members
that are not taken -- the header's constants and that it compiles as C and C++,
the twin's argument checks, the checksum step against the reference's recorded
results (tests/golden/ip4_fwd_cksum_ref.npz), and fwd.c's node under the
address / undefined-behaviour sanitizers in a stand-alone program.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.fwd import node_host
from cndp_amd.mbuf import FRAME

import fwd_ref as R
import mq_ip4fwd_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["region_end", "buf_len"])


@pytest.fixture(scope="module")
def std():
    w = R.standard_world()
    arp, rt4, tbl = R.make_tables(w)
    yield w, tbl
    R.close_tables(arp, rt4, tbl)


@FORMS
def test_burst_sizes(std, zero_copy):
    w, tbl = std
    pool = M.make_pool(sum(M.BURST_SIZES))
    M.fill_random(pool, 3, data_offs=(214, 215, 216, 217))
    want = M.expect(pool, w, tbl, M.split(list(range(pool.n)), M.BURST_SIZES), zero_copy)
    assert all(want["stats"]) and sum(want["stats"]) == pool.n


@FORMS
def test_group_rules(std, zero_copy):
    w, tbl = std
    pool = M.make_pool(40)
    bursts = M.fill_groups(pool)
    want = M.expect(pool, w, tbl, bursts, zero_copy)
    assert want["edges"].tolist() == [e for g in M.GROUP_EDGES for e in g]
    # the quirk on the wire: lane 2 of C's first group carries gateway 0's MAC as d_addr
    i = bursts[2][2]
    f = want["mem"][i * FRAME + 64 + 192:][:12]
    assert bytes(f[:6]) == w.arp[1][1] and bytes(f[6:]) == w.netif[4]


@FORMS
def test_l2_len_and_alignment(std, zero_copy):
    w, tbl = std
    pool = M.make_pool(80)
    n = M.fill_l2(pool)
    before = pool.mem.copy()
    want = M.expect(pool, w, tbl, M.split(list(range(n)), [16, 7, n - 23]), zero_copy)
    assert all(want["stats"])
    hdr = want["mem"].reshape(pool.n, FRAME)[:, :64].view(pool.hdr.dtype)[:, 0]
    for i in range(n):
        l2, doff = int(pool.hdr["tx_offload"][i]) & 0x7F, int(pool.hdr["data_off"][i])
        o = i * FRAME + 64 + doff
        if l2 > doff:       # no adjust, no MAC byte: only the TTL / checksum bytes moved
            assert (int(hdr["data_off"][i]), int(hdr["data_len"][i])) == (doff, 46)
            keep = np.ones(FRAME, bool)
            keep[[64 + doff + 8, 64 + doff + 10, 64 + doff + 11]] = False
            assert np.array_equal(want["mem"][i * FRAME:(i + 1) * FRAME][keep], before[i * FRAME:(i + 1) * FRAME][keep])
        else:
            assert (int(hdr["data_off"][i]), int(hdr["data_len"][i])) == (doff - l2, 46 + l2)
        if l2 == 0 and want["edges"][i] != 1:       # the MACs lie over header bytes 0-11 and win
            nif = (int(want["edges"][i]) & N.CNDP_MQ_EDGE_FWD_MASK) - 2
            assert bytes(want["mem"][o + 6:o + 12]) == w.mac(nif)


@FORMS
def test_readable_end(zero_copy):
    """The last mbuf's frame across the readable end: x bytes of the header readable."""
    w = R.standard_world()
    w.arp[7] = (3, bytes([2, 0xEE, 0, 0, 0, 7]))     # 0.0.0.0, what an unreadable destination reads as
    w.arp_fib.add(0, 32, 7)
    arp, rt4, tbl = R.make_tables(w)
    try:
        for x, l2 in ((1, 14), (5, 0), (9, 2), (11, 0), (12, 14), (17, 14), (19, 18), (20, 22)):
            pool = M.make_pool(8)
            for i in range(8):
                M.put(pool, i, M.D if i % 2 else M.G1, l2=l2)
            if zero_copy:
                M.put(pool, 7, M.D, l2=l2, data_off=FRAME - 64 - x)
            else:
                pool.hdr["buf_len"][7] = int(pool.hdr["data_off"][7]) + x
            want = M.expect(pool, w, tbl, [[0, 1, 2], [4, 5, 6, 7]], zero_copy)
            assert want["edges"][6] != M.EDGE_NONE
    finally:
        R.close_tables(arp, rt4, tbl)


def test_members_not_taken(std):
    """NULL entries and mbufs at or past readable_end keep their group position."""
    w, tbl = std
    pool = M.make_pool(12)
    for i, d in enumerate([M.G1, M.G2, M.G4, M.G6, M.G1, M.G2, M.G4, M.G6, M.D, M.G1, M.G2, M.G4]):
        M.put(pool, i, d)
    # lane 1 missing: the rest as before; lane 0 missing: lanes 1-3 take their own gateway's ha
    want = M.expect(pool, w, tbl, [[0, None, 2, 3], [None, 5, 6, 7], [8, 9, None, 11]], True)
    G = M.GATEWAY
    assert want["edges"].tolist() == [4 | G, 0xFFFF, 6 | G, 2 | G, 0xFFFF, 5 | G, 6 | G, 2 | G, 3, 1, 0xFFFF, 1]
    assert bytes(want["mem"][2 * FRAME + 256:][:6]) == w.arp[1][1]       # lane 0's gateway entry
    assert bytes(want["mem"][6 * FRAME + 256:][:6]) == w.arp[14][1]      # its own
    # readable_end in front of the last two mbufs: they are not taken
    mem = pool.mem.copy()
    ptrs = pool.ptrs(np.arange(8, 12))
    e = node_host(tbl, ptrs, 4, readable_end=pool.base + 10 * FRAME)
    assert e.tolist() == [3, 1, 0xFFFF, 0xFFFF]                         # still a group of four: D's hit keeps G1 off its route
    assert np.array_equal(pool.mem[10 * FRAME:], mem[10 * FRAME:])


def test_abi_constants_and_header():
    txt = open(os.path.join(ROOT, "include", "cndp_mqcnet.h")).read()
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define (CNDP_MQ_\w+) (0x[0-9A-Fa-f]+u?|\d+u?)\b", txt)}
    assert defs == {"CNDP_MQ_IP4_FORWARD": 7, "CNDP_MQ_EDGE_FWD_GATEWAY": 0x0400, "CNDP_MQ_EDGE_FWD_MASK": 0x01FF,
                    "CNDP_MQ_STAT_FWD_DIRECT": 8, "CNDP_MQ_STAT_FWD_GATEWAY": 9, "CNDP_MQ_STAT_FWD_ARP_REQUEST": 10}
    for k, v in defs.items():
        assert getattr(N, k) == v, k
    # the edge bits stay clear of the node's edges (netif_idx + 2 <= 257) and of EDGE_NONE
    assert N.CNDP_MQ_EDGE_FWD_MASK >= 255 + 2 and not N.CNDP_MQ_EDGE_FWD_GATEWAY & N.CNDP_MQ_EDGE_FWD_MASK
    assert (N.CNDP_MQ_EDGE_FWD_GATEWAY | N.CNDP_MQ_EDGE_FWD_MASK) < N.CNDP_MQ_EDGE_NONE
    mqfwd = open(os.path.join(ROOT, "include", "cndp_mqfwd.h")).read()
    taken = {int(v) for v in re.findall(r"#define CNDP_MQ_STAT_\w+ (\d+)", mqfwd)} | {1, 2}
    assert not taken & {8, 9, 10}
    names = N.l4_exported_symbols("cndp_mqcnet.h")
    assert set(names) == {"cndp_gpu_mq_create_ip4_forward", "cndp_fwd_node_host"}
    L = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert hasattr(L, nm), nm
    assert set(names) <= set(N.exported_symbols())
    for cc, std_ in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        r = subprocess.run([cc, std_, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c" if cc == "gcc" else "c++",
                            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "cndp_mqcnet.h")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_argument_checks(std):
    w, tbl = std
    L = N.lib()
    pool = M.make_pool(4)
    for i in range(4):
        M.put(pool, i, M.D)
    mem = pool.mem.copy()
    ptrs = pool.ptrs(np.arange(4))
    edges = np.zeros(300, np.uint16)
    assert L.cndp_fwd_node_host(None, ptrs, 4, edges.ctypes.data, None) == -22
    assert L.cndp_fwd_node_host(tbl.h, None, 4, edges.ctypes.data, None) == -22
    assert L.cndp_fwd_node_host(tbl.h, ptrs, 4, None, None) == -22
    many = (ctypes.c_void_p * 257)(*[pool.addr(0)] * 257)
    assert L.cndp_fwd_node_host(tbl.h, many, 257, edges.ctypes.data, None) == -22
    assert np.array_equal(pool.mem, mem)                                    # a refused call touches nothing
    assert L.cndp_fwd_node_host(tbl.h, None, 0, None, None) == 0            # an empty burst is no error
    # the queue's create calls refuse what they cannot run before they touch a device
    assert L.cndp_gpu_mq_create_ip4_forward(None, None, None, None) == -22
    c, h = N.MqConf(), ctypes.c_void_p()
    c.mode = N.CNDP_MQ_IP4_FORWARD
    assert L.cndp_gpu_mq_create_ip4_forward(None, ctypes.byref(c), tbl.h, ctypes.byref(h)) == -22


def test_cksum_pinned_by_reference_golden(std):
    """The twin's TTL / checksum bytes for every recorded (ttl, checksum) pair."""
    w, tbl = std
    g = np.load(os.path.join(HERE, "golden", "ip4_fwd_cksum_ref.npz"))
    ttl, ck, to, co = (g[k].astype(np.int64) for k in ("ttl", "cksum", "ttl_out", "cksum_out"))
    pick = np.unique(np.concatenate([np.arange(0, len(ttl), 5), np.arange(len(ttl) - 21, len(ttl))]))
    pool = M.make_pool(256)
    for lo in range(0, len(pick), 256):
        idx = pick[lo:lo + 256]
        for k, j in enumerate(idx):
            M.put(pool, k, M.D, ttl=int(ttl[j]), ck=int(ck[j]))
        e = node_host(tbl, pool.ptrs(np.arange(len(idx))), len(idx))
        assert (e == 3).all()
        at = np.arange(len(idx)) * FRAME + 64 + 206
        assert np.array_equal(pool.mem[at + 8], to[idx]), lo
        assert np.array_equal(pool.mem[at + 10].astype(np.int64) | pool.mem[at + 11].astype(np.int64) << 8, co[idx]), lo


def test_node_under_sanitizers():
    """tests/mq_ip4fwd_host/node_san: fwd.c's node (over fib.c / rib.c) built with
    -fsanitize=address,undefined in a program of its own, run as a child process."""
    d = os.path.join(HERE, "mq_ip4fwd_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "node_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "-fsanitize=address,undefined" in open(os.path.join(d, "Makefile")).read()

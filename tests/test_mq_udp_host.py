"""Host side of the udp_input queue mode (include/cndp_mql4.h): the two nodes
on the calling thread (cndp_udp_input_node_host, cndp_amd/csrc/pcb.c) against the
Python restatement over mbufs (tests/mq_udp_ref.py) for every fill the GPU tests
use -- lookup classes, flags, checksums of every length and alignment, clipped
frames, pktmbuf_adj_offset refusing, metadata hooks, mbufs that are not taken --
the header's constants and that it compiles as C and C++, the argument checks,
the PCB user values, the checksum step against the reference's recorded results
(tests/golden/udp_cksum_ref.npz), and pcb.c's twin under the address /
undefined-behaviour sanitizers in a stand-alone program.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.l4 import PcbTable, udp_input_node_host
from cndp_amd.mbuf import FRAME

import mq_udp_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["region_end", "stage_max"])


@pytest.fixture(scope="module")
def std():
    w = M.standard_world()
    yield w
    w.close()


@FORMS
def test_mixed_bursts(std, zero_copy):
    pool = M.make_pool(600)
    M.fill_mix(pool)
    want = M.expect(pool, std, M.split(list(range(600)), [1, 63, 64, 65, 256, 151]), zero_copy)
    assert all(want["stats"][k] for k in (M.RECV, M.NOMATCH, M.CKSUM, M.PDROP)) and sum(want["stats"]) == 600


@FORMS
@pytest.mark.parametrize("punt,tcp", [(True, False), (False, False), (True, True), (False, True)])
def test_lookup_classes(zero_copy, punt, tcp):
    w = M.standard_world()
    try:
        w.set_flags(punt, tcp)
        pool = M.make_pool(64)
        n = M.fill_lookup(pool)
        want = M.expect(pool, w, [list(range(n))], zero_copy)
        e = want["edges"][:21].tolist()
        miss = M.UDP_PUNT if punt else M.UDP_DROP
        pt = M.PROTO_TCP if tcp else M.PROTO_DROP
        assert e == [M.UDP_RECV] * 6 + [miss, M.UDP_RECV, miss, M.UDP_RECV, M.UDP_RECV, M.UDP_RECV, miss, miss,
                     M.UDP_RECV, M.UDP_DROP | M.CK, M.UDP_RECV, M.PROTO_DROP, pt, M.PROTO_DROP, pt]
        hdr = want["mem"].reshape(pool.n, FRAME)[:, :64].view(pool.hdr.dtype)[:, 0]
        got = [int(hdr["udata64"][i]) for i in (0, 1, 2, 3, 4, 5, 7, 9, 10, 11, 14, 16)]
        assert got == [0, w.users[1], w.users[2], 3, w.users[1], 4, 5, 7, 8, 9, w.users[10], w.users[10]]
        assert int(hdr["udata64"][6]) == 0 and int(hdr["udata64"][15]) == 0xABABABABABABABAB   # NULL; left alone
        assert int(hdr["udata64"][17]) == 0xABABABABABABABAB
        st = want["stats"]
        assert st[M.RECV] and st[M.NOMATCH] and st[M.CKSUM] and st[M.PDROP] and bool(st[M.TCP]) == tcp and not st[M.NOMD]
    finally:
        w.close()


@FORMS
def test_checksum_lengths_and_alignments(std, zero_copy):
    pool = M.make_pool(512)
    n, sp = M.fill_cksum(pool)
    want = M.expect(pool, std, M.split(list(range(n)), [256, n - 256]), zero_copy)
    half = sp // 2
    assert (want["edges"][:half] == M.UDP_RECV).all() and (want["edges"][half:sp] == (M.UDP_DROP | M.CK)).all()
    e = want["edges"][sp:sp + 9].tolist()
    assert e[0] == M.UDP_RECV and e[1] == M.UDP_RECV and e[2] == M.UDP_RECV        # field 0; sums of 0xFFFF
    assert e[3] == M.UDP_DROP | M.CK and e[4] == M.UDP_DROP | M.CK and e[5] == M.UDP_DROP | M.CK
    assert e[7] == M.UDP_RECV and e[8] == M.UDP_DROP | M.CK


def test_stage_max_clips(std):
    """Staged, stage_max = 128: a 256-byte datagram is summed over its first 128 bytes."""
    pool = M.make_pool(512)
    n, sp = M.fill_cksum(pool)
    full = M.expect(pool, std, [list(range(sp, n))], False)
    clip = M.expect(pool, std, [list(range(sp, n))], False, stage_max=128)
    assert full["edges"][7] == M.UDP_RECV and clip["edges"][7] == M.UDP_DROP | M.CK
    assert (clip["edges"][[0, 1, 3]] == full["edges"][[0, 1, 3]]).all()


def test_region_end(std):
    """Zero-copy: the pool's last mbuf with its datagram ending exactly at the region's end, and reaching past it."""
    for over, ck in ((0, "good"), (0, "last"), (2, "good"), (40, "good")):
        pool = M.make_pool(4)
        for i in range(4):
            M.put(pool, i, dport=5002, dgram=100, cksum=ck)
        M.put(pool, 3, dport=5002, dgram=100, l3=24, data_off=FRAME - 64 - 124 + over, cksum=ck)
        pool.hdr["buf_len"][3] = 4000                       # the buffer is no bound here: the region is
        want = M.expect(pool, std, [[0, 1], [2, 3]], True)
        assert want["edges"][3] == (M.UDP_RECV if over == 0 and ck == "good" else M.UDP_DROP | M.CK)


@FORMS
def test_waves_of_verifies(std, zero_copy):
    pool = M.make_pool(320)
    n = M.fill_waves(pool)
    want = M.expect(pool, std, M.split(list(range(n)), [256, 64]), zero_copy)
    assert want["stats"][M.CKSUM] == 2 + 2 + 21 and want["stats"][M.RECV] == 320 - 25


@FORMS
def test_adj_offset_refuses(std, zero_copy):
    pool = M.make_pool(8)
    n = M.fill_adj(pool)
    want = M.expect(pool, std, [list(range(n))], zero_copy)
    assert (want["edges"] == M.UDP_RECV).all()
    hdr = want["mem"].reshape(pool.n, FRAME)[:, :64].view(pool.hdr.dtype)[:, 0]
    assert [(int(hdr["data_off"][i]), int(hdr["data_len"][i])) for i in range(n)] == \
        [(220, 18), (192, 120), (192, 27), (192, 60), (220, 32), (220, 0)]


@FORMS
def test_metadata_hooks(std, zero_copy):
    pool = M.make_pool(48)
    M.fill_mix(pool, seed=9)
    before = pool.mem.copy()
    M.expect(pool, std, [list(range(48))], zero_copy)
    M.expect(pool, std, [list(range(48))], zero_copy, md_delta=128)
    want = M.expect(pool, std, [list(range(20)), list(range(20, 48))], zero_copy, md_delta=128, md_null=lambda i: i % 3 == 0)
    assert want["stats"][M.NOMD] and want["stats"][M.RECV]
    for i in range(0, 48, 3):
        assert np.array_equal(want["mem"][i * FRAME:(i + 1) * FRAME], before[i * FRAME:(i + 1) * FRAME])
        assert want["edges"][i] in (M.UDP_DROP, M.PROTO_DROP)


def test_members_not_taken(std):
    pool = M.make_pool(6)
    for i in range(6):
        M.put(pool, i, dport=5000)
    want = M.expect(pool, std, [[0, None, 2], [None, 4, 5]], True)
    assert want["edges"].tolist() == [M.UDP_RECV, 0xFFFF, M.UDP_RECV, 0xFFFF, M.UDP_RECV, M.UDP_RECV]
    mem = pool.mem.copy()
    e = udp_input_node_host(std.tbl, pool.ptrs(np.arange(3, 6)), 3, readable_end=pool.base + 4 * FRAME + 63)
    assert e.tolist() == [M.UDP_RECV, 0xFFFF, 0xFFFF]        # mbuf 4's header ends past the end
    assert np.array_equal(pool.mem[4 * FRAME:], mem[4 * FRAME:])
    e = udp_input_node_host(std.tbl, pool.ptrs(np.arange(4, 6)), 2, readable_end=pool.base + 4 * FRAME + 64 + 192)
    assert e.tolist() == [0xFFFF, 0xFFFF]                    # mbuf 4's frame begins at the end
    assert np.array_equal(pool.mem[4 * FRAME:], mem[4 * FRAME:])


def test_abi_constants_and_header():
    txt = open(os.path.join(ROOT, "include", "cndp_mql4.h")).read()
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define (CNDP_MQ_\w+) (0x[0-9A-Fa-f]+u?|\d+u?)\b", txt)}
    assert defs == {"CNDP_MQ_UDP_INPUT": 8, "CNDP_MQ_NODE_IP4_PROTO": 3, "CNDP_MQ_NODE_UDP_INPUT": 4,
                    "CNDP_MQ_EDGE_L4_CKSUM": 0x0080, "CNDP_MQ_EDGE_L4_MASK": 0xFF7F, "CNDP_MQ_STAT_L4_RECV": 11,
                    "CNDP_MQ_STAT_L4_NOMATCH": 12, "CNDP_MQ_STAT_L4_CKSUM": 13, "CNDP_MQ_STAT_L4_PROTO_DROP": 14,
                    "CNDP_MQ_STAT_L4_TCP": 15, "CNDP_MQ_STAT_L4_NOMD": 16}
    for k, v in defs.items():
        assert getattr(N, k) == v, k
    assert (M.PROTO_DROP, M.PROTO_TCP, M.UDP_DROP, M.UDP_RECV, M.UDP_PUNT) == (0x0300, 0x0302, 0x0400, 0x0401, 0x0402)
    assert (M.UDP_DROP | M.CK) & N.CNDP_MQ_EDGE_L4_MASK == M.UDP_DROP and (M.UDP_DROP | M.CK) != N.CNDP_MQ_EDGE_NONE
    taken = set()
    for h in ("cndp_gpu.h", "cndp_mqfwd.h", "cndp_mqcnet.h"):
        taken |= {int(v) for v in re.findall(r"#define CNDP_MQ_STAT_\w+ (\d+)", open(os.path.join(ROOT, "include", h)).read())}
    assert not taken & set(range(11, 17))
    names = N.l4_exported_symbols("cndp_mql4.h")
    assert set(names) == {"cndp_gpu_mq_create_udp_input", "cndp_udp_input_node_host", "cndp_pcb_user_set",
                          "cndp_pcb_user_get"}
    L = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert hasattr(L, nm), nm
    assert set(names) <= set(N.exported_symbols())
    for cc, std_ in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        r = subprocess.run([cc, std_, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c" if cc == "gcc" else "c++",
                            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "cndp_mql4.h")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_argument_checks(std):
    L = N.lib()
    pool = M.make_pool(4)
    for i in range(4):
        M.put(pool, i)
    mem = pool.mem.copy()
    ptrs = pool.ptrs(np.arange(4))
    edges = np.zeros(300, np.uint16)
    assert L.cndp_udp_input_node_host(None, ptrs, 4, edges.ctypes.data, None, 0, None) == -22
    assert L.cndp_udp_input_node_host(std.tbl.h, None, 4, edges.ctypes.data, None, 0, None) == -22
    assert L.cndp_udp_input_node_host(std.tbl.h, ptrs, 4, None, None, 0, None) == -22
    many = (ctypes.c_void_p * 257)(*[pool.addr(0)] * 257)
    assert L.cndp_udp_input_node_host(std.tbl.h, many, 257, edges.ctypes.data, None, 0, None) == -22
    assert np.array_equal(pool.mem, mem)                                    # a refused call touches nothing
    assert L.cndp_udp_input_node_host(std.tbl.h, None, 0, None, None, 0, None) == 0   # an empty burst is no error
    # the queue's create call refuses what it cannot run before it touches a device
    assert L.cndp_gpu_mq_create_udp_input(None, None, None, None) == -22
    c, h = N.MqConf(), ctypes.c_void_p()
    c.mode = N.CNDP_MQ_UDP_INPUT
    assert L.cndp_gpu_mq_create_udp_input(None, ctypes.byref(c), std.tbl.h, ctypes.byref(h)) == -22


def test_user_values():
    t = PcbTable(8)
    try:
        L = N.lib()
        a, b = t.add(lport=5000), t.add(lport=5001)
        assert (t.user_get(a), t.user_get(b)) == (0, 1)                     # the default is the index
        assert t.user_set(b, 0xFFFF800012345678) == 0 and t.user_get(b) == 0xFFFF800012345678
        assert t.user_get(a) == 0
        assert t.delete(b) == 0 and t.user_get(b) == 1                      # reset by delete
        v = ctypes.c_uint64()
        assert t.user_set(2, 5) == -22 and L.cndp_pcb_user_get(t.h, 2, ctypes.byref(v)) == -22   # outside the vector
        assert L.cndp_pcb_user_set(None, 0, 1) == -22 and L.cndp_pcb_user_get(None, 0, ctypes.byref(v)) == -22
        assert L.cndp_pcb_user_get(t.h, 0, None) == -22
        # not part of the image: a lookup answers as before
        from cndp_amd.l4 import make_keys, port_net
        assert t.user_set(a, 77) == 0
        assert t.lookup(make_keys(0, port_net(5000), 0, 0))[0] == a
    finally:
        t.close()


def test_cksum_pinned_by_reference_golden():
    """The twin's verdict for every recorded datagram with a nonzero checksum field."""
    g = np.load(os.path.join(HERE, "golden", "udp_cksum_ref.npz"))
    off, verify, l3s = g["off"], g["verify"], g["l3_len"]
    pick = []
    for i in range(len(verify)):
        s, l3 = g["data"][off[i]:off[i + 1]], int(l3s[i])
        if s[9] == 17 and len(s) >= l3 + 8 and (s[l3 + 6] or s[l3 + 7]):
            pick.append(i)
    assert len(pick) >= 200 and {int(verify[i]) for i in pick} == {-1, 0}
    t = PcbTable(len(pick))
    try:
        ports = set()
        pool = M.make_pool(len(pick))
        for k, i in enumerate(pick):
            s, l3 = g["data"][off[i]:off[i + 1]], int(l3s[i])
            lport = int(s[l3 + 2]) | int(s[l3 + 3]) << 8
            if lport not in ports:
                ports.add(lport)
                assert t.add_raw(0, 0, lport, 0, N.CNDP_UDP_CHKSUM_FLAG) >= 0
            doff = 192 + k % 16
            o = k * FRAME + 64 + doff
            pool.mem[o:o + len(s)] = s
            pool.hdr["data_off"][k], pool.hdr["data_len"][k] = doff, len(s)
            pool.hdr["tx_offload"][k] = 14 | l3 << 7 | 8 << 16
        for lo in range(0, len(pick), 256):
            idx = np.arange(lo, min(lo + 256, len(pick)))
            e = udp_input_node_host(t, pool.ptrs(idx), len(idx))
            want = [M.UDP_RECV if verify[pick[k]] == 0 else M.UDP_DROP | M.CK for k in idx]
            assert e.tolist() == want, [str(g["kind"][pick[k]]) for k in idx if e[k - lo] != want[k - lo]][:5]
    finally:
        t.close()


def test_node_under_sanitizers():
    """tests/mq_udp_host/node_san: pcb.c's twin built with
    -fsanitize=address,undefined in a program of its own, run as a child process."""
    d = os.path.join(HERE, "mq_udp_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "node_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "-fsanitize=address,undefined" in open(os.path.join(d, "Makefile")).read()

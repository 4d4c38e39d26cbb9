"""Host side of the tcp_input queue mode (include/cndp_mqtcp.h): the node on
the calling thread (cndp_tcp_input_node_host, cndp_amd/csrc/pcb.c) against the
Python restatement over mbufs (tests/mq_tcp_ref.py) for every fill the GPU tests
use -- lookup classes, the punt flag, checksums of every length and alignment,
clipped frames, every header step of cnet_tcp_input's opening, metadata hooks,
mbufs that are not taken -- the header's constants and that it compiles as C and
C++, the argument checks, the checksum step against the reference's recorded
results (tests/golden/tcp_cksum_ref.npz), and pcb.c's twin under the address /
undefined-behaviour sanitizers in a stand-alone program.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.l4 import PcbTable, tcp_input_node_host
from cndp_amd.mbuf import FRAME

import mq_tcp_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["region_end", "stage_max"])
UNTOUCHED = 0xABABABABABABABAB


@pytest.fixture(scope="module")
def std():
    w = M.standard_world()
    yield w
    w.close()


def hdr_of(want, pool):
    return want["mem"].reshape(pool.n, FRAME)[:, :64].view(pool.hdr.dtype)[:, 0]


@FORMS
def test_mixed_bursts(std, zero_copy):
    pool = M.make_pool(600)
    M.fill_mix(pool)
    want = M.expect(pool, std, M.split(list(range(600)), [1, 63, 64, 65, 256, 151]), zero_copy)
    st = want["stats"]
    assert all(st[k] > 0 for k in (M.SEGMENT, M.NOMATCH, M.CKSUM, M.ADJUST, M.SHORT, M.BADOFF, M.OPT)) and sum(st) == 600
    assert st[M.NOMD] == 0
    seg = want["edges"] == M.TCP_SEG
    assert (want["segs"]["offset"][seg] >= 20).all() and not want["segs"][want["edges"] == M.TCP_DROP].view(np.uint8).any()


@FORMS
@pytest.mark.parametrize("punt", [True, False])
def test_lookup_classes(zero_copy, punt):
    w = M.standard_world()
    try:
        w.set_flags(punt, False)
        pool = M.make_pool(64)
        n = M.fill_lookup(pool)
        want = M.expect(pool, w, [list(range(n))], zero_copy)
        miss = M.TCP_PUNT if punt else M.TCP_DROP
        S = M.TCP_SEG
        assert want["edges"][:11].tolist() == [S, S, S, S, S, S, S, S, miss, miss, S]
        hdr = hdr_of(want, pool)
        C = M.NCONN
        got = [int(hdr["udata64"][i]) for i in range(11)]
        assert got == [w.users[2], w.users[5], C + 1, w.users[1], w.users[1], 0, C + 3, w.users[C + 4],
                       UNTOUCHED, UNTOUCHED, C + 2]                  # no match: userptr is not written
        assert w.users[2] != 2 and w.users[C + 4] != C + 4             # cndp_pcb_user_set's values travel
        assert want["stats"][M.SEGMENT] > 0 and want["stats"][M.NOMATCH] > 0
    finally:
        w.close()


@FORMS
def test_table_of_4096(zero_copy):
    w = M.big_world()
    try:
        pool = M.make_pool(256)
        M.fill_big(pool)
        want = M.expect(pool, w, [list(range(256))], zero_copy)
        assert want["stats"][M.SEGMENT] > 0 and want["stats"][M.NOMATCH] > 0
        users = set(int(x) for x in hdr_of(want, pool)["udata64"])
        assert 0x7F00DEAD0000 in users and 1 in users and len(users) > 200   # the last entry; a deleted one's listener
    finally:
        w.close()


@FORMS
def test_checksum_lengths_and_alignments(std, zero_copy):
    pool = M.make_pool(512)
    n, sp = M.fill_cksum(pool)
    want = M.expect(pool, std, M.split(list(range(n)), [256, n - 256]), zero_copy)
    half = sp // 2
    assert half == len(M.SEG_LENS) * 8
    assert (want["edges"][:half] == M.TCP_SEG).all() and (want["edges"][half:sp] == (M.TCP_DROP | M.CK)).all()
    bad, ok = M.TCP_DROP | M.CK, M.TCP_SEG
    for rep in range(4):
        e = want["edges"][sp + 12 * rep:sp + 12 * rep + 12].tolist()
        assert e == [bad, ok, ok, ok, bad, bad, bad, bad, bad, ok, bad, ok], (rep, e)
    assert want["stats"][M.CKSUM] > 0 and want["stats"][M.SEGMENT] > 0


def test_stage_max_clips(std):
    """Staged, stage_max = 128: a 256-byte segment is summed over its first 108 bytes."""
    pool = M.make_pool(512)
    n, sp = M.fill_cksum(pool)
    full = M.expect(pool, std, [list(range(sp, n))], False)
    clip = M.expect(pool, std, [list(range(sp, n))], False, stage_max=128)
    assert full["edges"][9] == M.TCP_SEG and clip["edges"][9] == M.TCP_DROP | M.CK
    assert (clip["edges"][[0, 1, 3, 4]] == full["edges"][[0, 1, 3, 4]]).all()
    assert clip["stats"][M.CKSUM] > full["stats"][M.CKSUM] > 0


def test_region_end(std):
    """Zero-copy: the pool's last mbuf with its segment ending exactly at the region's end, and reaching past it."""
    for over, ck in ((0, "good"), (0, "last"), (2, "good"), (40, "good")):
        pool = M.make_pool(4)
        for i in range(4):
            M.put(pool, i, seglen=100, cksum=ck)
        M.put(pool, 3, seglen=100, data_off=FRAME - 64 - 120 + over, cksum=ck)
        pool.hdr["buf_len"][3] = 4000                       # the buffer is no bound here: the region is
        want = M.expect(pool, std, [[0, 1], [2, 3]], True)
        assert want["edges"][3] == (M.TCP_SEG if over == 0 and ck == "good" else M.TCP_DROP | M.CK)
        assert want["stats"][M.SEGMENT if ck == "good" else M.CKSUM] > 0


@FORMS
def test_waves_of_hits_and_misses(std, zero_copy):
    pool = M.make_pool(320)
    n = M.fill_waves(pool)
    want = M.expect(pool, std, M.split(list(range(n)), [256, 64]), zero_copy)
    st = want["stats"]
    assert st[M.CKSUM] == 2 + 2 + 21 and st[M.SEGMENT] == 74 - 25 and st[M.NOMATCH] == 320 - 74


@FORMS
def test_header_steps(std, zero_copy):
    pool = M.make_pool(16)
    n = M.fill_steps(pool)
    before = pool.mem.copy()
    want = M.expect(pool, std, [list(range(n))], zero_copy)
    S, D, O = M.TCP_SEG, M.TCP_DROP, M.TCP_SEG | M.IPOPT
    assert want["edges"].tolist() == [O, O, D, D, D, S, D, S, S, D, S, S, S, S]
    st = want["stats"]
    assert (st[M.OPT], st[M.ADJUST], st[M.SHORT], st[M.BADOFF], st[M.SEGMENT]) == (2, 2, 1, 2, 7)
    hdr = hdr_of(want, pool)
    got = [(int(hdr["data_off"][i]), int(hdr["data_len"][i])) for i in range(n)]
    assert got == [(192, 64), (192, 64), (192, 19), (192, 60), (212, 19), (232, 0), (228, 24), (272, 0), (212, 40),
                   (212, 24), (232, 1), (232, 0), (232, 0), (212, 20)]
    sg = want["segs"]
    assert sg["offset"].tolist() == [20, 0, 0, 0, 0, 20, 0, 60, 60, 0, 20, 20, 20, 24]
    assert sg["len"].tolist() == [20, 0, 0, 0, 0, 0, 0, 0, 0xFFEC, 0, 2, 1, 2, 0xFFFC]
    assert sg["flags"][[10, 11, 12]].tolist() == [0x02, 0x11, 0x03]
    assert not sg[1].tobytes().strip(b"\0")
    # IPOPT: step 5 is done (userptr, the metadata), the header is as it stood
    assert int(hdr["udata64"][0]) == std.users[2] and int(hdr["udata64"][2]) == M.NCONN + 2
    b_hdr = before.reshape(pool.n, FRAME)[:, :64].view(pool.hdr.dtype)[:, 0]
    assert (hdr["data_off"][:2] == b_hdr["data_off"][:2]).all() and (hdr["data_len"][:2] == b_hdr["data_len"][:2]).all()
    # no frame byte is ever written
    assert np.array_equal(want["mem"].reshape(pool.n, FRAME)[:, 128:], before.reshape(pool.n, FRAME)[:, 128:])


@FORMS
def test_metadata_hooks(std, zero_copy):
    pool = M.make_pool(48)
    M.fill_mix(pool, seed=9)
    before = pool.mem.copy()
    M.expect(pool, std, [list(range(48))], zero_copy)
    M.expect(pool, std, [list(range(48))], zero_copy, md_delta=128)
    want = M.expect(pool, std, [list(range(20)), list(range(20, 48))], zero_copy, md_delta=128,
                    md_null=lambda i: i % 3 == 0)
    assert want["stats"][M.NOMD] == 16 and want["stats"][M.SEGMENT] > 0
    for i in range(0, 48, 3):
        assert np.array_equal(want["mem"][i * FRAME:(i + 1) * FRAME], before[i * FRAME:(i + 1) * FRAME])
        assert want["edges"][i] == M.TCP_DROP and not want["segs"][i].tobytes().strip(b"\0")


def test_members_not_taken(std):
    pool = M.make_pool(6)
    for i in range(6):
        M.put(pool, i)
    want = M.expect(pool, std, [[0, None, 2], [None, 4, 5]], True)
    assert want["edges"].tolist() == [M.TCP_SEG, 0xFFFF, M.TCP_SEG, 0xFFFF, M.TCP_SEG, M.TCP_SEG]
    assert want["stats"][M.SEGMENT] == 4 and sum(want["stats"]) == 4
    mem = pool.mem.copy()
    e, s = tcp_input_node_host(std.tbl, pool.ptrs(np.arange(3, 6)), 3, readable_end=pool.base + 4 * FRAME + 63)
    assert e.tolist() == [M.TCP_SEG, 0xFFFF, 0xFFFF]         # mbuf 4's header ends past the end
    assert s["offset"].tolist() == [20, 0, 0]
    assert np.array_equal(pool.mem[4 * FRAME:], mem[4 * FRAME:])
    e, s = tcp_input_node_host(std.tbl, pool.ptrs(np.arange(4, 6)), 2, readable_end=pool.base + 4 * FRAME + 64 + 192)
    assert e.tolist() == [0xFFFF, 0xFFFF]                    # mbuf 4's frame begins at the end
    assert np.array_equal(pool.mem[4 * FRAME:], mem[4 * FRAME:])


def test_abi_constants_and_header():
    txt = open(os.path.join(ROOT, "include", "cndp_mqtcp.h")).read()
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define (CNDP_MQ_\w+) (0x[0-9A-Fa-f]+u?|\d+u?)\b", txt)}
    assert defs == {"CNDP_MQ_TCP_INPUT": 9, "CNDP_MQ_NODE_TCP_INPUT": 5, "CNDP_MQ_EDGE_TCP_IPOPT": 0x0040,
                    "CNDP_MQ_EDGE_TCP_MASK": 0xFF3F, "CNDP_MQ_STAT_TCP_SEGMENT": 17, "CNDP_MQ_STAT_TCP_NOMATCH": 18,
                    "CNDP_MQ_STAT_TCP_CKSUM": 19, "CNDP_MQ_STAT_TCP_NOMD": 20, "CNDP_MQ_STAT_TCP_ADJUST": 21,
                    "CNDP_MQ_STAT_TCP_SHORT": 22, "CNDP_MQ_STAT_TCP_BADOFF": 23, "CNDP_MQ_STAT_TCP_IPOPT": 24}
    for k, v in defs.items():
        assert getattr(N, k) == v, k
    assert '#include "cndp_mql4.h"' in txt and '#include "cndp_tcp.h"' in txt
    assert (M.TCP_DROP, M.TCP_SEG, M.TCP_PUNT) == tuple(N.CNDP_MQ_EDGE(N.CNDP_MQ_NODE_TCP_INPUT, e) for e in
                                                        (N.CNDP_TCP_INPUT_PKT_DROP, N.CNDP_TCP_INPUT_SEGMENT,
                                                         N.CNDP_TCP_INPUT_PKT_PUNT))
    assert M.CK == N.CNDP_MQ_EDGE_L4_CKSUM and M.IPOPT == N.CNDP_MQ_EDGE_TCP_IPOPT
    assert (M.TCP_DROP | M.CK) & N.CNDP_MQ_EDGE_TCP_MASK == M.TCP_DROP
    assert (M.TCP_SEG | M.IPOPT) & N.CNDP_MQ_EDGE_TCP_MASK == M.TCP_SEG and (M.TCP_SEG | M.IPOPT) != N.CNDP_MQ_EDGE_NONE
    taken = set()
    for h in ("cndp_gpu.h", "cndp_mqfwd.h", "cndp_mqcnet.h", "cndp_mql4.h"):
        taken |= {int(v) for v in re.findall(r"#define CNDP_MQ_STAT_\w+ (\d+)", open(os.path.join(ROOT, "include", h)).read())}
    assert taken and not taken & set(range(17, 25))
    names = N.l4_exported_symbols("cndp_mqtcp.h")
    assert set(names) == {"cndp_gpu_mq_create_tcp_input", "cndp_gpu_mq_poll_tcp", "cndp_tcp_input_node_host"}
    L = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert hasattr(L, nm), nm
    assert set(names) <= set(N.exported_symbols())
    assert M.SEG_DT.itemsize == 16
    for cc, std_ in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        r = subprocess.run([cc, std_, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c" if cc == "gcc" else "c++",
                            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "cndp_mqtcp.h")],
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
    segs = np.zeros(300, M.SEG_DT)
    assert L.cndp_tcp_input_node_host(None, ptrs, 4, edges.ctypes.data, segs.ctypes.data, None, 0, None) == -22
    assert L.cndp_tcp_input_node_host(std.tbl.h, None, 4, edges.ctypes.data, segs.ctypes.data, None, 0, None) == -22
    assert L.cndp_tcp_input_node_host(std.tbl.h, ptrs, 4, None, segs.ctypes.data, None, 0, None) == -22
    many = (ctypes.c_void_p * 257)(*[pool.addr(0)] * 257)
    assert L.cndp_tcp_input_node_host(std.tbl.h, many, 257, edges.ctypes.data, segs.ctypes.data, None, 0, None) == -22
    assert np.array_equal(pool.mem, mem)                                    # a refused call touches nothing
    assert L.cndp_tcp_input_node_host(std.tbl.h, None, 0, None, None, None, 0, None) == 0   # an empty burst is no error
    # segs may be NULL: the same edges and edits
    twin = pool.mem.copy()
    assert L.cndp_tcp_input_node_host(std.tbl.h, ptrs, 4, edges.ctypes.data, None, None, 0, None) == 0
    assert edges[:4].tolist() == [M.TCP_SEG] * 4 and not np.array_equal(pool.mem, twin)
    # the queue's calls refuse what they cannot run before they touch a device
    assert L.cndp_gpu_mq_create_tcp_input(None, None, None, None) == -22
    c, h = N.MqConf(), ctypes.c_void_p()
    c.mode = N.CNDP_MQ_TCP_INPUT
    assert L.cndp_gpu_mq_create_tcp_input(None, ctypes.byref(c), std.tbl.h, ctypes.byref(h)) == -22
    assert L.cndp_gpu_mq_poll_tcp(None, None, None, None, 0) == -22


def test_cksum_pinned_by_reference_golden():
    """The twin's verdict for every recorded string long enough to carry the ports."""
    g = np.load(os.path.join(HERE, "golden", "tcp_cksum_ref.npz"))
    off, verify, l3s = g["off"], g["verify"], g["l3_len"]
    pick = [i for i in range(len(verify)) if off[i + 1] - off[i] >= int(l3s[i]) + 4 and off[i + 1] - off[i] <= 1800]
    assert len(pick) >= 300 and {int(verify[i]) for i in pick} == {-1, 0}
    t = PcbTable(len(pick))
    try:
        ports = set()
        pool = M.make_pool(len(pick))
        for k, i in enumerate(pick):
            s, l3 = g["data"][off[i]:off[i + 1]], int(l3s[i])
            lport = int(s[l3 + 2]) | int(s[l3 + 3]) << 8
            if lport not in ports:
                ports.add(lport)
                assert t.add_raw(0, 0, lport, 0, 0) >= 0
            doff = 192 + k % 16
            o = k * FRAME + 64 + doff
            pool.mem[o:o + len(s)] = s
            pool.hdr["data_off"][k], pool.hdr["data_len"][k] = doff, len(s)
            pool.hdr["tx_offload"][k] = 14 | l3 << 7 | 20 << 16
        bad = M.TCP_DROP | M.CK
        for lo in range(0, len(pick), 256):
            idx = np.arange(lo, min(lo + 256, len(pick)))
            e, _ = tcp_input_node_host(t, pool.ptrs(idx), len(idx))
            for k in idx:
                if verify[pick[k]] == 0:
                    assert e[k - lo] != bad and (e[k - lo] >> 8) == 5, str(g["kind"][pick[k]])
                else:
                    assert e[k - lo] == bad, str(g["kind"][pick[k]])
    finally:
        t.close()


def test_node_under_sanitizers():
    """tests/mq_tcp_host/node_san: pcb.c's twin built with
    -fsanitize=address,undefined in a program of its own, run as a child process."""
    d = os.path.join(HERE, "mq_tcp_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "node_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "-fsanitize=address,undefined" in open(os.path.join(d, "Makefile")).read()

"""Host side of the ip4_output queue mode (include/cndp_mqtx.h): udp_output +
ip4_output on the calling thread (cndp_ip4_output_node_host, cndp_amd/csrc/tx.c)
against the Python restatement over mbufs (tests/mq_tx_ref.py) for every fill
the GPU tests use -- both tx_modes, every stopping point of the rule, headrooms
0-50, every payload length at every alignment of mtod, a checksum that computes
to 0, counters that wrap, metadata hooks, userptr values that name no PCB,
clipped payloads -- the header's constants and that it compiles as C and C++,
the argument checks, and tx.c's twin under the address / undefined-behaviour
sanitizers in a stand-alone program.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.mbuf import FRAME, HDR

import mq_tx_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["region_end", "stage_max"])
MODES = pytest.mark.parametrize("mode", [M.TX_UDP, M.TX_IP4], ids=["udp", "ip4"])


@pytest.fixture(scope="module")
def std():
    w = M.standard_world()
    yield w
    w.close()


def hdr_of(want, pool):
    return want["mem"].reshape(pool.n, FRAME)[:, :64].view(pool.hdr.dtype)[:, 0]


def own(e):
    return e & N.CNDP_MQ_EDGE_TX_MASK


@MODES
@FORMS
def test_mixed_bursts(std, mode, zero_copy):
    pool = M.make_pool(600)
    M.fill_mix(pool, std, mode)
    want = M.expect(pool, std, M.split(list(range(600)), [1, 63, 64, 65, 256, 151]), mode, zero_copy)
    st = want["stats"]
    assert all(st[k] > 0 for k in (M.SENT, M.ARP, M.HEADROOM, M.NOROUTE, M.PROTO, M.CKSUM)) and st[M.NOMD] == 0
    none = int((want["edges"] == M.EDGE_NONE).sum())
    assert none > 0 and sum(st[:6]) + none == 600
    # every netif of the world sent, and a counter that started at 0xFFF0 wrapped
    nifs = {int(own(e)) - 2 for e in want["edges"] if e != M.EDGE_NONE and own(e) >= 2}
    assert nifs == {0, 1, 2, 3, 4}
    assert any(want["ident1"][k] < want["ident0"][k] for k in nifs)
    # userptr is never written
    assert np.array_equal(hdr_of(want, pool)["udata64"], pool.hdr["udata64"])


@MODES
def test_headrooms(std, mode):
    pool = M.make_pool(256)
    n = M.fill_headrooms(pool, std, mode)
    want = M.expect(pool, std, [list(range(n))], mode, True)
    e, hdr = want["edges"], hdr_of(want, pool)
    need = 42 if mode == M.TX_UDP else 34
    for H in range(51):
        routed, unrouted, tcp, proto1 = (int(x) for x in e[4 * H:4 * H + 4])
        assert (own(routed) != 0) == (H >= need), (H, hex(routed))
        if H < need:
            assert routed == unrouted == tcp == proto1 == M.drop(M.HEADROOM_C) or H >= need - 14
        else:
            assert unrouted == M.drop(M.NOROUTE_C) and proto1 == M.drop(M.PROTO_C) and tcp & M.CKBIT
        # how far each got shows in data_off
        got = H - int(hdr["data_off"][4 * H])
        assert got == (0 if H < need - 34 else need - 34 if H < need - 14 else need - 14 if H < need else need)
        assert H - int(hdr["data_off"][4 * H + 1]) == (got if H < need - 14 else need - 14)     # no route: the IP header stays
        txo = int(hdr["tx_offload"][4 * H])
        if mode == M.TX_UDP:
            assert txo == (0 if H < 8 else 20 << 7 if H < 28 else 20 << 7 | 14)
        else:
            assert txo == (M.TXO0 if H < 20 else M.TXO0 & ~0x7F | 14)    # l3_len was 20 already; the other bits stay
    assert all(want["stats"][k] > 0 for k in (M.SENT, M.ARP, M.HEADROOM, M.NOROUTE, M.PROTO, M.CKSUM))


@MODES
@FORMS
def test_payload_lengths_and_alignments(std, mode, zero_copy):
    pool = M.make_pool(256)
    n = M.fill_lens(pool, std, mode)
    assert n == len(M.PAYLOADS) * 16
    want = M.expect(pool, std, [list(range(n))], mode, zero_copy)
    assert want["stats"][M.CKSUM] == n and (want["edges"] & M.CKBIT).all()
    if mode == M.TX_UDP:                                     # every UDP datagram verifies at the receiver
        import tx_ref as T
        k = 0
        for i in range(n):
            o = i * FRAME + HDR + int(hdr_of(want, pool)["data_off"][i])
            fr = want["mem"][o:o + int(hdr_of(want, pool)["data_len"][i])]
            ip = bytes(fr[14:34])
            assert T.raw_cksum(ip) == 0xFFFF
            if ip[9] == 17:
                psd = ip[12:20] + bytes([0, 17]) + bytes(fr[38:40])
                c = T.raw_cksum(bytes(fr[34:])) + T.raw_cksum(psd)
                assert ((c >> 16) + (c & 0xFFFF)) & 0xFFFF == 0xFFFF, i
                k += 1
        assert k > n // 2


def test_checksum_that_computes_to_zero(std):
    pool = M.make_pool(4)
    for i, ln in enumerate((2, 18, 333, 17)):
        M.craft_zero(pool, std, i, 1, length=ln, data_off=192 + i)
    want = M.expect(pool, std, [list(range(4))], M.TX_UDP, True)
    for i in range(4):
        o = i * FRAME + HDR + 192 + i
        assert bytes(want["mem"][o - 2:o]) == b"\xff\xff" and want["edges"][i] & M.CKBIT


def test_counter_wraps(std):
    """One netif, frames of 0x2E00-byte steps: the counter crosses 0xFFFF several times in one burst."""
    pool = M.make_pool(64)
    for i in range(64):
        M.put(pool, std, i, 0, length=18, data_off=192)      # total_length 46: the counter moves by 0x2E00
    want = M.expect(pool, std, [list(range(64))], M.TX_UDP, True)
    nif = int(own(want["edges"][0])) - 2
    assert want["ident1"][nif] == (want["ident0"][nif] + 64 * 0x2E00) & 0xFFFF
    ids = [int.from_bytes(bytes(want["mem"][i * FRAME + HDR + 150 + 18:i * FRAME + HDR + 150 + 20]), "big") for i in range(64)]
    assert ids == [(want["ident0"][nif] + k * 0x2E00) & 0xFFFF for k in range(64)]


@MODES
@FORMS
@pytest.mark.parametrize("hook", ["offset", "null"])
def test_metadata_hooks(std, mode, zero_copy, hook):
    pool = M.make_pool(64)
    for i in range(64):
        M.put(pool, std, i, M.ROUTED[i % len(M.ROUTED)], length=20 + i, md_at=1024 if hook == "offset" else 64)
    kw = {"md_delta": 1024} if hook == "offset" else {"md_null": lambda i: i % 3 == 0}
    want = M.expect(pool, std, [list(range(64))], mode, zero_copy, **kw)
    if hook == "null":
        assert want["stats"][M.NOMD] == 22 and (want["edges"][::3] == M.drop(M.NOMD_C)).all()
        rows = want["mem"].reshape(64, FRAME)[::3]
        assert np.array_equal(rows, pool.mem.reshape(64, FRAME)[::3])          # nothing written
    else:
        assert want["stats"][M.NOMD] == 0 and want["stats"][M.SENT] + want["stats"][M.ARP] == 64


@MODES
def test_userptr_values_that_name_no_pcb(std, mode):
    pool = M.make_pool(8)
    n_pcb = len(std.tw.pcbs)
    ups = [1 << 32, (1 << 32) | 1, n_pcb, n_pcb + 1000, 0xFFFFFFFF, M.PCB_DEAD, (1 << 63) | 2, 1]
    for i, up in enumerate(ups):
        M.put(pool, std, i, 1, userptr=up)
    want = M.expect(pool, std, [list(range(8))], mode, True)
    assert (want["edges"][:7] == M.EDGE_NONE).all() and own(want["edges"][7]) != 0
    assert np.array_equal(want["mem"][:7 * FRAME], pool.mem[:7 * FRAME]) and sum(want["stats"][:6]) == 1


def test_clips(std):
    """A 333-byte payload summed over its first 64 bytes (stage_max), a payload that
    the buffer cuts, and one that the region's end cuts; a checksum field past the
    clip is not written."""
    pool = M.make_pool(4)
    M.put(pool, std, 0, 1, length=333)
    M.put(pool, std, 1, 1, length=100, data_off=1984 - 10)                   # the buffer holds 10 bytes of it
    M.put(pool, std, 2, M.PCB_TCP, length=100, data_off=1984 - 12)           # TCP field at +16: past the buffer
    M.put(pool, std, 3, 1, length=400, data_off=1984 - 100)
    full = M.expect(pool, std, [[0, 1, 2]], M.TX_IP4, False)
    M.rewind(std, full)
    clip = M.expect(pool, std, [[0, 1, 2]], M.TX_IP4, False, stage_max=64)
    o = HDR + 192
    assert bytes(full["mem"][o + 6:o + 8]) != bytes(clip["mem"][o + 6:o + 8])
    assert np.array_equal(full["mem"][FRAME:], clip["mem"][FRAME:])
    assert (full["edges"][:3] & M.CKBIT).all()
    assert np.array_equal(full["mem"][3 * FRAME - 12:3 * FRAME], pool.mem[3 * FRAME - 12:3 * FRAME])
    pool.hdr["buf_len"][3] = 4000                                            # the buffer claims to pass the region's end
    end = M.expect(pool, std, [[3]], M.TX_UDP, True)
    pool.hdr["buf_len"][3] = 1984
    M.rewind(std, end)
    buf = M.expect(pool, std, [[3]], M.TX_UDP, True)
    assert np.array_equal(end["mem"][3 * FRAME + 64:], buf["mem"][3 * FRAME + 64:]) and end["edges"][0] & M.CKBIT
    assert end["mem"][3 * FRAME + 28] == 4000 & 0xFF


def test_header_and_exports():
    text = open(os.path.join(ROOT, "include", "cndp_mqtx.h")).read()
    assert int(re.search(r"#define CNDP_MQ_IP4_OUTPUT (\d+)u", text).group(1)) == N.CNDP_MQ_IP4_OUTPUT == 10
    keys = [int(v) for v in re.findall(r"#define CNDP_MQ_STAT_TX_\w+ (\d+)", text)]
    assert keys == list(range(25, 32)) == [N.CNDP_MQ_STAT_TX_SENT, N.CNDP_MQ_STAT_TX_ARP_REQUEST,
                                           N.CNDP_MQ_STAT_TX_DROP_NOMD, N.CNDP_MQ_STAT_TX_DROP_HEADROOM,
                                           N.CNDP_MQ_STAT_TX_DROP_NOROUTE, N.CNDP_MQ_STAT_TX_DROP_PROTO,
                                           N.CNDP_MQ_STAT_TX_CKSUM]
    taken = set()
    for h in ("cndp_gpu.h", "cndp_mqfwd.h", "cndp_mqcnet.h", "cndp_mql4.h", "cndp_mqtcp.h"):
        taken |= {int(v) for v in re.findall(r"#define CNDP_MQ_STAT_\w+ (\d+)", open(os.path.join(ROOT, "include", h)).read())}
    assert taken and not taken & set(keys)
    L = ctypes.CDLL(N.LIB_PATH)
    names = N.l4_exported_symbols("cndp_mqtx.h")
    assert set(names) == {"cndp_gpu_mq_create_ip4_output", "cndp_ip4_output_node_host"}
    for nm in names:
        assert hasattr(L, nm), nm
    assert set(names) <= set(N.exported_symbols())
    for cc, std_ in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        r = subprocess.run([cc, std_, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c" if cc == "gcc" else "c++",
                            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "cndp_mqtx.h")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_argument_checks(std):
    L = N.lib()
    pool = M.make_pool(4)
    for i in range(4):
        M.put(pool, std, i, 1)
    mem = pool.mem.copy()
    ptrs = pool.ptrs(np.arange(4))
    edges = np.zeros(300, np.uint16)
    f, p, e = std.fwd.h, std.pt.h, edges.ctypes.data
    assert L.cndp_ip4_output_node_host(None, p, 0, ptrs, 4, e, None, 0, None) == -22
    assert L.cndp_ip4_output_node_host(f, None, 0, ptrs, 4, e, None, 0, None) == -22
    assert L.cndp_ip4_output_node_host(f, p, 2, ptrs, 4, e, None, 0, None) == -22
    assert L.cndp_ip4_output_node_host(f, p, 0, None, 4, e, None, 0, None) == -22
    assert L.cndp_ip4_output_node_host(f, p, 0, ptrs, 4, None, None, 0, None) == -22
    many = (ctypes.c_void_p * 257)(*[pool.addr(0)] * 257)
    assert L.cndp_ip4_output_node_host(f, p, 0, many, 257, e, None, 0, None) == -22
    assert np.array_equal(pool.mem, mem)                                    # a refused call touches nothing
    assert L.cndp_ip4_output_node_host(f, p, 0, None, 0, None, None, 0, None) == 0   # an empty burst is no error
    # the queue's create call refuses what it cannot run before it touches a device
    assert L.cndp_gpu_mq_create_ip4_output(None, None, None, None, 0, None) == -22
    c, h = N.MqConf(), ctypes.c_void_p()
    c.mode = N.CNDP_MQ_IP4_OUTPUT
    assert L.cndp_gpu_mq_create_ip4_output(None, ctypes.byref(c), f, p, 0, ctypes.byref(h)) == -22


def test_node_under_sanitizers():
    """tests/mq_tx_host/node_san: tx.c's twin built with
    -fsanitize=address,undefined in a program of its own, run as a child process."""
    d = os.path.join(HERE, "mq_tx_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "node_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "-fsanitize=address,undefined" in open(os.path.join(d, "Makefile")).read()

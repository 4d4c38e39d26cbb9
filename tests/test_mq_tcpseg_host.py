"""Host side of the tcp_segment queue mode (include/cndp_mqtcb.h): the node on
the calling thread (cndp_tcp_segment_node_host, cndp_amd/csrc/tcb.c) against the
Python reference (tests/mq_tcpseg_ref.py: tests/mq_tcp_ref.py's node and
tests/tcpseg_ref.py's segment rule composed, FIRST over an explicit batch) --
lookup classes and punt, checksums, the header steps, the metadata hooks, option
bytes at the readable edge, every verdict, FIRST behind dropped mbufs, the sum
rule of the counters' keys, the recorded reference vectors pushed through mbufs,
random segments, the header's constants, the argument checks, and tcb.c's twin
under the address / undefined-behaviour sanitizers in a stand-alone program.
No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.l4 import PcbTable, TcbTable
from cndp_amd.mbuf import FRAME

import mq_tcp_ref as M
import mq_tcpseg_ref as T
import tcp_golden as TG
import tcpseg_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMS = pytest.mark.parametrize("zero_copy", [True, False], ids=["region_end", "stage_max"])


@pytest.fixture(scope="module")
def std():
    tw = T.standard_tworld()
    yield tw
    tw.close()


def first_of(want):
    return [k for k in range(len(want["verdicts"])) if want["verdicts"][k] & S.FIRST]


@FORMS
def test_mixed_batches(std, zero_copy):
    pool = M.make_pool(600)
    T.fill_mix(pool, std)
    want = T.expect(pool, std, M.split(list(range(600)), [1, 63, 64, 65, 256, 151]), zero_copy, now=T.NOW)
    st, ts = want["stats"], want["tstats"]
    assert all(st[k] > 0 for k in (M.SEGMENT, M.NOMATCH, M.CKSUM, M.ADJUST, M.SHORT, M.BADOFF, M.OPT)) and sum(st) == 600
    assert all(x > 0 for x in ts), ts
    v = want["verdicts"]
    judged = (v & S.VMASK) != 0
    assert not want["opts"][~judged].view(np.uint8).any()
    assert ((want["edges"][judged] & N.CNDP_MQ_EDGE_TCP_MASK) == M.TCP_SEG).all()
    assert (v[judged] & S.FIRST).any() and not (v[judged] & S.FIRST).all()


@FORMS
@pytest.mark.parametrize("punt", [True, False])
def test_lookup_classes_and_punt(zero_copy, punt):
    tw = T.standard_tworld()
    try:
        tw.w.set_flags(punt, False)
        pool = M.make_pool(64)
        n = M.fill_lookup(pool)
        want = T.expect(pool, tw, [list(range(n))], zero_copy)
        miss = M.TCP_PUNT if punt else M.TCP_DROP
        assert want["edges"][:11].tolist() == [M.TCP_SEG] * 8 + [miss, miss, M.TCP_SEG]
        V = want["verdicts"][:11] & S.VMASK
        # connections 2 (TCB), 5 (none), NCONN + 1 (none / closed), the listeners (LISTEN: SLOW), no TCB behind them
        assert V[0] == S.SLOW and V[1] == S.RESET and V[3] == S.SLOW and V[5] == S.SLOW and V[6] == S.RESET
        assert V[8] == V[9] == S.NONE and want["verdicts"][0] & S.FIRST
        assert not want["verdicts"][11] & S.FIRST                   # the same connection again, later in the batch
    finally:
        tw.close()


@FORMS
def test_checksum_cases(std, zero_copy):
    pool = M.make_pool(512)
    n, sp = M.fill_cksum(pool)
    want = T.expect(pool, std, M.split(list(range(n)), [128, n - 128]), zero_copy)
    half = sp // 2
    assert ((want["verdicts"][:half] & S.VMASK) != 0).all() and (want["verdicts"][half:sp] == 0).all()
    f = first_of(want)                                              # one connection: one FIRST a batch, on its
    assert len(f) == 2 and f[0] == 0 and f[1] >= sp and not want["verdicts"][128:f[1]].any()   # first survivor
    assert want["stats"][M.CKSUM] > 0 and sum(want["tstats"]) == want["stats"][M.SEGMENT]


@FORMS
def test_header_steps(std, zero_copy):
    """NOMD / ADJUST / SHORT / BADOFF / IPOPT / zeroed IPOPT: only survivors are judged."""
    pool = M.make_pool(16)
    n = M.fill_steps(pool)
    want = T.expect(pool, std, [list(range(n))], zero_copy)
    S_, D, O = M.TCP_SEG, M.TCP_DROP, M.TCP_SEG | M.IPOPT
    assert want["edges"].tolist() == [O, O, D, D, D, S_, D, S_, S_, D, S_, S_, S_, S_]
    judged = [int(v & S.VMASK) != 0 for v in want["verdicts"]]
    assert judged == [True, False, False, False, False, True, False, True, True, False, True, True, True, True]
    assert want["verdicts"][0] & S.FIRST and not any(want["verdicts"][k] & S.FIRST for k in range(1, n))
    assert sum(want["tstats"]) == want["stats"][M.SEGMENT] + want["stats"][M.OPT] - 1
    assert not want["opts"][1].tobytes().strip(b"\0")
    want = T.expect(pool, std, [list(range(n))], zero_copy, md_null=lambda i: i in (0, 5))
    assert want["stats"][M.NOMD] == 2 and first_of(want) == [7]     # FIRST moves to the first survivor


@FORMS
def test_metadata_hooks(std, zero_copy):
    pool = M.make_pool(48)
    T.fill_mix(pool, std, seed=9)
    T.expect(pool, std, [list(range(48))], zero_copy, now=T.NOW)
    T.expect(pool, std, [list(range(48))], zero_copy, now=T.NOW, md_delta=128)
    want = T.expect(pool, std, [list(range(20)), list(range(20, 48))], zero_copy, now=T.NOW, md_delta=128,
                    md_null=lambda i: i % 3 == 0)
    assert want["stats"][M.NOMD] == 16 and sum(want["tstats"]) > 0
    assert not want["verdicts"][0::3].any() and not np.ascontiguousarray(want["opts"][0::3]).view(np.uint8).any()


@pytest.mark.parametrize("how", ["data_len", "stage_max", "region"])
def test_option_bytes_at_the_readable_edge(std, how):
    """data_len, stage_max and readable_end clip the option bytes; what lies behind them reads as zero."""
    for opts, clip, verdict, ts_val in T.EDGE_CASES:
        pool, batches, zc, sm = T.edge_case(std, opts, clip, how)
        want = T.expect(pool, std, batches, zc, now=T.NOW, stage_max=sm)
        assert want["edges"].tolist() == [M.TCP_SEG], (clip, want["edges"])
        assert int(want["verdicts"][0]) == verdict | S.FIRST, (clip, int(want["verdicts"][0]))
        assert int(want["opts"]["ts_val"][0]) == ts_val
    for opts, ihl, clip, verdict, ts_val in T.EDGE_CASES_64:
        pool, batches, zc, sm = T.edge_case(std, opts, clip, how, ihl=ihl)
        want = T.expect(pool, std, batches, zc, now=T.NOW, stage_max=sm)
        assert want["edges"].tolist() == [M.TCP_SEG | (M.IPOPT if ihl != 5 else 0)], (clip, want["edges"])
        assert int(want["verdicts"][0]) == verdict | S.FIRST and int(want["opts"]["ts_val"][0]) == ts_val


@FORMS
def test_every_verdict_and_ts_update(std, zero_copy):
    pool = M.make_pool(16)
    cases = T.verdict_specs(std, 2)
    for i, (spec, _) in enumerate(cases):
        T.put_spec(pool, i, spec, data_off=192 + i)
    n = len(cases)
    T.put_spec(pool, n, dict(pair=T.pair_of(std.w, 5), seq=1, ack=2, wnd=3, flags=S.ACK))        # connection 5: no TCB
    T.put_spec(pool, n + 1, dict(pair=T.pair_of(std.w, 3), seq=1, ack=2, wnd=3, flags=S.ACK))    # connection 3: closed
    assert 5 not in std.tcbs and std.tcbs[3]["state"] == S.CLOSED_STATE
    want = T.expect(pool, std, [list(range(n + 2))], zero_copy, now=T.NOW)
    got = [int(v) & ~S.FIRST for v in want["verdicts"]]
    assert got == [v for _, v in cases] + [S.RESET, S.CLOSED], got
    assert all(x > 0 for x in want["tstats"])
    assert first_of(want) == [0, n, n + 1]
    assert int(want["opts"]["ts_ecr"][3]) == T.NOW - 5 and int(want["opts"]["mss"][6]) == 1460
    later = T.expect(pool, std, [list(range(n + 2))], zero_copy, now=T.NOW - 6)                 # the echo is ahead of now
    assert int(later["opts"]["ts_ecr"][3]) == 0 and int(later["opts"]["ts_val"][3]) == 90


@FORMS
@pytest.mark.parametrize("cause", ["cksum", "nomd", "adjust", "short", "badoff"])
def test_first_behind_dropped_mbufs(std, zero_copy, cause):
    pool = M.make_pool(8)
    t = std.tcbs[2]
    spec = dict(pair=T.pair_of(std.w, 2), seq=t["rcv_nxt"], ack=600, wnd=t["snd_wnd"] >> t["snd_scale"], flags=S.ACK)
    for i in range(8):
        T.put_spec(pool, i, spec)
    null = None
    for i in (0, 1):
        if cause == "cksum":
            T.put_spec(pool, i, dict(spec, bad_cksum=True))
        elif cause == "nomd":
            null = lambda k: k < 2                                  # noqa: E731
        elif cause == "adjust":
            M.put(pool, i, seglen=40, data_len=19, clip=19, fix=12)
        elif cause == "short":
            M.put(pool, i, seglen=20, data_len=39, clip=39)
        else:
            M.put(pool, i, seglen=40, nib=4)
    want = T.expect(pool, std, [list(range(5)), list(range(5, 8))], zero_copy, md_null=null)
    key = dict(cksum=M.CKSUM, nomd=M.NOMD, adjust=M.ADJUST, short=M.SHORT, badoff=M.BADOFF)[cause]
    assert want["stats"][key] == 2
    assert first_of(want) == [2, 5] and not want["verdicts"][:2].any()


def test_reference_vectors_through_mbufs():
    """tests/golden/tcp_options_ref.npz: opt and verdict as test_tcp_reference_golden.py expects them."""
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
                batches = M.split(list(range(len(cases))), [256] * (len(cases) // 256) + [len(cases) % 256])
                e, s, o, v, _ = T.run_twin(pool, tw, [b for b in batches if b], True, now=now)
                assert (e == M.TCP_SEG).all() and ((v & S.FIRST) != 0).all()
                check(G, idx, v, o, f"twin, now {now:#x}")
                if cases_of is TG.parse_cases:
                    seen_p += len(idx)
                else:
                    seen_h += len(idx)
            finally:
                tw.close()
    assert seen_p == len(G["p_tail"]) and seen_h == len(G["h_branch"])


def test_random_segments_and_tcbs():
    rng = np.random.default_rng(20250)
    tw = T.TWorld(M.World(256))
    try:
        pool = M.make_pool(256)
        for i in range(256):
            tcb, spec = S.random_case(rng, T.NOW)
            if i % 2 == 0:                                          # two segments a connection
                c = tw.w.add(laddr=M.LADDR, lport=5000, faddr=M.PEER, fport=2000 + i // 2)
                tw.set(c, tcb)
            T.put_spec(pool, i, dict(spec, pair=T.pair_of(tw.w, c)), data_off=192 + i % 16)
        for zc in (True, False):
            want = T.expect(pool, tw, [list(range(256))], zc, now=T.NOW)
            assert (want["edges"] == M.TCP_SEG).all() and sum(want["tstats"]) == 256
            assert sum(1 for x in want["tstats"] if x) >= 6 and len(first_of(want)) == 128
    finally:
        tw.close()


def test_abi_constants_and_header():
    txt = open(os.path.join(ROOT, "include", "cndp_mqtcb.h")).read()
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define (CNDP_MQ_\w+) (0x[0-9A-Fa-f]+u?|\d+u?)\b", txt)}
    assert defs == {"CNDP_MQ_TCP_SEGMENT": 11, "CNDP_MQ_STAT_TSEG_RESET": 32, "CNDP_MQ_STAT_TSEG_CLOSED": 33,
                    "CNDP_MQ_STAT_TSEG_BADOPT": 34, "CNDP_MQ_STAT_TSEG_SLOW": 35, "CNDP_MQ_STAT_TSEG_PRED_ACK": 36,
                    "CNDP_MQ_STAT_TSEG_PRED_DATA": 37, "CNDP_MQ_STAT_TSEG_PRED_NONE": 38}
    for k, v in defs.items():
        assert getattr(N, k) == v, k
    assert N.CNDP_MQ_STAT_TSEG_RESET + N.CNDP_TCPSEG_PRED_NONE - 1 == N.CNDP_MQ_STAT_TSEG_PRED_NONE
    assert "Defined by this build" in txt and "cnet_tcp.c" in txt
    taken = set()
    for h in ("cndp_gpu.h", "cndp_mqfwd.h", "cndp_mqcnet.h", "cndp_mql4.h", "cndp_mqtcp.h", "cndp_mqtx.h"):
        taken |= {int(v) for v in re.findall(r"#define CNDP_MQ_STAT_\w+ (\d+)", open(os.path.join(ROOT, "include", h)).read())}
    assert taken and not taken & set(range(32, 39))
    names = N.l4_exported_symbols("cndp_mqtcb.h")
    assert set(names) == {"cndp_gpu_mq_create_tcp_segment", "cndp_gpu_mq_tcp_now", "cndp_gpu_mq_poll_tcpseg",
                          "cndp_tcp_segment_node_host"}
    L = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert hasattr(L, nm), nm
    assert set(names) <= set(N.exported_symbols())
    for nm in ("tcb_dev_begin", "tcb_dev_end", "tcb_dev_check", "pcb_tcp_node_walk"):     # internal: not exported
        assert not hasattr(L, nm), nm
    assert T.OPT_DT.itemsize == 16
    for cc, std_ in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        r = subprocess.run([cc, std_, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c" if cc == "gcc" else "c++",
                            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "cndp_mqtcb.h")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_argument_checks(std):
    L = N.lib()
    pool = M.make_pool(4)
    for i in range(4):
        M.put(pool, i)
    mem = pool.mem.copy()
    ptrs = pool.ptrs(np.arange(4))
    e, s = np.zeros(300, np.uint16), np.zeros(300, M.SEG_DT)
    o, v = np.zeros(300, T.OPT_DT), np.zeros(300, np.uint8)
    f = L.cndp_tcp_segment_node_host
    tail = (e.ctypes.data, s.ctypes.data, o.ctypes.data, v.ctypes.data, None, 0, None)
    assert f(None, std.tcb_tbl.h, 0, ptrs, 4, *tail) == -22
    assert f(std.tbl.h, None, 0, ptrs, 4, *tail) == -22
    assert f(std.tbl.h, std.tcb_tbl.h, 0, None, 4, *tail) == -22
    assert f(std.tbl.h, std.tcb_tbl.h, 0, ptrs, 4, None, *tail[1:]) == -22
    many = (ctypes.c_void_p * 257)(*[pool.addr(0)] * 257)
    assert f(std.tbl.h, std.tcb_tbl.h, 0, many, 257, *tail) == -22
    other = PcbTable(8)
    tcb_other = TcbTable(other)
    try:                                                                # a TCB table over another PCB table
        assert f(std.tbl.h, tcb_other.h, 0, ptrs, 4, *tail) == -22
        assert f(other.h, std.tcb_tbl.h, 0, ptrs, 4, *tail) == -22
        c, h = N.MqConf(), ctypes.c_void_p()
        c.mode = N.CNDP_MQ_TCP_SEGMENT
        assert L.cndp_gpu_mq_create_tcp_segment(None, ctypes.byref(c), std.tbl.h, std.tcb_tbl.h, ctypes.byref(h)) == -22
    finally:
        tcb_other.close()
        other.close()
    assert np.array_equal(pool.mem, mem)                                # a refused call touches nothing
    assert f(std.tbl.h, std.tcb_tbl.h, 0, None, 0, None, None, None, None, None, 0, None) == 0
    assert f(std.tbl.h, std.tcb_tbl.h, 0, ptrs, 4, e.ctypes.data, None, None, None, None, 0, None) == 0
    assert e[:4].tolist() == [M.TCP_SEG] * 4 and not np.array_equal(pool.mem, mem)
    assert L.cndp_gpu_mq_create_tcp_segment(None, None, None, None, None) == -22
    assert L.cndp_gpu_mq_poll_tcpseg(None, None, None, None, None, None, 0) == -22
    assert L.cndp_gpu_mq_tcp_now(None, 5) == -22


def test_node_under_sanitizers():
    """tests/mq_tcpseg_host/node_san: tcb.c's twin and the TCB table built with
    -fsanitize=address,undefined in a program of its own, run as a child process."""
    d = os.path.join(HERE, "mq_tcpseg_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "node_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "-fsanitize=address,undefined" in open(os.path.join(d, "Makefile")).read()

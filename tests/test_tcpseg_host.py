"""Host side of the TCP option parse and header-prediction triage
(include/cndp_tcb.h, cndp_amd/csrc/tcb.c): the TCB table's calls and return
codes, and cndp_tcp_segment_host -- the rule the kernel also runs -- against the
Python restatement (tests/tcpseg_ref.py) and against vectors worked out by hand
from the reference's text (lib/cnet/tcp/cnet_tcp.c:1179-1279, :3214-3281,
:3425-3482); 20480 seeded random segments and TCBs; and tcb.c under the address /
undefined-behaviour sanitizers in a stand-alone program.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.l4 import OPT_DT, PcbTable, TcbTable, addr_net, port_net

import l4_ref as R
import tcp_ref as T
import tcpseg_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
NOW = 1_000_000
CAP = 4096
TS, MSS, WS, SACK = S.TS_PRESENT, S.MSS_PRESENT, S.WS_PRESENT, S.SACK_PERMIT
# an established connection: peer window 1024 << 3, 1000 bytes in flight
EST = dict(rcv_nxt=1000, snd_una=5000, snd_nxt=6000, snd_max=6000, snd_wnd=8192, snd_cwnd=10000, ts_recent=500,
           last_ack_sent=900, rcv_space=100, max_mss=1460, state=S.ESTABLISHED, snd_scale=3, flags=1)
LISTEN = dict(S.TCB_ZERO, state=2, max_mss=1460, snd_scale=3, flags=1)
PURE_ACK = dict(seq=1000, ack=5500, wnd=1024, flags=S.ACK)       # PRED_ACK against EST
DATA = dict(seq=1000, ack=5000, wnd=1024, flags=S.ACK | S.PSH)   # + payload: PRED_DATA against EST


@pytest.fixture(scope="module")
def tables():
    """4096 connections and their (empty) TCB table, shared: every test sets the
    TCBs it uses."""
    pcbs = PcbTable(CAP)
    for i in range(CAP):
        assert pcbs.add(laddr=0x0A040001, lport=80, faddr=0xC6120000 + i, fport=40000) == i
    tcbs = TcbTable(pcbs)
    yield pcbs, tcbs
    tcbs.close()
    pcbs.close()


def judge(tcbs, cases, now=NOW, pcb=None, sel=None, layout="offsets", stats=None):
    """cases = [(tcb dict or None, spec)], case i on PCB pcb[i] (default i).  Sets
    the TCBs, runs the host twin and the restatement on the same arrays, requires
    them equal, and returns (verdict, opt, stats)."""
    n = len(cases)
    pcb = np.arange(n, dtype=np.uint32) if pcb is None else np.asarray(pcb, np.uint32)
    image = [None] * CAP
    for p in sorted(set(int(x) for x in pcb if x < CAP)):
        tcbs.clear(p)
    for (t, _), p in zip(cases, pcb):
        if t is not None and p < CAP and image[int(p)] is None:
            tcbs.set(int(p), **t)
            image[int(p)] = t
    b = S.build([c[1] for c in cases], layout=layout)
    sel = np.ones(n, np.uint8) if sel is None else np.asarray(sel, np.uint8)
    kw = dict(sel=sel, stride=b["stride"], offsets=b["offsets"], data_off=b["data_off"], stats=stats)
    got = tcbs.segment_host(b["slab"], n, b["rxmeta"], pcb, b["seg"], now, **kw)
    want = S.tcp_segment_ref(b["slab"], n, b["rxmeta"], image, pcb, b["seg"], now, **kw)
    for k in ("verdict", "opt", "stats"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[0]}: host {got[k][bad[0]]} restatement {want[k][bad[0]]}"
    return got["verdict"], got["opt"], got["stats"]


def one(tcbs, tcb, spec, now=NOW):
    v, o, _ = judge(tcbs, [(tcb, spec)], now)
    assert v[0] & S.FIRST
    return int(v[0]) & ~S.FIRST, tuple(int(x) for x in o[0])


def test_sizes_exports_and_the_frame_builder():
    assert ctypes.sizeof(N.Tcb) == 48 and OPT_DT.itemsize == 16 and S.OPT_DT == OPT_DT
    assert ctypes.sizeof(N.TcpSegIo) == 56
    names = N.l4_exported_symbols("cndp_tcb.h")
    assert set(names) == {"cndp_tcb_tbl_create", "cndp_tcb_tbl_destroy", "cndp_tcb_set", "cndp_tcb_clear",
                          "cndp_tcb_get", "cndp_gpu_tcp_segment", "cndp_tcp_segment_host"}
    L = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert hasattr(L, nm), nm
    assert (S.NONE, S.RESET, S.CLOSED, S.BADOPT, S.SLOW, S.PRED_ACK, S.PRED_DATA, S.PRED_NONE) == (
        N.CNDP_TCPSEG_NONE, N.CNDP_TCPSEG_RESET, N.CNDP_TCPSEG_CLOSED, N.CNDP_TCPSEG_BADOPT, N.CNDP_TCPSEG_SLOW,
        N.CNDP_TCPSEG_PRED_ACK, N.CNDP_TCPSEG_PRED_DATA, N.CNDP_TCPSEG_PRED_NONE)
    assert (S.TS_UPDATE, S.FIRST) == (N.CNDP_TCPSEG_TS_UPDATE, N.CNDP_TCPSEG_FIRST)
    # the builder's frames are what tcp_input accepts, and its seg records are tcp_input's
    specs = [dict(PURE_ACK, opts=bytes([1, 1]) + S.ts_opt(7, 8)), dict(DATA, payload=b"abc"),
             dict(seq=1, ack=0, wnd=9, flags=S.SYN, opts=bytes([2, 4, 5, 180]), urp=3)]
    b = S.build(specs)
    ent = np.array([(addr_net(S.PAIR[0][0]), 0, port_net(S.PAIR[0][1]), 0, 0)], R.ENTRY_DT)
    t = T.tcp_input_ref(b["slab"], 3, b["rxmeta"], ent, sel=np.ones(3, np.uint8), offsets=b["offsets"])
    assert (t["l4edge"] == T.E_SEG).all() and (t["seg"] == b["seg"]).all()


def test_table_calls_and_return_codes():
    L = N.lib()
    pcbs = PcbTable(8)
    h = ctypes.c_void_p()
    assert L.cndp_tcb_tbl_create(None, ctypes.byref(h)) == -22
    assert L.cndp_tcb_tbl_create(pcbs.h, None) == -22
    L.cndp_tcb_tbl_destroy(None)
    tcbs = TcbTable(pcbs)
    try:
        t = N.Tcb()
        assert L.cndp_tcb_set(None, 0, ctypes.byref(t)) == -22 and L.cndp_tcb_get(None, 0, ctypes.byref(t)) == -22
        assert L.cndp_tcb_clear(None, 0) == -22
        assert tcbs.set_raw(0, state=5) == -22                      # no PCB yet: idx >= cndp_pcb_count
        for i in range(3):
            assert pcbs.add(laddr=0x0A040001, lport=80, faddr=0xC6120001, fport=1000 + i) == i
        assert L.cndp_tcb_set(tcbs.h, 0, None) == -22 and L.cndp_tcb_get(tcbs.h, 0, None) == -22
        assert tcbs.set_raw(3, state=5) == -22 and tcbs.clear(3) == -22
        assert tcbs.set_raw(0, state=12) == -22 and tcbs.set_raw(0, state=11) == 0
        assert tcbs.get(1) is None and tcbs.clear(1) == -2          # never set: no TCB
        assert tcbs.set_raw(1, **dict(EST, flags=0xFF)) == 0
        assert tcbs.get(1) == dict(EST, flags=1)                    # only the defined flag is kept
        full = dict(rcv_nxt=0xFFFFFFFF, snd_una=0xFFFFFFFE, snd_nxt=0xFFFFFFFD, snd_max=0xFFFFFFFC,
                    snd_wnd=0xFFFFFFFB, snd_cwnd=0xFFFFFFFA, ts_recent=0xFFFFFFF9, last_ack_sent=0xFFFFFFF8,
                    rcv_space=0xFFFFFFF7, max_mss=0xFFFF, state=0, snd_scale=0xFF, flags=0)
        assert tcbs.set_raw(2, **full) == 0 and tcbs.get(2) == full and tcbs.get(1) == dict(EST, flags=1)
        assert tcbs.clear(2) == 0 and tcbs.get(2) is None and tcbs.clear(2) == -2
        # the segment call's own refusals
        b, io = N.Batch(), N.TcpSegIo()
        assert L.cndp_tcp_segment_host(None, 0, ctypes.byref(b), ctypes.byref(io)) == -22
        assert L.cndp_tcp_segment_host(tcbs.h, 0, None, ctypes.byref(io)) == -22
        assert L.cndp_tcp_segment_host(tcbs.h, 0, ctypes.byref(b), None) == -22
        assert L.cndp_tcp_segment_host(tcbs.h, 0, ctypes.byref(b), ctypes.byref(io)) == 0     # n == 0
        b.n = 1
        assert L.cndp_tcp_segment_host(tcbs.h, 0, ctypes.byref(b), ctypes.byref(io)) == -22   # arrays missing
        assert L.cndp_gpu_tcp_segment(None, None, None, None, 0, None) == -22
    finally:
        tcbs.close()
        pcbs.close()


def test_pcb_delete_takes_the_tcb_and_no_index_inherits_one():
    """cnet_pcb_free zeroes the PCB, its tcb pointer included: after cndp_pcb_del
    the index has no TCB (a segment that still reaches it, on port 0, is answered
    with a RST) and cannot be given one; the PCB added next gets a fresh index
    (an index is never handed out twice, cndp_l4.h) that starts without a TCB."""
    pcbs = PcbTable(4)
    tcbs = TcbTable(pcbs)
    try:
        assert pcbs.add(laddr=0x0A040001, lport=80, faddr=0xC6120001, fport=1) == 0
        assert pcbs.add(laddr=0x0A040001, lport=80, faddr=0xC6120001, fport=2) == 1
        tcbs.set(0, **EST)
        tcbs.set(1, **EST)
        b = S.build([PURE_ACK, PURE_ACK, PURE_ACK])
        run = lambda pcb: tcbs.segment_host(b["slab"], 3, b["rxmeta"], np.array(pcb, np.uint32), b["seg"], NOW,  # noqa: E731
                                            sel=np.ones(3, np.uint8), offsets=b["offsets"])["verdict"].tolist()
        assert run([0, 1, 2]) == [S.PRED_ACK | S.FIRST, S.PRED_ACK | S.FIRST, S.RESET | S.FIRST]
        assert pcbs.delete(1) == 0
        assert tcbs.get(1) is None and tcbs.get(0) == EST
        assert tcbs.set_raw(1, **EST) == -2 and tcbs.clear(1) == -2
        assert pcbs.add(laddr=0x0A040001, lport=80, faddr=0xC6120001, fport=2) == 2     # the same tuple again
        assert tcbs.get(2) is None
        assert run([0, 1, 2]) == [S.PRED_ACK | S.FIRST, S.RESET | S.FIRST, S.RESET | S.FIRST]
        tcbs.set(2, **dict(EST, state=1))
        assert run([2, 1, 0]) == [S.CLOSED | S.FIRST, S.RESET | S.FIRST, S.PRED_ACK | S.FIRST]
    finally:
        tcbs.close()
        pcbs.close()


# ---- tcp_do_options, by hand ------------------------------------------------
def test_syn_options(tables):
    _, tcbs = tables
    syn = dict(seq=77, ack=0x01020304, wnd=0xFFFF, flags=S.SYN)
    o = bytes([2, 4, 0x05, 0xB4, 1, 3, 3, 7, 4, 2]) + S.ts_opt(777, 0x01020304)     # MSS 1460, NOP, WS 7, SACK_OK, TS
    # no ACK: ts_ecr is 0 whatever the bytes say; SYN: the window is not scaled
    assert one(tcbs, LISTEN, dict(syn, opts=o)) == (S.SLOW, (777, 0, 0xFFFF, 1460, TS | MSS | WS | SACK | 7))
    # with ACK the echo is read: 0x01020304 is later than NOW and zeroed, 999 is kept
    assert one(tcbs, LISTEN, dict(syn, flags=S.SYN | S.ACK, opts=o)) == (S.SLOW, (777, 0, 0xFFFF, 1460, TS | MSS | WS | SACK | 7))
    assert one(tcbs, LISTEN, dict(syn, flags=S.SYN | S.ACK, opts=o[:10] + S.ts_opt(777, 999))) == (
        S.SLOW, (777, 999, 0xFFFF, 1460, TS | MSS | WS | SACK | 7))
    big = bytes([2, 4, 0x23, 0x28])                                                  # 9000 > max_mss
    assert one(tcbs, LISTEN, dict(syn, opts=big)) == (S.SLOW, (0, 0, 0xFFFF, 1460, MSS))
    assert one(tcbs, dict(LISTEN, max_mss=9000), dict(syn, opts=big))[1][3] == 9000
    assert one(tcbs, LISTEN, dict(syn, opts=bytes([3, 3, 15, 1])))[1] == (0, 0, 0xFFFF, 0, WS | 14)
    assert one(tcbs, LISTEN, dict(syn, opts=bytes([3, 3, 14, 1])))[1] == (0, 0, 0xFFFF, 0, WS | 14)
    assert one(tcbs, LISTEN, dict(syn, opts=bytes([3, 3, 0, 1])))[1] == (0, 0, 0xFFFF, 0, WS)
    # repeats: the later option overwrites the earlier one
    two = bytes([2, 4, 0x05, 0xB4, 2, 4, 0x02, 0x18, 3, 3, 9, 3, 3, 2, 0, 0])
    assert one(tcbs, LISTEN, dict(syn, opts=two))[1] == (0, 0, 0xFFFF, 536, MSS | WS | 2)
    # MSS and WS on a segment without SYN are walked over; the window is scaled by snd_scale
    o = bytes([2, 4, 0x05, 0xB4, 3, 3, 7, 1])
    assert one(tcbs, EST, dict(PURE_ACK, opts=o)) == (S.PRED_ACK, (0, 0, 8192, 0, 0))
    # lengths other than the option's own: not read, not failed
    assert one(tcbs, LISTEN, dict(syn, opts=bytes([2, 3, 9, 3, 4, 9, 9, 4, 3, 9, 1, 1])))[1] == (0, 0, 0xFFFF, 0, 0)
    assert one(tcbs, LISTEN, dict(syn, opts=bytes([4, 2, 1, 1])))[1] == (0, 0, 0xFFFF, 0, SACK)
    assert one(tcbs, EST, dict(PURE_ACK, opts=bytes([4, 2, 1, 1]))) == (S.PRED_ACK, (0, 0, 8192, 0, SACK))


def test_timestamp_option(tables):
    _, tcbs = tables
    ack = lambda o, **kw: dict(PURE_ACK, opts=o, **kw)  # noqa: E731
    nn = bytes([1, 1])
    assert one(tcbs, EST, ack(nn + S.ts_opt(501, NOW - 3))) == (S.PRED_ACK, (501, NOW - 3, 8192, 0, TS))
    # a length of 8: skipped, not failed -- the walk goes on 8 bytes later
    assert one(tcbs, EST, ack(bytes([8, 8, 0, 0, 3, 9, 1, 1]))) == (S.PRED_ACK, (0, 0, 8192, 0, 0))
    assert one(tcbs, EST, ack(bytes([8, 8, 0, 0, 3, 9, 1, 1, 4, 2, 1, 1])))[1][4] == SACK
    # no ACK flag: ecr is 0, and the entry test fails on the flags
    assert one(tcbs, EST, ack(nn + S.ts_opt(501, NOW - 3), flags=S.PSH)) == (S.SLOW, (501, 0, 8192, 0, TS))
    # ts_ecr later than now: zeroed; equal to now: kept; the comparison is a signed 32-bit difference
    assert one(tcbs, EST, ack(nn + S.ts_opt(501, NOW)))[1][1] == NOW
    assert one(tcbs, EST, ack(nn + S.ts_opt(501, NOW + 1)))[1][1] == 0
    assert one(tcbs, EST, ack(nn + S.ts_opt(501, 0xFFFFFFF0)), now=5)[1][1] == 0xFFFFFFF0       # 21 ticks ago
    assert one(tcbs, EST, ack(nn + S.ts_opt(501, 5)), now=0xFFFFFFF0)[1][1] == 0                # 21 ticks ahead
    assert one(tcbs, EST, ack(nn + S.ts_opt(501, 0x80000000 + NOW)))[1][1] == 0                 # now - ecr = -2^31
    assert one(tcbs, EST, ack(nn + S.ts_opt(501, 0x80000001 + NOW)))[1][1] == 0x80000001 + NOW  # now - ecr = 2^31 - 1
    # two timestamps: the later one stands
    assert one(tcbs, EST, ack(S.ts_opt(600, 1) + S.ts_opt(700, 2)))[1][:2] == (700, 2)


def test_option_bounds_and_malformed_lengths(tables):
    _, tcbs = tables
    ack = lambda o, **kw: dict(PURE_ACK, opts=o, **kw)  # noqa: E731
    bad, zero = S.BADOPT, (0, 0, 0, 0, 0)
    # a known kind whose length runs one past opt_end, and one that ends exactly there
    for kind in (2, 3, 4, 8):
        assert one(tcbs, EST, ack(bytes([1, 1, kind, 3]))) == (bad, zero), kind
        assert one(tcbs, EST, ack(bytes([1, 1, kind, 2])))[0] == S.PRED_ACK, kind
    assert one(tcbs, EST, ack(bytes([1, 1]) + S.ts_opt(501, 1)[:9] + bytes([1]))) == (S.PRED_ACK, (501, 1, 8192, 0, TS))
    assert one(tcbs, EST, ack(bytes([1, 1, 1]) + S.ts_opt(501, 1)[:9])) == (bad, zero)     # 10 bytes, 9 left
    # an unknown kind, SACK (5) included, has no bound test: it walks past the end and the parse is over
    assert one(tcbs, EST, ack(bytes([1, 1, 5, 200])))[0] == S.PRED_ACK
    assert one(tcbs, EST, ack(bytes([99, 255, 0, 0])))[0] == S.PRED_ACK
    # a known kind as the header's last byte: its length is the first payload byte
    d = lambda k, p: dict(DATA, opts=bytes([1, 1, 1, k]), payload=bytes([p]) + b"xyz")  # noqa: E731
    for kind in (2, 3, 4, 8):
        assert one(tcbs, EST, d(kind, 0x00)) == (bad, zero)          # 3 + 0 <= 4, then the zero-length test
        assert one(tcbs, EST, d(kind, 0x02)) == (bad, zero)          # 3 + 2 > 4
        assert one(tcbs, EST, d(kind, 0x01))[0] == S.PRED_DATA       # 3 + 1 <= 4 and opts += 1 ends the walk
    assert one(tcbs, EST, d(5, 0x00)) == (bad, zero)                 # unknown: only the zero-length test
    assert one(tcbs, EST, d(5, 0x02))[0] == S.PRED_DATA
    assert one(tcbs, EST, d(5, 0xFF))[0] == S.PRED_DATA
    # ... and with no payload behind it the byte is the next frame's first, or past the slab: zero
    assert one(tcbs, EST, ack(bytes([1, 1, 1, 4]))) == (bad, zero)
    # zero length
    assert one(tcbs, EST, ack(bytes([99, 0, 1, 1]))) == (bad, zero)
    assert one(tcbs, EST, ack(bytes([1, 4, 0, 1]))) == (bad, zero)
    assert one(tcbs, EST, ack(bytes([4, 2, 77, 0]))) == (bad, zero)  # what was parsed before the failure is not reported
    # a length of 1 re-reads the length byte as a kind
    assert one(tcbs, EST, ack(bytes([99, 1, 4, 2]))) == (S.PRED_ACK, (0, 0, 8192, 0, SACK))     # 1 = NOP
    assert one(tcbs, EST, ack(bytes([4, 1, 4, 2]))) == (S.PRED_ACK, (0, 0, 8192, 0, SACK))
    assert one(tcbs, EST, ack(bytes([99, 1, 1, 1, 99, 1, 0, 0])))[0] == S.PRED_ACK              # ... then EOL
    # EOL ends the parse with success, whatever follows
    assert one(tcbs, EST, ack(bytes([0, 99, 0, 0]))) == (S.PRED_ACK, (0, 0, 8192, 0, 0))
    assert one(tcbs, EST, ack(bytes([4, 2, 0, 8, 77, 0, 0, 0]))) == (S.PRED_ACK, (0, 0, 8192, 0, SACK))
    # NOP skips the zero-length test: 40 of them, then a NOP followed by a zero byte
    v, o = one(tcbs, EST, ack(bytes([1] * 40)))
    assert (v, o) == (S.PRED_ACK, (0, 0, 8192, 0, 0))
    assert one(tcbs, EST, ack(bytes([1] * 36) + S.ts_opt(501, 9)[:4]))[0] == bad                # TS, 10 > 4 left
    assert one(tcbs, EST, ack(bytes([1] * 28) + bytes([1, 1]) + S.ts_opt(501, 9))) == (S.PRED_ACK, (501, 9, 8192, 0, TS))


# ---- the header-prediction tests, by hand ------------------------------------
def test_entry_test_terms(tables):
    _, tcbs = tables
    ts = lambda v: bytes([1, 1]) + S.ts_opt(v, 1)  # noqa: E731
    assert one(tcbs, EST, PURE_ACK)[0] == S.PRED_ACK
    for s in range(12):                                             # every state
        want = {1: S.CLOSED, 5: S.PRED_ACK}.get(s, S.SLOW)
        v, o = one(tcbs, dict(EST, state=s), PURE_ACK)
        assert v == want and o == ((0, 0, 0, 0, 0) if s == 1 else (0, 0, 8192, 0, 0)), s
    v, o = one(tcbs, None, dict(PURE_ACK, opts=ts(501)))            # no TCB: nothing is parsed
    assert (v, o) == (S.RESET, (0, 0, 0, 0, 0))
    assert one(tcbs, dict(EST, state=1), dict(PURE_ACK, opts=bytes([99, 0, 0, 0])))[0] == S.CLOSED
    # flags & HDR_PREDIC == ACK: PSH is outside the mask, every other flag fails it
    for fl, want in ((S.ACK | S.PSH, S.PRED_ACK), (S.ACK | S.FIN, S.SLOW), (S.ACK | S.SYN, S.SLOW), (S.ACK | S.RST, S.SLOW),
                     (S.ACK | S.URG, S.SLOW), (0, S.SLOW), (S.PSH, S.SLOW)):
        # FIN makes seg.len 1, SYN leaves the window unscaled: either way the verdict is SLOW first
        assert one(tcbs, EST, dict(PURE_ACK, flags=fl))[0] == want, fl
    # the timestamp term: ts_val >= ts_recent, signed
    assert one(tcbs, EST, dict(PURE_ACK, opts=ts(500)))[0] == S.PRED_ACK | S.TS_UPDATE      # equal: GEQ and LEQ
    assert one(tcbs, EST, dict(PURE_ACK, opts=ts(501)))[0] == S.PRED_ACK
    assert one(tcbs, EST, dict(PURE_ACK, opts=ts(499)))[0] == S.SLOW
    assert one(tcbs, dict(EST, ts_recent=0xFFFFFFFF), dict(PURE_ACK, opts=ts(0)))[0] == S.PRED_ACK      # 0 is 1 later
    assert one(tcbs, dict(EST, ts_recent=0), dict(PURE_ACK, opts=ts(0xFFFFFFFF)))[0] == S.SLOW
    # the update also needs last_ack_sent < seq
    assert one(tcbs, dict(EST, last_ack_sent=1000), dict(PURE_ACK, opts=ts(500)))[0] == S.PRED_ACK
    assert one(tcbs, dict(EST, last_ack_sent=999), dict(PURE_ACK, opts=ts(500)))[0] == S.PRED_ACK | S.TS_UPDATE
    assert one(tcbs, dict(EST, rcv_nxt=5, last_ack_sent=0xFFFFFFFB), dict(PURE_ACK, seq=5, opts=ts(500)))[0] \
        == S.PRED_ACK | S.TS_UPDATE                                                          # wrapped: 10 below seq
    # seq == rcv_nxt
    assert one(tcbs, EST, dict(PURE_ACK, seq=1001))[0] == S.SLOW
    assert one(tcbs, EST, dict(PURE_ACK, seq=999))[0] == S.SLOW
    assert one(tcbs, dict(EST, rcv_nxt=0xFFFFFFFF, last_ack_sent=0xFFFFFF00), dict(PURE_ACK, seq=0xFFFFFFFF))[0] == S.PRED_ACK
    # the scaled window equals snd_wnd and is not zero
    assert one(tcbs, EST, dict(PURE_ACK, wnd=1023))[0] == S.SLOW
    assert one(tcbs, EST, dict(PURE_ACK, wnd=1025))[0] == S.SLOW
    assert one(tcbs, dict(EST, snd_wnd=0, snd_cwnd=0), dict(PURE_ACK, wnd=0)) == (S.SLOW, (0, 0, 0, 0, 0))
    assert one(tcbs, dict(EST, snd_wnd=1024, snd_scale=0), PURE_ACK) == (S.PRED_ACK, (0, 0, 1024, 0, 0))
    assert one(tcbs, dict(EST, snd_wnd=0xFFFF << 14, snd_scale=14, snd_cwnd=0xFFFFFFFF), dict(PURE_ACK, wnd=0xFFFF)) \
        == (S.PRED_ACK, (0, 0, 0xFFFF << 14, 0, 0))
    # snd_nxt == snd_max
    assert one(tcbs, dict(EST, snd_nxt=5999), PURE_ACK)[0] == S.SLOW


def test_ack_and_data_branches(tables):
    _, tcbs = tables
    A, D, X = S.PRED_ACK, S.PRED_DATA, S.PRED_NONE
    # seqGT(ack, snd_una) && seqLEQ(ack, snd_max) && snd_cwnd >= snd_wnd
    for ack, want in ((5000, X), (5001, A), (6000, A), (6001, X), (4999, X)):
        assert one(tcbs, EST, dict(PURE_ACK, ack=ack))[0] == want, ack
    assert one(tcbs, dict(EST, snd_cwnd=8192), PURE_ACK)[0] == A
    assert one(tcbs, dict(EST, snd_cwnd=8191), PURE_ACK)[0] == X
    # around 2^32: snd_una just below the wrap, snd_max above it
    w = dict(EST, snd_una=0xFFFFFF00, snd_nxt=0x100, snd_max=0x100)
    for ack, want in ((0xFFFFFF00, X), (0xFFFFFF01, A), (0xFFFFFFFF, A), (0, A), (0x100, A), (0x101, X), (0x80000100, X)):
        assert one(tcbs, w, dict(PURE_ACK, ack=ack))[0] == want, hex(ack)
    # data: ack == snd_una, reassembly empty, len <= rcv_space
    pl = lambda k: bytes(range(k))  # noqa: E731
    assert one(tcbs, EST, dict(DATA, payload=pl(1)))[0] == D
    assert one(tcbs, EST, dict(DATA, payload=pl(100)))[0] == D                      # len == rcv_space
    assert one(tcbs, EST, dict(DATA, payload=pl(101)))[0] == X                      # len == rcv_space + 1
    assert one(tcbs, dict(EST, rcv_space=0), dict(DATA, payload=pl(1)))[0] == X
    assert one(tcbs, EST, dict(DATA, ack=5001, payload=pl(10)))[0] == X             # an ACK that also moves snd_una
    assert one(tcbs, dict(EST, flags=0), dict(DATA, payload=pl(10)))[0] == X        # segments waiting in reassembly
    assert one(tcbs, dict(EST, snd_cwnd=0), dict(DATA, payload=pl(10)))[0] == D     # cwnd is the ACK branch's alone
    assert one(tcbs, w, dict(DATA, ack=0xFFFFFF00, payload=pl(10)))[0] == D
    ts = bytes([1, 1]) + S.ts_opt(500, 1)
    assert one(tcbs, EST, dict(DATA, payload=pl(10), opts=ts)) == (D | S.TS_UPDATE, (500, 1, 8192, 0, TS))
    assert one(tcbs, EST, dict(DATA, ack=5001, payload=pl(10), opts=ts))[0] == X | S.TS_UPDATE


def test_selection_first_and_counters(tables):
    _, tcbs = tables
    cases = [(EST, PURE_ACK), (EST, dict(DATA, payload=b"ab")), (EST, dict(PURE_ACK, seq=7)), (None, PURE_ACK),
             (EST, PURE_ACK), (dict(EST, state=1), PURE_ACK), (EST, dict(PURE_ACK, opts=bytes([99, 0, 0, 0]))),
             (EST, PURE_ACK), (EST, PURE_ACK)]
    pcb = [5, 5, 9, 6, 9, 7, 5, N.CNDP_PCB_NONE, CAP]        # PCB 5 three times, 9 twice; two that are no index
    sel = [1, 1, 1, 1, 1, 1, 1, 1, 1]
    v, o, st = judge(tcbs, cases, pcb=pcb, sel=sel, stats=[100, 0, 0, 0, 0, 0, 0, 1])
    F = S.FIRST
    assert v.tolist() == [S.PRED_ACK | F, S.PRED_DATA, S.SLOW | F, S.RESET | F, S.PRED_ACK, S.CLOSED | F, S.BADOPT,
                          S.NONE, S.NONE]
    assert not o[7:].view(np.uint8).any() and not o[3:4].view(np.uint8).any()
    assert st.tolist() == [102, 1, 1, 1, 1, 2, 1, 1]
    sel = [0, 1, 1, 0, 1, 1, 0, 1, 1]
    v, o, st = judge(tcbs, cases, pcb=pcb, sel=sel)
    assert v.tolist() == [S.NONE, S.PRED_DATA | F, S.SLOW | F, S.NONE, S.PRED_ACK, S.CLOSED | F, S.NONE, S.NONE, S.NONE]
    assert not o[[0, 3, 6]].view(np.uint8).any() and st.sum() == 9 and st[0] == 5
    # without sel the SEGMENT edge decides
    b = S.build([c[1] for c in cases])
    edge = np.array([T.E_SEG, T.E_DROP, T.E_SEG, T.E_PUNT, 0xFF, 0x02, T.E_SEG, T.E_SEG, 0x11], np.uint8)
    got = tcbs.segment_host(b["slab"], 9, b["rxmeta"], np.array(pcb, np.uint32), b["seg"], NOW, l4edge=edge,
                            offsets=b["offsets"])
    assert got["verdict"].tolist() == [S.PRED_ACK | F, 0, S.SLOW | F, 0, 0, 0, S.BADOPT, 0, 0]


@pytest.mark.parametrize("layout", ["offsets", "packed", "umem"])
def test_layouts_and_the_slab_end(tables, layout):
    """The same cases in every layout; in "offsets" the slab ends with the last
    frame's last byte, which is a known option kind: its length reads as zero."""
    _, tcbs = tables
    cases = [(EST, dict(PURE_ACK, opts=bytes([1, 1]) + S.ts_opt(500 + i, 3))) for i in range(5)]
    cases += [(EST, dict(DATA, payload=b"q" * 9, opts=bytes([1, 1, 1, 4]))), (EST, dict(PURE_ACK, opts=bytes([1, 1, 1, 8])))]
    v, o, _ = judge(tcbs, cases, layout=layout)
    assert (v[:5] & S.VMASK == S.PRED_ACK).all() and o["ts_val"][:5].tolist() == [500, 501, 502, 503, 504]
    assert v[5] & S.VMASK == S.BADOPT          # 'q' = 0x71: 3 + 113 > 4
    assert v[6] & S.VMASK == S.BADOPT


def test_random_segments_and_tcbs(tables):
    """20480 seeded cases in five batches of 4096, one PCB each except for a tail
    of each batch that shares PCBs with earlier frames.  The mix must reach
    everything: checked on the restatement's own answers (judge() has already
    required the host twin to equal them)."""
    _, tcbs = tables
    rng = np.random.default_rng(20251)
    stats, sflags, upd, nfirst, scales = np.zeros(8, np.int64), 0, 0, 0, set()
    for chunk in range(5):
        now = int(rng.integers(0, 1 << 32))
        cases = [S.random_case(rng, now) for _ in range(CAP)]
        pcb = np.arange(CAP, dtype=np.uint32)
        pcb[-256:] = rng.integers(0, CAP - 256, 256)
        sel = (rng.random(CAP) < 0.98).astype(np.uint8)
        v, o, st = judge(tcbs, cases, now=now, pcb=pcb, sel=sel)
        stats += st.astype(np.int64)
        sflags |= int(np.bitwise_or.reduce(o["sflags"]))
        scales |= set((o["sflags"][(o["sflags"] & WS) != 0] & 0xF).tolist())
        upd += int(((v & S.TS_UPDATE) != 0).sum())
        nfirst += int(((v & S.FIRST) != 0).sum())
        assert (((v & S.TS_UPDATE) == 0) | ((v & S.VMASK) >= S.PRED_ACK)).all()     # TS_UPDATE only with PRED_*
        dup = (v[-256:] & S.VMASK) != 0
        first_of = {}
        for i in np.nonzero(sel)[0]:
            first_of.setdefault(int(pcb[i]), int(i))
        assert ((v[-256:][dup] & S.FIRST) != 0).tolist() == [first_of[int(p)] == CAP - 256 + k
                                                            for k, p in enumerate(pcb[-256:]) if dup[k]]
    total = int(stats.sum())
    assert total == 5 * CAP and (stats > 0).all(), stats
    for k in (S.PRED_ACK, S.PRED_DATA, S.SLOW, S.BADOPT):
        assert stats[k] >= 0.05 * total, (S.NAMES[k], stats)
    assert sflags & 0xF000 == 0xF000 and {0, 7, 14} <= scales
    assert upd > 200 and 0 < nfirst < total - stats[0]


def test_tcb_table_under_sanitizers():
    """tests/tcb_host/tcbseg_san: tcb.c and pcb.c built with
    -fsanitize=address,undefined in a program of its own, run as a child process:
    entries set and cleared across the whole table, and options parsed at the last
    bytes of buffers sized exactly to their frames."""
    d = os.path.join(HERE, "tcb_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "tcbseg_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    flags = open(os.path.join(d, "Makefile")).read()
    assert "-fsanitize=address,undefined" in flags

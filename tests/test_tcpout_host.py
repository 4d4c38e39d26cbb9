"""Host side of the TCP transmit stage (include/cndp_tcpout.h,
cndp_amd/csrc/tcpout.c and the transmit attributes in tcb.c): option bytes worked
out by hand from tcp_send_options (lib/cnet/tcp/cnet_tcp.c:3742-3798), the
tcp_drop_with_reset table (:1120-1149), tcp_do_response's window rule
(:1087-1094), where the header lands, 20480 seeded random cases of
cndp_tcp_output_host against the Python
restatement (tests/tcpout_ref.py) with the whole buffer compared, the calls'
return codes, and tcpout.c under the address / undefined-behaviour sanitizers in
a stand-alone program.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.l4 import TXSEG_DT, PcbTable, TcbTable, send_optlen

import tcpout_ref as R
import tcpseg_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
NOW, TSR = 0x01020304, 0x0A0B0C0D
H = 64


def run(tcbs, conns, pcb, mode=R.SEGMENT, now=NOW, txseg=None, seg=None, verdict=None, rxmeta=None, sel=None,
        snd=None, src_off=None, lay=None, data_off=H, stats=None, prefill=None):
    """The host twin and the restatement over copies of one buffer: the whole
    buffer (guard bytes included), every output and the counters must be equal,
    and the inputs must come back as they went in.  Returns (outputs, buffer)."""
    n = len(pcb)
    if lay is None:
        d = txseg if txseg is not None else np.zeros(n, TXSEG_DT)
        lay = R.layout("packed", R.need_bytes(conns, pcb, d, now, data_off), data_off, seed=n)
    buf, slab_len, stride, offs = lay
    if prefill is not None:
        prefill(buf)
    mine, want_buf = buf.copy(), buf.copy()
    ins = {k: (None if v is None else np.array(v)) for k, v in
           dict(pcb=pcb, txseg=txseg, seg=seg, verdict=verdict, rxmeta=rxmeta, sel=sel, snd=snd, src_off=src_off).items()}
    keep = {k: (None if v is None else v.copy()) for k, v in ins.items()}
    kw = dict(mode=mode, now=now, txseg=ins["txseg"], seg=ins["seg"], verdict=ins["verdict"], rxmeta=ins["rxmeta"],
              sel=ins["sel"], snd=ins["snd"], src_off=ins["src_off"], stride=stride, offsets=offs, data_off=data_off,
              stats=stats)
    got = tcbs.output_host(mine[:slab_len], n, ins["pcb"], **kw)
    want = R.tcp_output_ref(want_buf, slab_len, n, conns, ins["pcb"], **kw)
    for k, v in keep.items():
        assert v is None or np.array_equal(ins[k], v), f"the stage wrote its input {k}"
    for k in ("taken", "len", "faddr", "laddr", "stats"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[0]}: host {got[k][bad[0]]} restatement {want[k][bad[0]]}"
    bad = np.nonzero(mine != want_buf)[0]
    assert len(bad) == 0, (f"buffer: {len(bad)} bytes differ, first at {bad[0]} (slab_len {slab_len}): "
                           f"host {mine[bad[0]]:#x} restatement {want_buf[bad[0]]:#x}")
    return got, mine


def desc(flags, seq=0x11223344, ack=0x55667788, wnd=0x1234, urp=0, ln=0):
    return np.array([(seq, ack, wnd, urp, ln, flags, 0)], TXSEG_DT)


def one_segment(tx, flags, tcb=None, ln=0, **kw):
    """One SEGMENT frame on a connection with these attributes: (option bytes,
    the 20 header bytes, outputs, buffer)."""
    conns = [R.conn(tcb={**dict(max_mss=1460, ts_recent=TSR), **(tcb or {})}, tx=tx)]
    pcbs, tcbs = R.make_tables(conns)
    try:
        d = desc(flags, ln=ln, **kw)
        snd = np.arange(ln, dtype=np.uint8) + 1 if ln else None
        got, buf = run(tcbs, conns, np.zeros(1, np.uint32), txseg=d, snd=snd, src_off=np.zeros(1, np.uint64) if ln else None)
    finally:
        tcbs.close()
        pcbs.close()
    optlen = int(got["len"][0]) - 20 - ln if got["taken"][0] else 0
    return bytes(buf[H + 46:H + 46 + optlen]), bytes(buf[H + 26:H + 46]), got, buf


def test_sizes_exports_and_refusals():
    assert ctypes.sizeof(N.TcbTx) == 4 and ctypes.sizeof(N.TcpOutIo) == 112
    assert TXSEG_DT.itemsize == 16 and R.TXSEG_DT == TXSEG_DT
    names = N.l4_exported_symbols("cndp_tcpout.h")
    assert set(names) == {"cndp_tcb_tx_set", "cndp_tcb_tx_get", "cndp_tcp_output_host", "cndp_tcp_send_optlen"}
    L = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert hasattr(L, nm), nm
    assert (R.SENT, R.NOTSEL, R.NOPCB, R.NOLADDR, R.TOOBIG, R.RST_IN, R.MCAST, R.OPTS, R.NSTATS) == (
        N.CNDP_TCPOUT_STAT_SENT, N.CNDP_TCPOUT_STAT_NOTSEL, N.CNDP_TCPOUT_STAT_NOPCB, N.CNDP_TCPOUT_STAT_NOLADDR,
        N.CNDP_TCPOUT_STAT_TOOBIG, N.CNDP_TCPOUT_STAT_RST_IN, N.CNDP_TCPOUT_STAT_MCAST, N.CNDP_TCPOUT_STAT_OPTS,
        N.CNDP_TCPOUT_NSTATS)
    assert (R.REQ_SCALE, R.RCVD_SCALE, R.REQ_TSTAMP, R.RCVD_TSTAMP) == (
        N.CNDP_TCBF_REQ_SCALE, N.CNDP_TCBF_RCVD_SCALE, N.CNDP_TCBF_REQ_TSTAMP, N.CNDP_TCBF_RCVD_TSTAMP)


# ---- tcp_send_options, by hand ------------------------------------------------
def test_option_bytes_by_hand():
    ts = bytes.fromhex("0101080a") + bytes.fromhex("01020304") + bytes.fromhex("0a0b0c0d")
    # the first SYN, scaling and timestamps requested: MSS 1460, WS 7 + NOP, NOP NOP TS(now, ts_recent)
    o, h, got, _ = one_segment(dict(tflags=R.REQ_SCALE | R.REQ_TSTAMP, req_recv_scale=7), R.SYN)
    assert o == bytes.fromhex("020405b4" "03030701") + ts and h[12] == 0xA0 and got["len"][0] == 40
    assert h == bytes.fromhex("0050" "9c40" "11223344" "55667788" "a002" "1234" "0000" "0000")
    # SYN|ACK: the window scale only if the peer sent one, the timestamp only if the peer sent one
    o, h, _, _ = one_segment(dict(tflags=R.REQ_SCALE, req_recv_scale=7), R.SYN | R.ACK)
    assert o == bytes.fromhex("020405b4") and h[12] == 0x60
    o, _, _, _ = one_segment(dict(tflags=R.REQ_SCALE | R.RCVD_SCALE, req_recv_scale=7), R.SYN | R.ACK)
    assert o == bytes.fromhex("020405b4" "03030701")
    o, h, _, _ = one_segment(dict(tflags=R.REQ_TSTAMP), R.SYN | R.ACK)
    assert o == bytes.fromhex("020405b4") and h[12] == 0x60
    o, h, _, _ = one_segment(dict(tflags=R.REQ_TSTAMP | R.RCVD_TSTAMP), R.SYN | R.ACK)
    assert o == bytes.fromhex("020405b4") + ts and h[12] == 0x90
    # RST with timestamps negotiated: no options
    for fl in (R.RST, R.RST | R.ACK):
        o, h, got, _ = one_segment(dict(tflags=0x0F, req_recv_scale=7), fl)
        assert o == b"" and h[12] == 0x50 and got["len"][0] == 20
    # a plain ACK with the timestamp negotiated: 12 bytes; requested but not received: none
    o, h, got, _ = one_segment(dict(tflags=R.REQ_TSTAMP | R.RCVD_TSTAMP), R.ACK)
    assert o == ts and h[12] == 0x80 and got["len"][0] == 32 and got["stats"][R.OPTS] == 1
    o, _, got, _ = one_segment(dict(tflags=R.REQ_TSTAMP), R.ACK)
    assert o == b"" and got["stats"][R.OPTS] == 0
    o, _, _, _ = one_segment(dict(tflags=R.RCVD_TSTAMP | R.RCVD_SCALE), R.SYN)      # received but never requested
    assert o == bytes.fromhex("020405b4")
    # SYN with RST: MSS and WS still go out, the timestamp does not
    o, _, _, _ = one_segment(dict(tflags=0x0F, req_recv_scale=14), R.SYN | R.RST)
    assert o == bytes.fromhex("020405b4" "03030e01")
    # timestamp alone on a first SYN: MSS then TS at word 1
    o, h, _, _ = one_segment(dict(tflags=R.REQ_TSTAMP), R.SYN, tcb=dict(max_mss=0x0218))
    assert o == bytes.fromhex("02040218") + ts and h[12] == 0x90


def test_send_optlen_is_the_options_length():
    for tf in range(16):
        for fl in range(64):
            tcb, tx = dict(R.TCB_ZERO, max_mss=1460), dict(R.TX_ZERO, tflags=tf)
            assert send_optlen(tf, fl) == len(R.send_options(tcb, tx, fl, 5)), (tf, fl)
    assert {send_optlen(tf, fl) for tf in range(16) for fl in range(64)} == {0, 4, 8, 12, 16, 20}
    assert send_optlen(0xF0, 0xC2) == 4      # bits outside the four flags / the six TCP flags are not read


def test_where_the_header_lands_and_the_memset():
    """H + 26 whatever the options; the memset clears 46 + optlen bytes at P, so a
    short segment leaves zeroes behind its payload and [H, H + 26) is untouched."""
    for tx, fl, optlen in ((dict(), R.ACK, 0), (dict(tflags=0x0F), R.SYN, 20), (dict(tflags=0x0C), R.ACK, 12)):
        for ln in (0, 1, 45 + optlen, 46 + optlen, 47 + optlen):
            o, h, got, buf = one_segment(tx, fl, ln=ln)
            assert len(o) == optlen and got["len"][0] == 20 + optlen + ln
            P = H + 46 + optlen
            assert bytes(buf[P:P + ln]) == bytes((np.arange(ln) + 1).astype(np.uint8))
            assert not buf[P + ln:P + 46 + optlen].any()
            lay = R.layout("packed", [H + 46 + optlen + max(ln, 46 + optlen)], H, seed=1)
            assert np.array_equal(buf[:H + 26], lay[0][:H + 26])                          # the same seeded bytes
            end = P + max(ln, 46 + optlen)
            assert np.array_equal(buf[end:], lay[0][end:])


# ---- tcp_drop_with_reset, by hand ----------------------------------------------
def respond(conns, segs, verdict=None, sel=None, rxmeta=None, prefill=None, now=NOW, txseg=None):
    pcbs, tcbs = R.make_tables(conns)
    try:
        n = len(segs) if segs is not None else len(txseg)
        seg = None if segs is None else np.array(segs, R.SEG_DT)
        if verdict is None and sel is None:
            verdict = np.full(n, N.CNDP_TCPSEG_RESET | N.CNDP_TCPSEG_FIRST, np.uint8)
        lay = R.layout("packed", [H + 66 + 66] * n, H, seed=n)
        got, buf = run(tcbs, conns, np.arange(n, dtype=np.uint32) % len(conns), mode=R.RESPOND, seg=seg, verdict=verdict,
                       sel=sel, rxmeta=rxmeta, lay=lay, prefill=prefill, now=now, txseg=txseg)
        rows = buf[:lay[1]].reshape(n, lay[2])
        return got, [bytes(r[H + 26:H + 66]) for r in rows], buf, lay
    finally:
        tcbs.close()
        pcbs.close()


def test_drop_with_reset_table():
    c = [R.conn(tcb=None)]
    segs = [(1000, 7000, 512, 0, 0, R.ACK, 20),              # ACK: <SEQ=SEG.ACK><CTL=RST>
            (1000, 7000, 512, 0, 10, R.PSH, 20),             # no ACK: <SEQ=0><ACK=SEG.LEN><CTL=RST,ACK>
            (1000, 0, 512, 0, 1, R.SYN, 24),                 # SYN: len 1 already counts it, and is bumped again
            (1000, 0, 512, 0, 0xFFFF, R.SYN, 20),            # ... in uint16_t
            (1000, 7000, 512, 0, 0, R.RST, 20), (1000, 7000, 512, 0, 0, R.RST | R.ACK, 20),     # RST in: nothing
            (1000, 7000, 512, 0, 1, R.SYN | R.ACK, 20)]
    got, hdr, buf, lay = respond(c, segs)
    assert got["taken"].tolist() == [1, 1, 1, 1, 0, 0, 1] and got["len"].tolist() == [20, 20, 20, 20, 0, 0, 20]
    ports = bytes.fromhex("00509c40")
    # seg->seq is zeroed before seg->seq + seg->len is formed: the ACK number is 0 + len (+ 1 for SYN)
    assert hdr[0][:20] == ports + (7000).to_bytes(4, "big") + bytes(4) + bytes([0x50, R.RST]) + bytes(6)
    assert hdr[1][:20] == ports + bytes(4) + (0 + 10).to_bytes(4, "big") + bytes([0x50, R.RST | R.ACK]) + bytes(6)
    assert hdr[2][:20] == ports + bytes(4) + (0 + 1 + 1).to_bytes(4, "big") + bytes([0x50, R.RST | R.ACK]) + bytes(6)
    assert hdr[3][:20] == ports + bytes(4) + bytes(4) + bytes([0x50, R.RST | R.ACK]) + bytes(6)
    assert hdr[6][:20] == ports + (7000).to_bytes(4, "big") + bytes(4) + bytes([0x50, R.RST]) + bytes(6)
    assert got["stats"].tolist() == [5, 0, 0, 0, 0, 2, 0, 0]
    # the slots of the two RST segments, and everything outside [H + 26, H + 46) of the others, are untouched
    rows, orig = buf[:lay[1]].reshape(7, -1), lay[0][:lay[1]].reshape(7, -1)
    assert np.array_equal(rows[4:6], orig[4:6])
    assert np.array_equal(rows[:, :H + 26], orig[:, :H + 26]) and np.array_equal(rows[:, H + 46:], orig[:, H + 46:])
    # faddr / laddr as ip4_output takes them
    assert got["faddr"][0] == R.net32(0xC6120001) and got["laddr"][0] == R.net32(0x0A040001) and got["faddr"][4] == 0


def test_respond_selection_key_addresses_and_multicast():
    listener = R.conn(faddr=0, fport=0, tcb=dict(max_mss=1460))             # a wildcard PCB
    gone = R.conn(live=False)
    c = [listener, gone, R.conn(laddr=0, tcb=None)]
    seg = (5, 9, 1, 0, 0, R.ACK, 20)
    # without sel the RESET verdict decides; with it, sel alone
    v = np.array([N.CNDP_TCPSEG_RESET, N.CNDP_TCPSEG_SLOW | 0x80, N.CNDP_TCPSEG_RESET | 0x80], np.uint8)
    got, hdr, _, _ = respond([listener], [seg] * 3, verdict=v)
    assert got["taken"].tolist() == [1, 0, 1] and got["stats"][R.NOTSEL] == 1
    got, hdr, _, _ = respond(c, [seg] * 3, sel=np.array([1, 1, 1], np.uint8), verdict=np.zeros(3, np.uint8))
    assert got["taken"].tolist() == [1, 0, 1] and got["stats"].tolist() == [2, 0, 1, 0, 0, 0, 0, 0]
    # addresses AND ports from the key: the listener's reply goes to 0.0.0.0:0, from a zero laddr likewise
    assert hdr[0][:4] == bytes.fromhex("00500000") and got["faddr"][0] == 0 and got["laddr"][0] == R.net32(0x0A040001)
    assert got["laddr"][2] == 0 and got["faddr"][2] == R.net32(0xC6120001)
    # the multicast tests, only with rxmeta: ip->dst_addr as loaded against the host-order range looks at the
    # address's LAST byte; the group bit of the destination MAC
    rx = np.full(4, 14 | 20 << 7, np.uint32)
    stride = H + 132 + 1

    def frames(buf):
        rows = buf[:4 * stride].reshape(4, stride)
        rows[:, H] = 0x02
        rows[:, H + 14 + 16:H + 14 + 20] = [10, 4, 0, 1]
        rows[1, H + 14 + 16:H + 14 + 20] = [10, 4, 0, 224]      # 10.4.0.224 "is" multicast
        rows[2, H + 14 + 16:H + 14 + 20] = [224, 0, 0, 1]       # 224.0.0.1 is not
        rows[3, H] = 0x03                                       # a group MAC
    got, _, _, _ = respond([listener], [seg] * 4, rxmeta=rx, prefill=frames)
    assert got["taken"].tolist() == [1, 0, 1, 0] and got["stats"][R.MCAST] == 2
    got, _, _, _ = respond([listener], [seg] * 4, prefill=frames)                     # no rxmeta: no test
    assert got["taken"].tolist() == [1, 1, 1, 1]


def test_response_window_rule():
    """tcp_do_response alone (txseg + sel): the window only with a TCB and without
    RST, min(rcv_space, TCP_MAXWIN << rcv_scale) >> rcv_scale; options as
    tcp_send_options gives them for the flags."""
    wnd = lambda h: int.from_bytes(h[14:16], "big")  # noqa: E731
    sel = np.ones(1, np.uint8)
    for space, sc, want in ((1000, 0, 1000), (65535, 0, 65535), (65536, 0, 65535), (1 << 20, 0, 65535),
                            (1 << 20, 7, (1 << 20) >> 7), ((65535 << 7) + 1, 7, 65535), (0xFFFFFFFF, 14, 65535),
                            (65535 << 14, 14, 65535), ((65535 << 14) - 1, 14, 65534), (0, 3, 0), (7, 3, 0), (8, 3, 1)):
        c = [R.conn(tcb=dict(max_mss=1460, rcv_space=space, ts_recent=TSR), tx=dict(rcv_scale=sc, tflags=0x0C))]
        got, hdr, _, _ = respond(c, None, sel=sel, txseg=desc(R.ACK, seq=77, ack=99, wnd=0xAAAA, urp=0xBBBB, ln=500))
        assert wnd(hdr[0]) == want, (space, sc)
        assert got["len"][0] == 32 and hdr[0][12] == 0x80 and hdr[0][18:20] == b"\0\0"       # the descriptor's urp is not read
        assert hdr[0][4:12] == (77).to_bytes(4, "big") + (99).to_bytes(4, "big")
        assert hdr[0][20:32] == bytes.fromhex("0101080a010203040a0b0c0d")
        got, hdr, _, _ = respond(c, None, sel=sel, txseg=desc(R.RST | R.ACK))
        assert wnd(hdr[0]) == 0 and got["len"][0] == 20
    got, hdr, _, _ = respond([R.conn(tcb=None)], None, sel=sel, txseg=desc(R.ACK))
    assert wnd(hdr[0]) == 0 and got["len"][0] == 20 and got["taken"][0] == 1          # no TCB: no options, window 0


# ---- random cases ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["packed", "umem", "offsets"])
def test_random_cases_against_the_restatement(kind):
    """20480 seeded cases over the three layouts (with H + 26 at every residue mod
    4), both modes, with and without a send buffer, sparse selection, and slabs
    that end inside the last frames."""
    rng = np.random.default_rng({"packed": 11, "umem": 12, "offsets": 13}[kind])
    conns = R.random_world(rng, 300)
    pcbs, tcbs = R.make_tables(conns)
    seen = np.zeros(R.NSTATS, np.int64)
    optlens = set()
    try:
        batches = [(R.SEGMENT, 683)] * 8 + [(R.RESPOND, 683)] * 2       # 10 x 683 = 6830 per layout, 20490 in all
        for b, (mode, n) in enumerate(batches):
            now = int(rng.integers(0, 1 << 32))
            data_off = 256 if kind == "umem" else 8 + b % 4
            pcb, d = R.random_descs(rng, conns, n, now)
            if kind == "umem":
                d["len"] = np.minimum(d["len"], 1600)                    # a 2 KiB frame: the jumbo MSS does not fit
            sel = (rng.random(n) < 0.8).astype(np.uint8) if b % 3 else None
            need = R.need_bytes(conns, pcb, d, now, data_off)
            cut = [None, 0, 3, 30, 70][b % 5] if kind == "offsets" else None
            lay = R.layout(kind, need, data_off, seed=b, align=1, cut=cut)
            if mode == R.SEGMENT:
                snd = rng.integers(0, 256, 5000, dtype=np.uint8) if b % 4 != 3 else None
                src = rng.integers(0, 5000 - 1400, n).astype(np.uint64) if snd is not None else None
                if snd is not None:
                    src[::17] = 5000 - 5                                 # a source that ends with snd_len, and past it
                    src[5::41] = 5000 + 9
                got, _ = run(tcbs, conns, pcb, txseg=d, sel=sel, snd=snd, src_off=src, lay=lay, data_off=data_off, now=now)
                optlens |= set((got["len"][got["taken"] != 0].astype(int) - 20 - d["len"][got["taken"] != 0]).tolist())
            else:
                seg = np.zeros(n, R.SEG_DT)
                for f in ("seq", "ack", "wnd", "urp", "len", "flags"):
                    seg[f] = d[f]
                seg["offset"] = 20
                verdict = rng.choice([1, 1, 1, 4, 0x81], n).astype(np.uint8)
                rx = np.full(n, 14 | 20 << 7, np.uint32) if b % 2 else None
                got, _ = run(tcbs, conns, pcb, mode=R.RESPOND, seg=seg, verdict=verdict, sel=sel, rxmeta=rx, lay=lay,
                             data_off=data_off, now=now)
            seen += got["stats"].astype(np.int64)
    finally:
        tcbs.close()
        pcbs.close()
    assert seen[:R.OPTS].sum() == 6830 and (seen > 0).all(), seen
    assert optlens == {0, 4, 8, 12, 16, 20}


# ---- the calls' return codes ---------------------------------------------------
def test_attribute_calls_and_return_codes():
    L = N.lib()
    pcbs = PcbTable(8)
    tcbs = TcbTable(pcbs)
    try:
        a = N.TcbTx()
        assert L.cndp_tcb_tx_set(None, 0, ctypes.byref(a)) == -22 and L.cndp_tcb_tx_get(None, 0, ctypes.byref(a)) == -22
        assert tcbs.tx_set_raw(0, tflags=1) == -22                       # no PCB yet
        for i in range(4):
            assert pcbs.add(laddr=0x0A040001, lport=80, faddr=0xC6120001, fport=1000 + i) == i
        assert L.cndp_tcb_tx_set(tcbs.h, 0, None) == -22 and L.cndp_tcb_tx_get(tcbs.h, 0, None) == -22
        assert tcbs.tx_set_raw(4, tflags=1) == -22 and tcbs.tx_set_raw(0xFFFFFFFF, tflags=1) == -22
        assert tcbs.tx_set_raw(0, tflags=1) == -2 and tcbs.tx_get(0) is None          # a PCB without a TCB
        tcbs.set(0, state=5, max_mss=1460)
        assert tcbs.tx_get(0) == dict(tflags=0, req_recv_scale=0, rcv_scale=0)        # a fresh TCB: all zero
        assert tcbs.tx_set_raw(0, tflags=0xFF, req_recv_scale=255, rcv_scale=14) == 0
        assert tcbs.tx_get(0) == dict(tflags=0x0F, req_recv_scale=255, rcv_scale=14)  # only the four flags are kept
        snap = tcbs.get(0)
        tcbs.set(0, state=4, max_mss=536, ts_recent=9)                                # cndp_tcb_set keeps them
        assert tcbs.tx_get(0) == dict(tflags=0x0F, req_recv_scale=255, rcv_scale=14)
        assert tcbs.get(0) == dict(snap, state=4, max_mss=536, ts_recent=9)           # and tx_set left the snapshot alone
        assert tcbs.clear(0) == 0 and tcbs.tx_get(0) is None and tcbs.tx_set_raw(0, tflags=1) == -2
        tcbs.set(0, state=5)
        assert tcbs.tx_get(0) == dict(tflags=0, req_recv_scale=0, rcv_scale=0)        # cleared with the TCB
        tcbs.set(1, state=5)
        tcbs.tx_set(1, tflags=5, rcv_scale=3)
        assert pcbs.delete(1) == 0                                                    # ... and by a PCB delete
        assert tcbs.tx_get(1) is None and tcbs.tx_set_raw(1, tflags=1) == -2
        assert pcbs.add(laddr=0x0A040001, lport=80, faddr=0xC6120001, fport=1001) == 4
        tcbs.set(4, state=5)
        assert tcbs.tx_get(4) == dict(tflags=0, req_recv_scale=0, rcv_scale=0)
    finally:
        tcbs.close()
        pcbs.close()


def test_output_call_refusals():
    L = N.lib()
    conns = [R.conn(tcb=dict(max_mss=1460))]
    pcbs, tcbs = R.make_tables(conns)
    try:
        slab = np.zeros(512, np.uint8)
        raw = np.zeros(64, np.uint8)
        a16 = raw[(-raw.ctypes.data) % 16:]
        pcb, ln, fa, la = np.zeros(1, np.uint32), np.zeros(1, np.uint16), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        tk, sel, off = np.zeros(1, np.uint8), np.ones(1, np.uint8), np.zeros(1, np.uint64)

        def call(mode=0, t=tcbs.h, n=1, slab_p=slab.ctypes.data, slab_len=512, **f):
            io = N.TcpOutIo()
            base = dict(pcb=pcb.ctypes.data, txseg=a16.ctypes.data, len=ln.ctypes.data, faddr=fa.ctypes.data,
                        laddr=la.ctypes.data, taken=tk.ctypes.data)
            for k, v in {**base, **f}.items():
                setattr(io, k, v)
            return L.cndp_tcp_output_host(t, mode, 0, slab_p, slab_len, 256, None, 64, n, ctypes.byref(io))

        assert call() == 0 and tk[0] == 1
        assert call(t=None) == -22 and call(mode=2) == -22 and call(slab_p=None) == -22 and call(slab_len=1 << 63) == -22
        assert L.cndp_tcp_output_host(tcbs.h, 0, 0, slab.ctypes.data, 512, 256, None, 64, 1, None) == -22
        for k in ("pcb", "txseg", "len", "faddr", "laddr", "taken"):
            assert call(**{k: None}) == -22, k
        assert call(txseg=a16.ctypes.data + 4) == -22 and call(txseg=a16.ctypes.data + 8) == -22      # misaligned
        assert call(snd=slab.ctypes.data, snd_len=4) == -22                                         # snd without src_off
        assert call(snd=slab.ctypes.data, snd_len=4, src_off=off.ctypes.data) == 0
        assert call(n=0, pcb=None, txseg=None, len=None) == 0                                         # an empty batch
        # RESPOND: seg (aligned) and a verdict or sel; or txseg with sel
        assert call(mode=1, txseg=None) == -22 and call(mode=1, txseg=None, seg=a16.ctypes.data) == -22
        assert call(mode=1, txseg=None, seg=a16.ctypes.data + 4, sel=sel.ctypes.data) == -22
        assert call(mode=1, txseg=None, seg=a16.ctypes.data, sel=sel.ctypes.data) == 0
        assert call(mode=1, txseg=None, seg=a16.ctypes.data, verdict=sel.ctypes.data) == 0
        assert call(mode=1) == -22 and call(mode=1, sel=sel.ctypes.data) == 0
        assert not slab[:64 + 26].any() and not slab[64 + 46:].any()
    finally:
        tcbs.close()
        pcbs.close()


def test_not_taken_reasons_in_one_batch_leave_their_slots_alone():
    conns = [R.conn(tcb=dict(max_mss=100), tx=dict(tflags=0x0C)), R.conn(tcb=None), R.conn(live=False),
             R.conn(laddr=0, tcb=dict(max_mss=100)), R.conn(tcb=dict(max_mss=12), tx=dict(tflags=0x0F))]
    pcbs, tcbs = R.make_tables(conns, cap=8)
    try:
        pcb = np.array([0, 0, 1, 2, 3, 0, 0, 0xFFFFFFFF, 5, 8, 4, 4], np.uint32)
        d = np.zeros(12, TXSEG_DT)
        d["flags"] = R.ACK
        d["len"] = [88, 88, 1, 1, 1, 89, 88, 1, 1, 1, 0, 0]             # 100 - 12 = 88 is the most PCB 0 carries
        d["flags"][11] = R.SYN                                          # max_mss 12 - optlen 20 < 0: even len 0 is too big
        sel = np.array([1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], np.uint8)
        snd = np.arange(256, dtype=np.uint8)
        got, buf = run(tcbs, conns, pcb, txseg=d, sel=sel, snd=snd, src_off=np.zeros(12, np.uint64),
                       lay=R.layout("packed", [H + 300] * 12, H, seed=3))
        assert got["taken"].tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0]
        assert got["stats"].tolist() == [3, 1, 5, 1, 2, 0, 0, 3]
        lay = R.layout("packed", [H + 300] * 12, H, seed=3)
        rows, orig = buf[:lay[1]].reshape(12, -1), lay[0][:lay[1]].reshape(12, -1)
        for i in np.nonzero(got["taken"] == 0)[0]:
            assert np.array_equal(rows[i], orig[i]), i
        assert (got["len"][got["taken"] == 0] == 0).all() and got["len"][0] == 20 + 12 + 88
    finally:
        tcbs.close()
        pcbs.close()


def test_tcp_segment_host_is_unchanged_by_tx_set():
    rng = np.random.default_rng(5)
    pcbs = PcbTable(64)
    for i in range(64):
        assert pcbs.add(laddr=0x0A040001, lport=80, faddr=0xC6120000 + i, fport=40000) == i
    tcbs = TcbTable(pcbs)
    try:
        cases = [S.random_case(rng, 1000) for _ in range(64)]
        for i, (t, _) in enumerate(cases):
            if t is not None:
                tcbs.set(i, **t)
        b = S.build([c[1] for c in cases])
        args = (b["slab"], 64, b["rxmeta"], np.arange(64, dtype=np.uint32), b["seg"], 1000)
        kw = dict(sel=np.ones(64, np.uint8), offsets=b["offsets"])
        before = tcbs.segment_host(*args, **kw)
        snaps = [tcbs.get(i) for i in range(64)]
        for i, (t, _) in enumerate(cases):
            if t is not None:
                tcbs.tx_set(i, tflags=0x0F, req_recv_scale=255, rcv_scale=255)
        after = tcbs.segment_host(*args, **kw)
        for k in ("opt", "verdict", "stats"):
            assert np.array_equal(before[k], after[k]), k
        assert [tcbs.get(i) for i in range(64)] == snaps
    finally:
        tcbs.close()
        pcbs.close()


def test_tcpout_under_sanitizers():
    """tests/tcpout_host/tcpout_san: tcpout.c, tcb.c and pcb.c built with
    -fsanitize=address,undefined in a program of its own, run as a child process:
    both modes over heap buffers that end inside the header, the options, the
    payload and the zero fill, and send buffers that end inside the payload."""
    d = os.path.join(HERE, "tcpout_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "tcpout_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    flags = open(os.path.join(d, "Makefile")).read()
    assert "-fsanitize=address,undefined" in flags

"""TCP option parse and header-prediction triage on the GPU
(cndp_gpu_tcp_segment, include/cndp_tcb.h): cnet classify -> udp_input ->
tcp_input -> tcp_segment, and opt, verdict and the counters must equal the
Python restatement (tests/tcpseg_ref.py) applied to the same arrays, for every
frame.  Shapes are the smallest that can still go wrong: one frame, a wave and
its neighbours, more than one 256-lane block (and more than one 1024-lane block
of tcp_input); packed slots, the UMEM stride, odd byte offsets; tables of 1, 513
and 4096 connections; options that end with the slab.  The last three tests
hold the stage against recorded outputs of the compiled reference
(tests/golden/tcp_options_ref.npz, tests/tcp_golden.py) and put IP options in
front of the TCP header."""
import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd.l4 import PcbTable, TcbTable, alloc_tcpseg_outputs, opt_records, seg_records

import tcp_golden as TG
import tcp_ref as T
import tcpseg_ref as S
from helpers import cnet_fibs

pytestmark = pytest.mark.gpu
LAYOUTS = {"packed": dict(layout="packed", slot=128), "umem": dict(layout="umem"), "odd": dict(layout="offsets", align=1)}
NOBODY = 4444      # no PCB has this local port: tcp_input punts the frame
EST = dict(rcv_nxt=1000, snd_una=5000, snd_nxt=6000, snd_max=6000, snd_wnd=8192, snd_cwnd=10000, ts_recent=500,
           last_ack_sent=900, rcv_space=100, max_mss=1460, state=S.ESTABLISHED, snd_scale=3, flags=1)
PURE_ACK = dict(seq=1000, ack=5500, wnd=1024, flags=S.ACK)


@pytest.fixture(scope="module")
def cnet(gpu):
    from cndp_amd.classify import Classifier
    fib, fib6, routes, *_ = cnet_fibs()
    cl = Classifier(0)
    cl.set_fib(fib, fib6)
    local = [ip for ip, d, _ in routes if d == 32]      # ip4_input's proto edge
    udp = PcbTable(4)                                   # the UDP vector: empty, ip4_proto built with TCP
    udp.set_flags(punt_enabled=True, tcp_enabled=True)
    yield cl, local[0], udp
    udp.close()
    cl.close()


class Conns:
    """k connections to local:80 (PCB index = connection index) and their TCBs."""

    def __init__(self, local, k, cap=None):
        self.local, self.k, self.cap = local, k, cap or k
        self.peers = [(0xC6130000 + (i % 251), 1024 + i) for i in range(k)]
        self.pcbs = PcbTable(self.cap)
        for i, (fa, fp) in enumerate(self.peers):
            assert self.pcbs.add(laddr=local, lport=80, faddr=fa, fport=fp) == i
        self.tcbs = TcbTable(self.pcbs)
        self.image = [None] * self.cap

    def set(self, i, tcb):
        if tcb is None:
            if self.image[i] is not None:
                assert self.tcbs.clear(i) == 0
        else:
            self.tcbs.set(i, **tcb)
        self.image[i] = tcb

    def pair(self, i):
        return ((self.local, 80), self.peers[i])

    def close(self):
        self.tcbs.close()
        self.pcbs.close()


def host(t, dt):
    return t.cpu().numpy().view(dt)


def upstream(cnet, co, specs, layout):
    """The frames of `specs` on the device and the three stages in front:
    (frames, classify outputs, tcp_input's result)."""
    cl, _, udp = cnet
    fr = S.to_frames(S.build(specs, **LAYOUTS[layout]), "cuda:0")
    cl.set_tuning(cnet_spec=256)     # a fresh ptype-node state, as in test_tcp_gpu
    out = cl.alloc_outputs(fr.n, 64, device=fr.slab.device, meta=True)
    cl.classify(fr, N.CNDP_MODE_CNET, out=out)
    l4 = cl.udp_input(fr, out, udp)
    tcp = cl.tcp_input(fr, out, co.pcbs, l4=l4)
    torch.cuda.synchronize()
    return fr, out, tcp


def segment(cnet, co, fr, out, tcp, now, sel=None, seg=None, stats0=None):
    """tcp_segment against the restatement on the same arrays; the inputs must
    come back as they went in.  Returns (got, want, the result tensors)."""
    cl = cnet[0]
    before = {k: tcp[k].clone() for k in ("l4edge", "pcb", "seg")}
    slab0 = fr.slab.clone()
    sel_t = torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).to(fr.slab.device) if sel is not None else None
    res = cl.tcp_segment(fr, out, co.tcbs, tcp, now=now, sel=sel_t, seg=seg)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(tcp[k], v), f"the stage wrote its input {k}"
    assert torch.equal(fr.slab, slab0), "the stage wrote the frames"
    got = {"opt": opt_records(res["opt"]), "verdict": host(res["verdict"], np.uint8), "stats": host(res["stats"], np.uint64)}
    offs = fr.offsets.cpu().numpy() if fr.offsets is not None else None
    want = S.tcp_segment_ref(fr.slab.cpu().numpy(), fr.n, host(out["rxmeta"], np.uint32), co.image,
                             host(tcp["pcb"], np.uint32), seg_records(tcp["seg"]), now,
                             l4edge=host(tcp["l4edge"], np.uint8), sel=sel, stride=fr.stride, offsets=offs,
                             data_off=fr.data_off, stats=stats0)
    for k in ("verdict", "opt", "stats"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[0]}: got {got[k][bad[0]]} want {want[k][bad[0]]}"
    return got, want, res


def random_batch(rng, co, n, now, one_per_conn=False):
    """n random cases on random connections of `co` (their TCBs set from the
    first case that lands on each), a few of them frames tcp_input will not put
    on the SEGMENT edge."""
    specs = []
    for i in range(n):
        c = i % co.k if one_per_conn else int(rng.integers(0, co.k))
        tcb, spec = S.random_case(rng, now)
        if co.image[c] is None and tcb is not None:
            co.set(c, tcb)
        spec["pair"] = co.pair(c)
        r = rng.random()
        if r < 0.04:
            spec["pair"] = ((co.local, NOBODY), co.peers[c])
        elif r < 0.08:
            spec["bad_cksum"] = True
        specs.append(spec)
    return specs


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_sizes_and_layouts(cnet, gpu, n, layout):
    rng = np.random.default_rng(100 + n)
    co = Conns(cnet[1], max(n - 60, 4))      # a connection per frame; the last 60 frames share the first 60's
    try:
        now = 0x7FFFFFF0
        specs = random_batch(rng, co, n, now, one_per_conn=True)
        if n == 1:
            specs[0].pop("bad_cksum", None)
            specs[0]["pair"] = co.pair(0)
        fr, out, tcp = upstream(cnet, co, specs, layout)
        got, want, _ = segment(cnet, co, fr, out, tcp, now)
        edge = host(tcp["l4edge"], np.uint8)
        assert ((got["verdict"] == 0) == (edge != T.E_SEG)).all()           # off the SEGMENT edge: NONE, opt zero
        assert not got["opt"][edge != T.E_SEG].view(np.uint8).any()
        assert got["stats"].sum() == n
        if n == 1025:      # the larger batch reaches every verdict and every flag
            assert (want["stats"] > 0).all(), want["stats"]
            assert int(np.bitwise_or.reduce(want["opt"]["sflags"])) & 0xF000 == 0xF000
            assert (want["verdict"] & S.TS_UPDATE).any() and (edge == T.E_PUNT).any() and (edge == T.E_DROP).any()
    finally:
        co.close()


@pytest.mark.parametrize("k", [1, 513, 4096])
def test_table_sizes(cnet, gpu, k):
    """One connection; 513; the fullest table, every TCB set, each connection's
    segment judged against its own entry of the 192 KiB image."""
    rng = np.random.default_rng(200 + k)
    co = Conns(cnet[1], k)
    try:
        now = 12345
        n = 257 if k < 4096 else 4096
        specs = random_batch(rng, co, n, now, one_per_conn=True)
        fr, out, tcp = upstream(cnet, co, specs, "packed")
        got, want, _ = segment(cnet, co, fr, out, tcp, now)
        taken = got["verdict"] != 0
        assert taken.sum() > 0.8 * n
        if k == 4096:
            assert len(np.unique(host(tcp["pcb"], np.uint32)[taken])) > 3500
            assert ((got["verdict"][taken] & S.FIRST) != 0).all()           # one frame per connection
            assert (want["stats"][1:] > 0).all()
    finally:
        co.close()


def test_options_that_end_with_the_slab(cnet, gpu):
    """Frames laid end to end, the slab sized to the last byte: the last frame's
    options end there with a known kind, whose length is then read past the slab
    and is zero.  The frame before it ends the same way, and its length byte is
    the next frame's first byte."""
    co = Conns(cnet[1], 4)
    try:
        for i in range(4):
            co.set(i, EST)
        ts = S.ts_opt(501, 7)
        specs = [dict(PURE_ACK, pair=co.pair(0), opts=bytes([1, 1]) + ts),
                 dict(PURE_ACK, pair=co.pair(1), opts=ts + bytes([1, 8])),          # length = 0x02, the next frame's dst MAC
                 dict(PURE_ACK, pair=co.pair(2), opts=bytes([1] * 39) + bytes([4])),
                 dict(PURE_ACK, pair=co.pair(3), opts=ts + bytes([1, 2]))]          # length past the slab: zero
        fr, out, tcp = upstream(cnet, co, specs, "odd")
        assert fr.slab.numel() == sum(14 + 20 + 20 + len(s["opts"]) for s in specs)
        got, _, _ = segment(cnet, co, fr, out, tcp, 1000)
        F = S.FIRST
        assert got["verdict"].tolist() == [S.PRED_ACK | F, S.BADOPT | F, S.BADOPT | F, S.BADOPT | F]
        assert tuple(got["opt"][0]) == (501, 7, 8192, 0, S.TS_PRESENT) and not got["opt"][1:].view(np.uint8).any()
        # an unknown kind there has no bound test: the next frame's 0x02 walks it off the end, the slab's zero fails it
        specs[1]["opts"], specs[3]["opts"] = ts + bytes([1, 5]), ts + bytes([1, 5])
        fr, out, tcp = upstream(cnet, co, specs, "odd")
        got, _, _ = segment(cnet, co, fr, out, tcp, 1000)
        assert got["verdict"].tolist() == [S.PRED_ACK | F, S.PRED_ACK | F, S.BADOPT | F, S.BADOPT | F]
    finally:
        co.close()


def test_first_frame_of_each_connection(cnet, gpu):
    """Several segments per connection, interleaved across blocks: exactly the
    lowest-index taken frame of each PCB carries FIRST, and a second run gives
    the same bytes."""
    rng = np.random.default_rng(31)
    co = Conns(cnet[1], 300)
    try:
        now, n = 99, 2500
        specs = random_batch(rng, co, n, now, one_per_conn=True)    # connection i % 300: 300 frames apart
        fr, out, tcp = upstream(cnet, co, specs, "packed")
        got, _, res = segment(cnet, co, fr, out, tcp, now)
        pcb, v = host(tcp["pcb"], np.uint32), got["verdict"]
        taken = np.nonzero(v != 0)[0]
        firsts = np.nonzero(v & S.FIRST)[0]
        lowest = {}
        for i in taken:
            lowest.setdefault(int(pcb[i]), int(i))
        assert sorted(lowest.values()) == firsts.tolist() and len(firsts) == 300
        assert (firsts >= 300).any()       # a connection whose first frame was dropped upstream: its next one is first
        assert np.bincount(pcb[taken], minlength=300).min() >= 5
        keep = {k: res[k].clone() for k in ("opt", "verdict")}
        got2, _, res2 = segment(cnet, co, fr, out, tcp, now)
        assert torch.equal(res2["opt"], keep["opt"]) and torch.equal(res2["verdict"], keep["verdict"])
    finally:
        co.close()


def test_selection_counters_and_tcb_changes_between_calls(cnet, gpu):
    rng = np.random.default_rng(32)
    co = Conns(cnet[1], 64)
    try:
        now, n = 5000, 321
        specs = random_batch(rng, co, n - 1, now) + [dict(PURE_ACK, pair=co.pair(63))]
        co.set(63, EST)
        fr, out, tcp = upstream(cnet, co, specs, "umem")
        got, want, res = segment(cnet, co, fr, out, tcp, now)
        assert got["verdict"][-1] & S.VMASK == S.PRED_ACK
        # the counters accumulate when the result is passed back
        got2, _, res = segment(cnet, co, fr, out, tcp, now, seg=res, stats0=want["stats"])
        assert (got2["stats"] == 2 * want["stats"]).all() and got2["stats"].sum() == 2 * n
        # sel decides alone; a selected frame that is not on the SEGMENT edge has no PCB and is not taken
        sel = (rng.random(n) < 0.5).astype(np.uint8)
        edge = host(tcp["l4edge"], np.uint8)
        sel[np.nonzero(edge != T.E_SEG)[0][:4]] = 1
        got3, _, _ = segment(cnet, co, fr, out, tcp, now, sel=sel)
        assert ((got3["verdict"] != 0) == ((sel != 0) & (edge == T.E_SEG))).all()
        assert (sel != 0).sum() > (got3["verdict"] != 0).sum() > 100
        # TCBs changed on the host reach the device before the next launch: closed, gone, set again
        for tcb, want_v in ((dict(EST, state=1), S.CLOSED), (None, S.RESET), (dict(EST, rcv_nxt=1001), S.SLOW),
                            (EST, S.PRED_ACK)):
            co.set(63, tcb)
            got4, _, _ = segment(cnet, co, fr, out, tcp, now)
            assert got4["verdict"][-1] & S.VMASK == want_v
        # ... and a PCB delete takes its TCB along
        assert co.pcbs.delete(63) == 0
        co.image[63] = None
        got5, _, _ = segment(cnet, co, fr, out, tcp, now)       # tcp_input's arrays still name PCB 63
        assert got5["verdict"][-1] & S.VMASK == S.RESET
    finally:
        co.close()


def test_errno_rules_and_empty_batch(cnet, gpu):
    cl = cnet[0]
    co = Conns(cnet[1], 2)
    try:
        co.set(0, EST)
        fr, out, tcp = upstream(cnet, co, [dict(PURE_ACK, pair=co.pair(0))] * 5, "packed")
        seg = alloc_tcpseg_outputs(5, gpu)
        seg["opt"] = torch.empty(6 * 4 + 1, dtype=torch.int32, device=gpu)[1:]        # 4 bytes off
        with pytest.raises(OSError) as e:
            cl.tcp_segment(fr, out, co.tcbs, tcp, seg=seg)
        assert e.value.errno == 22
        for missing in ("pcb", "seg", "l4edge"):
            with pytest.raises(OSError) as e:
                cl.tcp_segment(fr, out, co.tcbs, {k: v for k, v in tcp.items() if k != missing})
            assert e.value.errno == 22
        with pytest.raises(OSError) as e:
            cl.tcp_segment(fr, {}, co.tcbs, tcp)                                       # no rxmeta
        assert e.value.errno == 22
        from cndp_amd import pktgen
        fr0 = pktgen.Frames(fr.slab, 0, stride=fr.stride)
        res = cl.tcp_segment(fr0, {"rxmeta": out["rxmeta"][:0]}, co.tcbs, {k: tcp[k][:0] for k in ("l4edge", "pcb", "seg")})
        torch.cuda.synchronize()
        assert res["stats"].tolist() == [0] * 8
    finally:
        co.close()


# ---- against recorded outputs of the compiled reference (tests/golden/tcp_options_ref.npz) ----
def golden_batch(cnet, cases, now, layout):
    """One connection per case, the frames through classify -> udp_input ->
    tcp_input -> tcp_segment in one call: what the stage gave, after segment()
    has held it against the restatement.  Every frame must have reached the
    SEGMENT edge on its own connection, or the vector would go unjudged."""
    co = Conns(cnet[1], len(cases))
    try:
        specs = []
        for i, (tcb, spec) in enumerate(cases):
            co.set(i, tcb)
            specs.append(dict(spec, pair=co.pair(i)))
        fr, out, tcp = upstream(cnet, co, specs, layout)
        assert (host(tcp["l4edge"], np.uint8) == T.E_SEG).all()
        assert (host(tcp["pcb"], np.uint32) == np.arange(len(cases))).all()
        got, _, _ = segment(cnet, co, fr, out, tcp, now)
        assert ((got["verdict"] & S.FIRST) != 0).all() and got["stats"].sum() == len(cases) and got["stats"][0] == 0
        return got
    finally:
        co.close()


@pytest.mark.parametrize("layout", ["odd", "packed"])
def test_reference_option_vectors(cnet, gpu, layout):
    """The parse vectors of the golden file, one call per recorded `now`: BADOPT
    exactly where the compiled tcp_do_options returned -1, and its ts_val,
    ts_ecr, mss and sflags | req_scale where it returned 0.  In the odd layout
    the option bytes start at every byte alignment, so both of rd_words' paths
    run; each frame's one payload byte is the recorded byte behind the options."""
    G = TG.load()
    seen = 0
    for k, now in enumerate(G["nows"].tolist()):
        idx, cases = TG.parse_cases(G, k)
        got = golden_batch(cnet, cases, now, layout)
        TG.parse_check(G, idx, got["verdict"], got["opt"], f"GPU, {layout}, now {now:#x}")
        seen += len(idx)
    assert seen == len(G["p_tail"]) and seen <= 4096


@pytest.mark.parametrize("layout", ["odd", "packed"])
def test_reference_prediction_vectors(cnet, gpu, layout):
    """The prediction vectors: the branch tcp_header_prediction took (ack / data /
    neither) and whether it took ts_recent, as recorded.  The entry test in front
    of it is inline in cnet_tcp_input and stays restated: every vector passes it
but eight hand-built ones with ts_val = ts_recent - 1, which must come out SLOW."""
    G = TG.load()
    seen = 0
    for k, now in enumerate(G["nows"].tolist()):
        idx, cases = TG.pred_cases(G, k)
        if len(idx):
            got = golden_batch(cnet, cases, now, layout)
            TG.pred_check(G, idx, got["verdict"], got["opt"], f"GPU, {layout}, now {now:#x}")
            seen += len(idx)
    assert seen == len(G["h_branch"]) and seen <= 4096


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ip_options_in_front_of_tcp(cnet, gpu, layout):
    """65 pure ACKs with IHL 5, 6 and 15 mixed: the option bytes are at
    L2 + L3 + 20 with L3 up to 60, which needs all of CNDP_RXMETA_L3's bits.  The
    ptype node has no ip4_input edge for IPV4_EXT | TCP (the checker says so in
    test_tcp_reference_golden.py, and the stages say so here), so such frames
    never reach the SEGMENT edge by themselves: tcp_input is run again with
    sel=, over the rxmeta classify wrote, and tcp_segment takes what it left."""
    cl = cnet[0]
    cases = TG.ip_option_cases()
    co = Conns(cnet[1], len(cases))
    try:
        specs = []
        for i, (tcb, spec) in enumerate(cases):
            co.set(i, tcb)
            specs.append(dict(spec, pair=co.pair(i)))
        fr, out, tcp = upstream(cnet, co, specs, layout)
        ihl = np.array([s["ihl"] for s in specs])
        assert ((host(tcp["l4edge"], np.uint8) == T.E_SEG) == (ihl == 5)).all()
        assert (host(out["rxmeta"], np.uint32) & 0xFFFF == (14 | ihl * 4 << 7)).all()
        tcp = cl.tcp_input(fr, out, co.pcbs, sel=torch.ones(fr.n, dtype=torch.uint8, device=fr.slab.device))
        torch.cuda.synchronize()
        assert (host(tcp["l4edge"], np.uint8) == T.E_SEG).all() and (host(tcp["pcb"], np.uint32) == np.arange(fr.n)).all()
        got, _, _ = segment(cnet, co, fr, out, tcp, 1000)
        TG.ip_option_check(got["verdict"], got["opt"])
    finally:
        co.close()

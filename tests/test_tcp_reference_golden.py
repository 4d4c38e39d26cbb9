"""The TCP option parse, the send options and the header-prediction tests against
recorded outputs of the compiled reference (tests/golden/tcp_options_ref.npz,
made by tools/gen_tcp_options_golden.py from lib/cnet/tcp/cnet_tcp.c itself):
the Python restatements (tcpseg_ref, tcpout_ref) and the product's host twins
(cndp_tcp_segment_host -- the rule the kernel also runs -- cndp_tcp_output_host,
cndp_tcp_send_optlen) must all give what the reference gave.  No GPU."""
import numpy as np
import pytest

from cndp_amd.l4 import TXSEG_DT, PcbTable, TcbTable, addr_net, port_net, send_optlen

import l4_ref as L
import tcp_golden as TG
import tcp_ref as T
import tcpout_ref as R
import tcpseg_ref as S

CAP = 4096
H = 64


@pytest.fixture(scope="module")
def G():
    return TG.load()


@pytest.fixture(scope="module")
def tables():
    pcbs = PcbTable(CAP)
    for i in range(CAP):
        assert pcbs.add(laddr=0x0A040001, lport=80, faddr=0xC6120000 + i, fport=40000) == i
    tcbs = TcbTable(pcbs)
    yield pcbs, tcbs
    tcbs.close()
    pcbs.close()


def host_twin(tcbs, cases, now, layout):
    """One connection per case (PCB i = case i), one call: (verdict, opt)."""
    n = len(cases)
    assert n <= CAP
    for p, (t, _) in enumerate(cases):
        tcbs.set(p, **t)
    b = S.build([c[1] for c in cases], **layout)
    got = tcbs.segment_host(b["slab"], n, b["rxmeta"], np.arange(n, dtype=np.uint32), b["seg"], now,
                            sel=np.ones(n, np.uint8), stride=b["stride"], offsets=b["offsets"], data_off=b["data_off"])
    assert ((got["verdict"] & S.FIRST) != 0).all()
    return got["verdict"], got["opt"]


# ---- the golden file itself ----------------------------------------------------
def test_the_golden_file_meets_its_conditions(G):
    for f, sz in TG.sizes().items():
        assert sz < TG.LIMIT, (f, sz)
    names = G["p_cls_names"].tolist()
    for c in TG.P_CLASSES:
        assert c in names and int((G["p_cls"] == names.index(c)).sum()) >= 8, c
    cls = lambda c: G["p_cls"] == names.index(c)  # noqa: E731
    assert cls("last_byte").sum() >= 6 * 4 and cls("last_two").sum() >= 6 * 4 * 2 and cls("mid_len").sum() == 4 * 13 * 2
    assert cls("ts_ecr_now").sum() == 14 and cls("seeded").sum() >= 300 and cls("uniform").sum() >= 100
    assert set(G["p_rc"].tolist()) == {0, -1}
    assert len(G["nows"]) == 3 and set(G["p_now"].tolist()) <= {0, 1, 2}
    lens = np.diff(G["p_off"])
    assert set(lens.tolist()) == set(range(4, 44, 4)) and len(G["p_tail"]) == len(lens)
    hn = G["h_cls_names"].tolist()
    for c in TG.H_CLASSES:
        assert c in hn and int((G["h_cls"] == hn.index(c)).sum()) >= 8, c
    called = G["h_entry"] == 1
    assert set(G["h_branch"][called].tolist()) == {0, 1, 2} and set(G["h_ts"][called].tolist()) == {0, 1}
    assert int((G["h_cls"] == hn.index("seeded")).sum()) >= 300 and called[G["h_cls"] == hn.index("seeded")].all()
    # the hand-built timestamp edges are all there: ts_val = ts_recent - 1 fails the entry test, and only that does
    assert int((G["h_cls"] == hn.index("ts_edge")).sum()) == 24 and (G["h_cls"][~called] == hn.index("ts_edge")).all()
    assert int((~called).sum()) == 8
    # send: 16 attribute sets x 16 flag sets x 4 parameter sets, one of them with max_mss > 255 and top bits set
    assert len(G["s_tf"]) == 1024 and len({(a, b, c) for a, b, c in zip(G["s_tf"], G["s_flags"], G["s_set"])}) == 1024
    assert set(G["s_flags"].tolist()) == {s | a | r | f for s in (0, S.SYN) for a in (0, S.ACK) for r in (0, S.RST) for f in (0, S.FIN)}
    assert (G["s_max_mss"] > 255).all() and (G["s_max_mss"] & 0x8000).any() and (G["s_ts_recent"] >> 31).any() and (G["s_now"] >> 31).any()
    assert set(G["s_optlen"].tolist()) == {0, 4, 8, 12, 16, 20}
    # tcp_send_options' own side effect: snd_nxt = snd_iss on a SYN, else untouched
    syn = (G["s_flags"] & S.SYN) != 0
    assert (G["s_nxt"] == np.where(syn, G["s_iss"][G["s_set"]], G["s_nxt0"][G["s_set"]])).all()
    assert len(G["c_a"]) >= 200


# ---- the restatements ----------------------------------------------------------
def test_restated_parse_equals_the_recording(G):
    for i in range(len(G["p_tail"])):
        data = TG.p_opts(G, i) + bytes([int(G["p_tail"][i])])
        rd = lambda k, data=data: data[k] if k < len(data) else 0xFF  # noqa: E731   (0xFF: must not matter)
        got = S.do_options(rd, len(data) - 1, int(G["p_flags"][i]), int(G["p_max_mss"][i]), int(G["nows"][G["p_now"][i]]))
        assert got == TG.p_expect(G, i), (i, data.hex(), got, TG.p_expect(G, i))


def test_restated_send_options_equal_the_recording(G):
    for i in range(len(G["s_tf"])):
        k = int(G["s_set"][i])
        tcb = dict(R.TCB_ZERO, max_mss=int(G["s_max_mss"][k]), ts_recent=int(G["s_ts_recent"][k]))
        tx = dict(R.TX_ZERO, tflags=int(G["s_tf"][i]), req_recv_scale=int(G["s_scale"][k]))
        got = R.send_options(tcb, tx, int(G["s_flags"][i]), int(G["s_now"][k]))
        assert got == G["s_bytes"][i, :int(G["s_optlen"][i])].tobytes(), (i, got.hex())
        assert (G["s_bytes"][i, int(G["s_optlen"][i]):] == 0xEE).all()


def test_restated_comparisons_equal_the_recording(G):
    ops = {"seqLT": lambda d: d < 0, "seqLEQ": lambda d: d <= 0, "seqGT": lambda d: d > 0, "seqGEQ": lambda d: d >= 0,
           "seqEQ": lambda d: d == 0, "seqNE": lambda d: d != 0, "tstampLT": lambda d: d < 0, "tstampLEQ": lambda d: d <= 0,
           "tstampGEQ": lambda d: d >= 0}
    names = G["c_names"].tolist()
    assert set(names) == set(ops)
    for a, b, res in zip(G["c_a"].tolist(), G["c_b"].tolist(), G["c_res"].tolist()):
        for bit, nm in enumerate(names):
            assert ops[nm](S.s32(a - b)) == bool(res >> bit & 1), (nm, hex(a), hex(b))
    d = (G["c_a"].astype(np.int64) - G["c_b"].astype(np.int64)) & 0xFFFFFFFF
    assert {0, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0x80000001} <= set(d.tolist())


def test_restated_prediction_equals_the_recording(G):
    """The entry test is inline in cnet_tcp_input and cannot be called on its
    own, so it stays restated (tcpseg_ref.predic_entry): the generator kept the
    seeded cases that pass it on the compiled parse's results, and here every
    such vector must get past it to the PRED_* verdict the reference recorded.
    Eight hand-built edges (ts_val = ts_recent - 1) fail it and must be SLOW."""
    for j in range(len(G["h_branch"])):
        tcb, spec = TG.h_tcb(G, j), TG.h_spec(G, j)
        data = spec["opts"] + (spec["payload"][:1] or b"\0")
        seg = np.array([S.seg_of(spec)], T.SEG_DT)[0]
        v, opt = S.segment_one(tcb, seg, lambda k, data=data: data[k] if k < len(data) else 0, int(G["nows"][G["h_now"][j]]))
        assert v == TG.h_verdict(G, j), (j, G["h_cls_names"][G["h_cls"][j]], hex(v), hex(TG.h_verdict(G, j)))


# ---- the host twins ---------------------------------------------------------------
@pytest.mark.parametrize("layout", [dict(layout="packed", slot=128), dict(layout="offsets", align=1)], ids=["packed", "odd"])
def test_host_twin_parse_equals_the_recording(G, tables, layout):
    _, tcbs = tables
    seen = 0
    for k, now in enumerate(G["nows"].tolist()):
        idx, cases = TG.parse_cases(G, k)
        v, o = host_twin(tcbs, cases, now, layout)
        TG.parse_check(G, idx, v, o, f"host twin, now {now:#x}")
        seen += len(idx)
    assert seen == len(G["p_tail"])


@pytest.mark.parametrize("layout", [dict(layout="packed", slot=128), dict(layout="offsets", align=1)], ids=["packed", "odd"])
def test_host_twin_prediction_equals_the_recording(G, tables, layout):
    _, tcbs = tables
    seen = 0
    for k, now in enumerate(G["nows"].tolist()):
        idx, cases = TG.pred_cases(G, k)
        if len(idx):
            v, o = host_twin(tcbs, cases, now, layout)
            TG.pred_check(G, idx, v, o, f"host twin, now {now:#x}")
            seen += len(idx)
    assert seen == len(G["h_branch"])


def test_the_vectors_frames_reach_the_segment_edge(G):
    """What tcp_input (restated) makes of the frames built from the vectors: all
    of them go to the SEGMENT edge with the seg record build() gives, whatever
    their flags -- so the GPU tests, which send them through the real stages,
    judge every vector."""
    _, cases = TG.parse_cases(G, 2)
    _, more = TG.pred_cases(G, 2)
    specs = [c[1] for c in cases[::7] + more[::7]]
    b = S.build(specs, layout="packed", slot=128)
    ent = np.array([(addr_net(S.PAIR[0][0]), 0, port_net(S.PAIR[0][1]), 0, 0)], L.ENTRY_DT)
    t = T.tcp_input_ref(b["slab"], b["n"], b["rxmeta"], ent, sel=np.ones(b["n"], np.uint8), stride=b["stride"])
    assert (t["l4edge"] == T.E_SEG).all() and (t["seg"] == b["seg"]).all()


def test_host_send_options_equal_the_recording(G):
    """cndp_tcp_output_host, SEGMENT mode, one connection per (attributes,
    parameter set), one call per recorded `now`: the option bytes found in the
    built frame, the header's data offset and the reported length are the
    reference's; cndp_tcp_send_optlen gives the recorded length."""
    for k in range(len(G["s_max_mss"])):
        sel = np.nonzero(G["s_set"] == k)[0]
        conns = [R.conn(faddr=0xC6120000 + tf, fport=1024 + tf,
                        tcb=dict(max_mss=int(G["s_max_mss"][k]), ts_recent=int(G["s_ts_recent"][k])),
                        tx=dict(tflags=tf, req_recv_scale=int(G["s_scale"][k]))) for tf in range(16)]
        pcbs, tcbs = R.make_tables(conns)
        try:
            n, now = len(sel), int(G["s_now"][k])
            pcb = G["s_tf"][sel].astype(np.uint32)
            d = np.zeros(n, TXSEG_DT)
            d["seq"], d["ack"], d["wnd"], d["flags"] = 0x11223344, 0x55667788, 0x1234, G["s_flags"][sel]
            buf, slab_len, stride, offs = R.layout("packed", R.need_bytes(conns, pcb, d, now, H), H, seed=k)
            got = tcbs.output_host(buf[:slab_len], n, pcb, mode=R.SEGMENT, now=now, txseg=d, stride=stride, offsets=offs,
                                   data_off=H)
        finally:
            tcbs.close()
            pcbs.close()
        assert got["taken"].all()
        for j, i in enumerate(sel):
            ol, at = int(G["s_optlen"][i]), j * stride + H
            assert send_optlen(int(G["s_tf"][i]), int(G["s_flags"][i])) == ol, i
            assert int(got["len"][j]) == 20 + ol and buf[at + 26 + 12] >> 4 == (20 + ol) // 4, i
            assert buf[at + 46:at + 46 + ol].tobytes() == G["s_bytes"][i, :ol].tobytes(), (i, buf[at + 46:at + 66].tobytes().hex())
        assert int(got["stats"][R.OPTS]) == int((G["s_optlen"][sel] != 0).sum())


# ---- IP options in front of the TCP header -------------------------------------------
def test_ip_option_tcp_frames_stop_at_the_ptype_node():
    """Where the stages in front of tcp_segment send such frames, by the checker's
    classify (oracle/): IPv4 with options is L3_IPV4_EXT, and the ptype node has
    no ip4_input edge for IPV4_EXT | TCP (it has one for IPV4_EXT | UDP), so the
    frames leave the graph there with no FIB value, while rxmeta does carry their
    L3 length.  The stage therefore only meets IP options through its sel= path,
    which is how the tests here and on the GPU drive it."""
    from oracle import oracle as O
    from helpers import CNET_DEF, cnet_fibs
    _, _, routes, _, v4vals, v6vals = cnet_fibs()
    t4, t6 = O.dir24_8_build(v4vals, CNET_DEF, 256), O.trie_build(v6vals, CNET_DEF, 1 << 15)
    local = [ip for ip, d, _ in routes if d == 32][0]
    specs = [dict(c[1], pair=((local, 80), (0xC6130001, 1024))) for c in TG.ip_option_cases()[:9]]
    b = S.build(specs, layout="packed", slot=128)
    ref = O.classify(O.MODE_CNET, np.concatenate([b["slab"], np.zeros(4096, np.uint8)]), 9, stride=128, tables4=t4,
                     tables6=t6, spec_burst=256, spec_state=np.array([0], np.uint16))
    plain = np.array([s["ihl"] == 5 for s in specs])
    assert (ref["ptype"][plain] & 0xFFFF == 0x111).all() and (ref["ptype"][~plain] & 0xFFFF == 0x131).all()
    assert 0x131 not in L.IP4_INPUT_TYPES and 0x111 in L.IP4_INPUT_TYPES
    assert (ref["nh"][plain] >> 24 == 2).all() and (ref["nh"][~plain] == 0xFFFFFFFF).all()
    assert (ref["rxmeta"] & 0xFFFF == b["rxmeta"]).all()


@pytest.mark.parametrize("layout", [dict(layout="packed", slot=128), dict(layout="offsets", align=1), dict(layout="umem")],
                         ids=["packed", "odd", "umem"])
def test_ip_options_in_front_of_tcp(tables, layout):
    _, tcbs = tables
    cases = TG.ip_option_cases()
    b = S.build([c[1] for c in cases], **layout)
    assert sorted(set((b["rxmeta"] >> 7).tolist())) == [20, 24, 60] and (b["rxmeta"] & 0x7F == 14).all()
    # the frames are what tcp_input accepts: the header checksum covers the options, the TCP header is found behind them
    ent = np.array([(addr_net(S.PAIR[0][0]), 0, port_net(S.PAIR[0][1]), 0, 0)], L.ENTRY_DT)
    t = T.tcp_input_ref(b["slab"], 65, b["rxmeta"], ent, sel=np.ones(65, np.uint8), stride=b["stride"], offsets=b["offsets"],
                        data_off=b["data_off"])
    assert (t["l4edge"] == T.E_SEG).all() and (t["seg"] == b["seg"]).all()
    for i in (0, 1, 2):
        f = S.frame_bytes(cases[i][1])
        hl = 4 * cases[i][1]["ihl"]
        assert S._fold(f[14:14 + hl]) == 0xFFFF and f[14] == 0x40 | hl // 4 and len(f) == 14 + hl + 32
    v, o = host_twin(tcbs, cases, 1000, layout)
    TG.ip_option_check(v, o)

"""tests/golden/tcp_options_ref.npz (tools/gen_tcp_options_golden.py): what the
compiled reference's tcp_do_options, tcp_send_options, tcp_header_prediction
and sequence comparisons returned, and the frames, TCBs and expected stage
outputs the host and GPU tests make from the recording.  Nothing here computes
an expectation: every expected value is a recorded one, rearranged."""
from __future__ import annotations

import os

import numpy as np

import tcpseg_ref as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("tcp_options_ref.npz", "tcp_predict_ref.npz")       # the second only if the generator had to split
LIMIT = 64 * 1024
P_CLASSES = ("last_byte", "last_two", "mid_len", "mss", "wscale", "ts_ack", "ts_ecr_now", "ts_len", "eol_garbage",
             "nops40", "unknown_edge", "len1", "seeded", "uniform", "pred_opts")
H_CLASSES = ("ack_edge", "cwnd_edge", "len_edge", "ts_edge", "las_edge", "no_ts", "seeded")
WND = 1024                  # the window field of every parse vector's frame
PARSE_TCB = dict(S.TCB_ZERO, state=2, flags=1)       # LISTEN: parsed, then SLOW
_cache = {}


def load() -> dict:
    if not _cache:
        for f in FILES:
            p = os.path.join(GOLD, f)
            if os.path.exists(p):
                with np.load(p, allow_pickle=False) as z:
                    _cache.update({k: z[k] for k in z.files})
    return _cache


def sizes() -> dict:
    return {f: os.path.getsize(os.path.join(GOLD, f)) for f in FILES if os.path.exists(os.path.join(GOLD, f))}


def p_opts(G, i: int) -> bytes:
    return G["p_data"][int(G["p_off"][i]):int(G["p_off"][i + 1])].tobytes()


def p_expect(G, i: int):
    """None where the reference returned -1, else the opt fields it left
    (ts_val, ts_ecr, mss, sflags | req_scale)."""
    if G["p_rc"][i] != 0:
        return None
    return int(G["p_ts_val"][i]), int(G["p_ts_ecr"][i]), int(G["p_mss"][i]), int(G["p_sflags"][i]) | int(G["p_scale"][i])


def parse_cases(G, now_idx: int):
    """The parse vectors recorded with nows[now_idx]: (indices, [(tcb, spec)]).
    Each frame carries the recorded tail byte as its one byte of payload."""
    idx = np.nonzero(G["p_now"] == now_idx)[0]
    cases = [(dict(PARSE_TCB, max_mss=int(G["p_max_mss"][i])),
              dict(seq=7, ack=9, wnd=WND, flags=int(G["p_flags"][i]), opts=p_opts(G, i), payload=bytes([int(G["p_tail"][i])])))
             for i in idx]
    return idx, cases


def parse_check(G, idx, verdict, opt, where: str):
    """BADOPT exactly where the reference returned -1; where it returned 0, the
    opt record is the recorded fields (and the window, which the parse leaves)."""
    for k, i in enumerate(idx):
        want, v = p_expect(G, i), int(verdict[k]) & S.VMASK
        got = tuple(int(x) for x in opt[k])
        if want is None:
            assert v == S.BADOPT and got == (0, 0, 0, 0, 0), f"{where}: parse vector {i} ({p_opts(G, i).hex()}): {S.NAMES[v]} {got}, the reference returned -1"
        else:
            assert v == S.SLOW and got == (want[0], want[1], WND, want[2], want[3]), \
                f"{where}: parse vector {i} ({p_opts(G, i).hex()} tail {G['p_tail'][i]:#x}): {S.NAMES[v]} {got}, the reference left {want}"


def h_tcb(G, j: int) -> dict:
    t = dict(S.TCB_ZERO, state=S.ESTABLISHED, flags=1)
    t.update({c: int(x) for c, x in zip(G["h_tcb_cols"].tolist(), G["h_tcb"][j])})
    return t


def h_spec(G, j: int) -> dict:
    """The segment of prediction vector j: its option bytes are its parse
    vector's, its payload starts with that vector's tail byte."""
    seq, ack, wnd, flags, plen = (int(x) for x in G["h_seg"][j])
    p = int(G["h_parse"][j])
    opts = p_opts(G, p) if p >= 0 else b""
    payload = (bytes([int(G["p_tail"][p])]) if p >= 0 else b"\0") + bytes(plen - 1) if plen else b""
    return dict(seq=seq, ack=ack, wnd=wnd, flags=flags, opts=opts, payload=payload)


def pred_cases(G, now_idx: int):
    idx = np.nonzero(G["h_now"] == now_idx)[0]
    return idx, [(h_tcb(G, j), h_spec(G, j)) for j in idx]


def h_verdict(G, j: int) -> int:
    """The stage's verdict for prediction vector j: the recorded branch and
    timestamp outcome -- or SLOW for the few hand-built edges that fail the
    (restated) entry test, where cnet_tcp_input would not have called
    tcp_header_prediction at all."""
    if not G["h_entry"][j]:
        return S.SLOW
    return(S.PRED_NONE, S.PRED_ACK, S.PRED_DATA)[int(G["h_branch"][j])] | (S.TS_UPDATE if G["h_ts"][j] else 0)


def pred_check(G, idx, verdict, opt, where: str):
    """The recorded branch and timestamp outcome, and the recorded parse of the
    segment's options."""
    for k, j in enumerate(idx):
        got, want = int(verdict[k]) & ~S.FIRST, h_verdict(G, j)
        assert got == want, (f"{where}: prediction vector {j} ({G['h_cls_names'][G['h_cls'][j]]}): verdict {got:#x}, "
                             f"the reference took {want:#x}")
        p = int(G["h_parse"][j])
        if p >= 0:
            e = p_expect(G, p)
            assert (int(opt[k]["ts_val"]), int(opt[k]["ts_ecr"]), int(opt[k]["mss"]), int(opt[k]["sflags"])) == e, (where, j)


# ---- IP options in front of the TCP header -----------------------------------
def ip_option_cases():
    """65 pure ACKs with a timestamp, IHL 5, 6 and 15 mixed: the options start at
    L2 + L3 + 20 with L3 up to 60, so CNDP_RXMETA_L3's upper bits matter."""
    est = dict(S.TCB_ZERO, rcv_nxt=1000, snd_una=5000, snd_nxt=6000, snd_max=6000, snd_wnd=8192, snd_cwnd=10000, ts_recent=500,
               last_ack_sent=900, rcv_space=100, max_mss=1460, state=S.ESTABLISHED, snd_scale=3, flags=1)
    return [(est, dict(seq=1000, ack=5001 + i, wnd=1024, flags=S.ACK, ihl=(5, 6, 15)[i % 3],
                       opts=bytes([1, 1]) + S.ts_opt(500 + i, 77 + i))) for i in range(65)]


def ip_option_check(verdict, opt):
    assert ((verdict & S.VMASK) == S.PRED_ACK).all(), verdict
    assert ((verdict[1:] & S.TS_UPDATE) == 0).all() and verdict[0] & S.TS_UPDATE       # ts_val == ts_recent only in frame 0
    assert opt["ts_val"].tolist() == [500 + i for i in range(65)] and opt["ts_ecr"].tolist() == [77 + i for i in range(65)]
    assert (opt["wnd"] == 8192).all() and (opt["sflags"] == S.TS_PRESENT).all() and (opt["mss"] == 0).all()

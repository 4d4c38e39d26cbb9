"""Python restatement of the TCP option parse and header-prediction triage for
the tcp_segment tests (include/cndp_tcb.h), written from the reference's text:
cnet_tcp_input from "Segment Arrives" on (lib/cnet/tcp/cnet_tcp.c:3425-3482: no
TCB, TCPS_CLOSED, the window scaling, tcp_do_options, the header-prediction entry
test), tcp_do_options itself (:1179-1279, byte by byte, quirks included) and the
tests inside tcp_header_prediction (:3214-3281).  Independent of tcb.c and of the
kernels; the bounded view is l4_ref's, the segment record tcp_ref's.

Also here: a builder of TCP frames with arbitrary option bytes (valid checksums,
so they pass classify -> udp_input -> tcp_input) and the seeded random cases the
host and GPU tests share."""
from __future__ import annotations

import numpy as np

from l4_ref import View
from tcp_ref import E_SEG, SEG_DT, SYN_FIN_CNT

OPT_DT = np.dtype([("ts_val", "<u4"), ("ts_ecr", "<u4"), ("wnd", "<u4"), ("mss", "<u2"), ("sflags", "<u2")])
NONE, RESET, CLOSED, BADOPT, SLOW, PRED_ACK, PRED_DATA, PRED_NONE = range(8)
NAMES = ("NONE", "RESET", "CLOSED", "BADOPT", "SLOW", "PRED_ACK", "PRED_DATA", "PRED_NONE")
TS_UPDATE, FIRST, VMASK = 0x40, 0x80, 0x0F
FIN, SYN, RST, PSH, ACK, URG = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
HDR_PREDIC = SYN | FIN | RST | URG | ACK
TS_PRESENT, MSS_PRESENT, WS_PRESENT, SACK_PERMIT = 0x8000, 0x4000, 0x2000, 0x1000
EOL, NOP, O_MSS, O_WS, O_SACK_OK, O_SACK, O_TS = 0, 1, 2, 3, 4, 5, 8
CLOSED_STATE, ESTABLISHED = 1, 5
M32 = 0xFFFFFFFF
TCB_ZERO = dict(rcv_nxt=0, snd_una=0, snd_nxt=0, snd_max=0, snd_wnd=0, snd_cwnd=0, ts_recent=0, last_ack_sent=0,
                rcv_space=0, max_mss=0, state=0, snd_scale=0, flags=0)


def s32(x: int) -> int:
    """(int32_t)x of a 32-bit difference."""
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def do_options(rd, optlen: int, flags: int, max_mss: int, now: int):
    """tcp_do_options.  rd(k) = opts[k], whatever k.  None when it returns -1,
    else (ts_val, ts_ecr, mss, sflags | req_scale)."""
    ts_val = ts_ecr = mss = sflags = scale = 0
    opts, opt_end = 0, optlen
    while opts < opt_end:
        kind = rd(opts)
        if kind == EOL:
            break
        if kind == NOP:
            opts += 1
            continue
        if kind == O_MSS:
            if rd(opts + 1) + opts > opt_end:
                return None
            if rd(opts + 1) == 4 and flags & SYN:
                mss = min(rd(opts + 2) << 8 | rd(opts + 3), max_mss)
                sflags |= MSS_PRESENT
        elif kind == O_WS:
            if rd(opts + 1) + opts > opt_end:
                return None
            if rd(opts + 1) == 3 and flags & SYN:
                scale = min(rd(opts + 2), 14)
                sflags |= WS_PRESENT
        elif kind == O_SACK_OK:
            if rd(opts + 1) + opts > opt_end:
                return None
            if rd(opts + 1) == 2:
                sflags |= SACK_PERMIT
        elif kind == O_TS:
            if rd(opts + 1) + opts > opt_end:
                return None
            if rd(opts + 1) == 10:
                ts_val = int.from_bytes(bytes(rd(opts + 2 + k) for k in range(4)), "big")
                ts_ecr = int.from_bytes(bytes(rd(opts + 6 + k) for k in range(4)), "big") if flags & ACK else 0
                sflags |= TS_PRESENT
                if ts_ecr != 0 and s32(now - ts_ecr) < 0:
                    ts_ecr = 0
        if rd(opts + 1) == 0:
            return None
        opts += rd(opts + 1)
    return ts_val, ts_ecr, mss, sflags | scale


def predic_entry(tcb, flags: int, sq: int, wnd: int, sflags: int, ts_val: int) -> bool:
    """The header-prediction entry test, inline in cnet_tcp_input (:3473-3482);
    wnd is the window after scaling."""
    ts = sflags & TS_PRESENT
    return bool(tcb["state"] == ESTABLISHED and (flags & HDR_PREDIC) == ACK
                and (not ts or s32(ts_val - tcb["ts_recent"]) >= 0)
                and sq == tcb["rcv_nxt"] and wnd and wnd == tcb["snd_wnd"] and tcb["snd_nxt"] == tcb["snd_max"])


def segment_one(tcb, seg, rd, now: int):
    """One segment against its PCB's TCB (a dict of struct cndp_tcb's fields, or
    None): (verdict | TS_UPDATE, opt tuple)."""
    zero = (0, 0, 0, 0, 0)
    if tcb is None:
        return RESET, zero
    if tcb["state"] == CLOSED_STATE:
        return CLOSED, zero
    flags, wnd = int(seg["flags"]), int(seg["wnd"])
    if not flags & SYN:
        wnd = (wnd << (tcb["snd_scale"] & 31)) & M32
    ts_val = ts_ecr = mss = sflags = 0
    if int(seg["offset"]) > 20:
        r = do_options(rd, int(seg["offset"]) - 20, flags, tcb["max_mss"], now)
        if r is None:
            return BADOPT, zero
        ts_val, ts_ecr, mss, sflags = r
    opt = (ts_val, ts_ecr, wnd, mss, sflags)
    sq, ak, ln = int(seg["seq"]), int(seg["ack"]), int(seg["len"])
    ts = sflags & TS_PRESENT
    if not predic_entry(tcb, flags, sq, wnd, sflags, ts_val):
        return SLOW, opt
    upd = TS_UPDATE if ts and s32(ts_val - tcb["ts_recent"]) <= 0 and s32(tcb["last_ack_sent"] - sq) < 0 else 0
    if ln == 0:
        if s32(ak - tcb["snd_una"]) > 0 and s32(ak - tcb["snd_max"]) <= 0 and tcb["snd_cwnd"] >= tcb["snd_wnd"]:
            return PRED_ACK | upd, opt
    elif ak == tcb["snd_una"] and tcb["flags"] & 1 and ln <= tcb["rcv_space"]:
        return PRED_DATA | upd, opt
    return PRED_NONE | upd, opt


def tcp_segment_ref(slab, n, rxmeta, tcbs, pcb, seg, now, l4edge=None, sel=None, stride=0, offsets=None,
                    data_off=0, stats=None) -> dict:
    """The stage's outputs for one batch.  tcbs[i] = PCB index i's TCB or None;
    its length is the table's capacity."""
    view = View(np.asarray(slab, np.uint8))
    out = {"opt": np.zeros(n, OPT_DT), "verdict": np.zeros(n, np.uint8),
           "stats": np.zeros(8, np.uint64) if stats is None else np.array(stats, np.uint64)}
    seen = set()
    for i in range(n):
        p = int(pcb[i])
        taken = (bool(sel[i]) if sel is not None else int(l4edge[i]) == E_SEG) and p < len(tcbs)
        v = NONE
        if taken:
            rx = int(rxmeta[i])
            base = (int(offsets[i] if offsets is not None else i * stride) + data_off + (rx & 0x7F)
                    + ((rx >> 7) & 0x1FF) + 20)
            v, opt = segment_one(tcbs[p], seg[i], lambda k, base=base: int(view.rd(base + k, 1)[0]), now)
            out["opt"][i] = opt
            if p not in seen:
                seen.add(p)
                v |= FIRST
        out["verdict"][i] = v
        out["stats"][v & VMASK] += 1
    return out


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
PAIR = ((0x0A040001, 80), (0xC6120001, 40000))


def _fold(b: bytes) -> int:
    b += b"\0" * (len(b) & 1)
    c = sum(int.from_bytes(b[k:k + 2], "big") for k in range(0, len(b), 2))
    while c >> 16:
        c = (c >> 16) + (c & 0xFFFF)
    return c


def frame_bytes(spec: dict) -> bytes:
    """Ethernet + IPv4 + TCP for one spec: pair, seq, ack, wnd, flags, opts (any
    bytes, a multiple of 4, at most 40), payload (bytes), urp, bad_cksum, ihl
    (5..15, default 5: the words past 5 are NOP IP options, and the header
    checksum covers the whole header)."""
    (dst, dport), (src, sport) = spec.get("pair", PAIR)
    opts, payload = bytes(spec.get("opts", b"")), bytes(spec.get("payload", b""))
    assert len(opts) % 4 == 0 and len(opts) <= 40
    tcp = bytearray(sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + (spec["seq"] & M32).to_bytes(4, "big")
                    + (spec["ack"] & M32).to_bytes(4, "big") + bytes([(5 + len(opts) // 4) << 4, spec["flags"]])
                    + (spec["wnd"] & 0xFFFF).to_bytes(2, "big") + b"\0\0"
                    + (spec.get("urp", 0) & 0xFFFF).to_bytes(2, "big") + opts + payload)
    ihl = spec.get("ihl", 5)
    assert 5 <= ihl <= 15
    ip = bytearray(20) + bytes([1]) * (4 * ihl - 20)
    ip[0], ip[8], ip[9] = 0x40 | ihl, 64, 6
    ip[2:4] = (4 * ihl + len(tcp)).to_bytes(2, "big")
    ip[12:16], ip[16:20] = src.to_bytes(4, "big"), dst.to_bytes(4, "big")
    ip[10:12] = ((~_fold(bytes(ip))) & 0xFFFF).to_bytes(2, "big")
    c = (~_fold(bytes(ip[12:20]) + bytes([0, 6]) + len(tcp).to_bytes(2, "big") + bytes(tcp))) & 0xFFFF
    if spec.get("bad_cksum"):      # tcp_input drops it: the frame never reaches the SEGMENT edge
        c ^= 0x5555
    tcp[16:18] = (c or 0xFFFF).to_bytes(2, "big")
    return bytes.fromhex("020000000001020000000002") + b"\x08\x00" + bytes(ip) + bytes(tcp)


def seg_of(spec: dict) -> tuple:
    """struct cndp_tcp_seg as tcp_input leaves it for frame_bytes(spec)."""
    fl = spec["flags"] & 0x3F
    return (spec["seq"] & M32, spec["ack"] & M32, spec["wnd"] & 0xFFFF, spec.get("urp", 0) & 0xFFFF,
            (len(spec.get("payload", b"")) + SYN_FIN_CNT[fl & 3]) & 0xFFFF, fl, 20 + len(spec.get("opts", b"")))


def build(specs, layout: str = "offsets", slot: int = 128, align: int = 1) -> dict:
    """The frames of `specs` in one slab: layout "packed" (slot-byte slots),
    "umem" (2 KiB frames, data at +256) or "offsets" (end to end, each start
    rounded up to `align`; the slab ends with the last frame's last byte).
    Returns slab, offsets (or None), stride, data_off, rxmeta and seg, as numpy."""
    frames = [frame_bytes(s) for s in specs]
    n = len(frames)
    data_off, stride = 0, 0
    if layout == "packed":
        stride, offs, total = slot, np.arange(n, dtype=np.int64) * slot, n * slot
        assert all(len(f) <= slot for f in frames)
    elif layout == "umem":
        stride, data_off, offs, total = 2048, 256, np.arange(n, dtype=np.int64) * 2048, n * 2048
    else:
        offs, at = np.zeros(n, np.int64), 0
        for i, f in enumerate(frames):
            at = (at + align - 1) // align * align
            offs[i] = at
            at += len(f)
        total = at
    slab = np.zeros(max(total, 1), np.uint8)
    for i, f in enumerate(frames):
        o = int(offs[i]) + data_off
        slab[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return {"slab": slab, "offsets": offs.astype(np.uint64) if layout == "offsets" else None, "stride": stride,
            "data_off": data_off, "rxmeta": np.array([14 | 4 * s.get("ihl", 5) << 7 for s in specs], np.uint32).reshape(n),
            "seg": np.array([seg_of(s) for s in specs], SEG_DT).reshape(n), "n": n}


def to_frames(b: dict, device):
    """build()'s result as a cndp_amd.pktgen.Frames on `device`."""
    import torch
    from cndp_amd import pktgen
    offs = torch.from_numpy(b["offsets"].astype(np.int64)).to(device) if b["offsets"] is not None else None
    return pktgen.Frames(torch.from_numpy(b["slab"]).to(device), b["n"], stride=b["stride"], offsets=offs,
                         data_off=b["data_off"])


# ---------------------------------------------------------------------------
# option strings and random cases
# ---------------------------------------------------------------------------
def pad4(b: bytes, fill: int = NOP) -> bytes:
    return b + bytes([fill]) * (-len(b) % 4)


def ts_opt(val: int, ecr: int) -> bytes:
    return bytes([O_TS, 10]) + (val & M32).to_bytes(4, "big") + (ecr & M32).to_bytes(4, "big")


def _u32(rng) -> int:
    """A sequence-space value; one in six sits just under 2^32."""
    if rng.random() < 1 / 6:
        return (0xFFFFFFFF - int(rng.integers(0, 2000))) & M32
    return int(rng.integers(0, 1 << 32))


def _random_opts(rng, syn: bool, ts_val: int, now: int) -> bytes:
    r = rng.random()
    ecr = (now - int(rng.integers(0, 1000))) & M32 if rng.random() < 0.8 else (now + int(rng.integers(1, 1000))) & M32
    if r < 0.22:
        return b""
    if r < 0.55 and not syn:
        return bytes([NOP, NOP]) + ts_opt(ts_val, ecr)
    if r < 0.55:
        o = b""
        if rng.random() < 0.9:
            o += bytes([O_MSS, 4]) + int(rng.choice([536, 1460, 9000, 65535])).to_bytes(2, "big")
        if rng.random() < 0.7:
            o += bytes([NOP, O_WS, 3, int(rng.choice([0, 7, 14, 15, 200]))])
        if rng.random() < 0.6:
            o += bytes([O_SACK_OK, 2])
        if rng.random() < 0.7:
            o += ts_opt(ts_val, ecr)
        if rng.random() < 0.2:
            o += bytes([O_MSS, 4]) + int(rng.integers(0, 65536)).to_bytes(2, "big")
        return pad4(o[:40], EOL if rng.random() < 0.5 else NOP)[:40]
    if r < 0.70:      # anything at all
        return rng.integers(0, 256, 4 * int(rng.integers(1, 11)), dtype=np.uint8).tobytes()
    if r < 0.80:      # small kinds and lengths: long walks, length 1, unknown kinds
        return rng.choice(np.array([0, 1, 1, 1, 2, 3, 4, 5, 8, 10, 30], np.uint8), 4 * int(rng.integers(1, 11))).tobytes()
    if r < 0.90:      # a well-formed timestamp, then a known kind in the header's last byte or two
        tail = bytes([int(rng.choice([O_MSS, O_WS, O_SACK_OK, O_TS, O_SACK, 99]))])
        if rng.random() < 0.5:
            tail += bytes([int(rng.choice([0, 1, 2, 3, 4, 10]))])
        return ts_opt(ts_val, ecr) + bytes([NOP] * (2 - len(tail))) + tail
    if r < 0.95:      # a timestamp of the wrong length, an unknown kind walking past the end
        return pad4(bytes([O_TS, 8]) + (ts_val & M32).to_bytes(4, "big") + bytes([NOP, NOP, O_SACK, 200]))
    return bytes([NOP] * (4 * int(rng.integers(1, 11))))


def random_case(rng, now: int):
    """(tcb dict or None, frame spec): an established connection and a segment
    that header prediction would take, then knocked off that path in one or two
    places, with option strings from well-formed to arbitrary bytes."""
    scale = int(rng.choice([0, 0, 2, 7, 8, 14]))
    w16 = int(rng.integers(1, 65536))
    una = _u32(rng)
    flight = int(rng.choice([0, 1, 1460, 5000, 40000]))
    t = dict(TCB_ZERO, rcv_nxt=_u32(rng), snd_una=una, snd_max=(una + flight) & M32, snd_wnd=(w16 << scale) & M32,
             ts_recent=_u32(rng), rcv_space=int(rng.choice([0, 1, 30, 1460, 65535])),
             max_mss=int(rng.choice([536, 1460, 9000])), state=ESTABLISHED, snd_scale=scale, flags=1)
    t["snd_nxt"] = t["snd_max"]
    t["snd_cwnd"] = (t["snd_wnd"] + int(rng.integers(0, 3000))) & M32
    t["last_ack_sent"] = (t["rcv_nxt"] - int(rng.choice([0, 1, 1460]))) & M32
    spec = dict(seq=t["rcv_nxt"], wnd=w16, flags=ACK | (PSH if rng.random() < 0.3 else 0))
    ts_val = (t["ts_recent"] + int(rng.choice([0, 0, 1, 1000]))) & M32
    if rng.random() < 0.5:      # a pure ACK
        spec["ack"] = (una + int(rng.integers(1, flight + 1))) & M32 if flight else una
        spec["payload"] = b""
    else:
        plen = int(rng.choice([1, 7, 30]))
        spec["ack"] = una
        spec["payload"] = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
    # off the fast path: one term at a time
    k = rng.random()
    if k < 0.03:
        t["state"] = int(rng.choice([0, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]))
    elif k < 0.06:
        spec["flags"] = int(rng.choice([SYN, SYN | ACK, FIN | ACK, RST, RST | ACK, ACK | URG, 0, 0x3F]))
    elif k < 0.08:
        spec["seq"] = (spec["seq"] + int(rng.choice([1, -1]))) & M32
    elif k < 0.10:
        spec["wnd"] = (w16 % 65535) + 1 if w16 != (w16 % 65535) + 1 else 7
    elif k < 0.12:
        t["snd_wnd"] = 0
        spec["wnd"] = 0
    elif k < 0.14:
        t["snd_nxt"] = (t["snd_max"] - 1) & M32
    elif k < 0.16:
        ts_val = (t["ts_recent"] - int(rng.choice([1, 1000]))) & M32
    elif k < 0.19:
        spec["ack"] = int(rng.choice([una, (t["snd_max"] + 1) & M32, (una - 1) & M32]))
    elif k < 0.21:
        t["snd_cwnd"] = (t["snd_wnd"] - 1) & M32 if t["snd_wnd"] else 0
    elif k < 0.23:
        t["flags"] = 0
    elif k < 0.25:
        t["rcv_space"] = max(len(spec["payload"]) - 1, 0)
    spec["opts"] = _random_opts(rng, bool(spec["flags"] & SYN), ts_val, now)
    if rng.random() < 0.04:
        t = None
    return t, spec

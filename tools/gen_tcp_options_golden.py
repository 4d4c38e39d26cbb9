#!/usr/bin/env python3
"""Generate tests/golden/tcp_options_ref.npz (and tcp_predict_ref.npz when one
file would pass 64 KiB): what the reference's own tcp_do_options,
tcp_send_options, tcp_header_prediction and sequence / timestamp comparisons
(lib/cnet/tcp/cnet_tcp.c, cnet_tcp.h) give for the inputs below.

    python tools/gen_tcp_options_golden.py --ref /path/to/cndp

A driver of our own (below) is compiled in a temporary directory; it reaches the
reference by `#include "cnet_tcp.c"` through an -I path, which makes the file's
static functions callable, and runs once normally and once more under
-fsanitize=address,undefined (the outputs must be equal).  A few stand-in
headers, also our own text, take the place of libbsd and of the reference's
generated build configuration.  Only data is written.

Every vector is labelled by how its input was built (cls), not by the answer.

Parse (p_*): option bytes (0, 4, .., 40 of them), the one byte behind them
(p_tail), TCP flags, max_mss and now (one of three values).  The driver copies
options and tail into a zeroed heap buffer of optlen + 1 + 16 bytes and runs
every vector twice, with the bytes from opt_end + 1 on filled with 0x00 and with
0xFF: the generator fails if any answer differs -- the parser reads at most one
byte past the header.  Recorded: p_rc, p_ts_val, p_ts_ecr, p_mss, p_sflags,
p_scale.

Send (s_*): s_tf (the four attributes tcp_send_options reads, in the product's
coding: REQ_SCALE 1, RCVD_SCALE 2, REQ_TSTAMP 4, RCVD_TSTAMP 8; the driver maps
them to the reference's TCBF_* by name), s_flags, s_set (the index into
s_max_mss, s_scale, s_ts_recent, s_now, s_iss, s_nxt0).  Recorded: s_optlen, the
bytes written (s_bytes, 20 per vector, 0xEE where nothing was written) and
tcb->snd_nxt afterwards (s_nxt).

Comparisons (c_*): pairs (c_a, c_b) and c_res, bit k = the k-th of CMP_NAMES.

Prediction (h_*): a TCB (h_tcb, columns TCB_COLS), a segment (h_seg: seq, ack,
wnd as on the wire, flags, payload length) and h_parse, the index of the parse
vector that holds its option bytes (-1: none; its tail byte is the payload's
first byte, its now is the call's).  The entry test in front of the routine is
inline in cnet_tcp_input and cannot be called, so it is restated
(tcpseg_ref.predic_entry, on the compiled parse's results): seeded cases are
kept only where it holds.  A hand-built edge where it fails (ts_val =
ts_recent - 1: the entry test wants ts_val >= ts_recent) is kept with
h_entry = 0; cnet_tcp_input would not have called the routine for it, so the
stage's answer there is SLOW and the recorded branch is for the record only.
A segment without payload has options whose parse does not depend on the tail
byte (checked here), so its frame may sit anywhere in a slab.  Recorded:
h_branch (0 neither, 1 ack, 2 data: the deltas of S_ack_predicted /
S_data_predicted) and h_ts (ts_recent taken: a sentinel in ts_recent_age was
overwritten).
"""
import argparse
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tcpseg_ref as S  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LIMIT = 64 * 1024
NOWS = (3, 0xFFFFFFFB, 0x5A5A1234)           # near 0, near 2^32, anywhere
M32 = 0xFFFFFFFF
CMP_NAMES = ("seqLT", "seqLEQ", "seqGT", "seqGEQ", "seqEQ", "seqNE", "tstampLT", "tstampLEQ", "tstampGEQ")
TCB_COLS = ("rcv_nxt", "snd_una", "snd_nxt", "snd_max", "snd_wnd", "snd_cwnd", "ts_recent", "last_ack_sent",
            "rcv_space", "max_mss", "snd_scale")
PROPER = {2: 4, 3: 3, 4: 2, 8: 10, 5: 10, 99: 4}
N_SEEDED_PRED, N_SEEDED_SYN, N_UNIFORM = 600, 120, 120

STANDINS = {
    "cne_build_config.h": "/* stand-in: the settings the driver needs are defined in front of its include */\n",
    "bsd/bsd.h": "#include <bsd/string.h>\n",
    "bsd/string.h": "#ifndef STANDIN_BSD_STRING_H\n#define STANDIN_BSD_STRING_H\n#include <stddef.h>\n#include <string.h>\n"
                    "size_t strlcpy(char *dst, const char *src, size_t n);\n"
                    "size_t strlcat(char *dst, const char *src, size_t n);\n#endif\n",
    "bsd/sys/queue.h": "#include <sys/queue.h>\n",
    "bsd/bitstring.h": "#include <bsd/sys/bitstring.h>\n",
    "bsd/sys/bitstring.h": "#ifndef STANDIN_BITSTRING_H\n#define STANDIN_BITSTRING_H\n#include <stdlib.h>\n"
                           "typedef unsigned char bitstr_t;\n"
                           "#define bitstr_size(n) (((n) + 7) >> 3)\n"
                           "#define bit_alloc(n) ((bitstr_t *)calloc(bitstr_size(n), 1))\n"
                           "#define bit_test(b, i) ((b)[(i) >> 3] & (1 << ((i) & 7)))\n"
                           "#define bit_set(b, i) ((b)[(i) >> 3] |= (1 << ((i) & 7)))\n"
                           "#define bit_clear(b, i) ((b)[(i) >> 3] &= ~(1 << ((i) & 7)))\n#endif\n",
}

DRIVER = r"""
#include <sys/queue.h>
#ifndef TAILQ_FOREACH_SAFE
#define TAILQ_FOREACH_SAFE(var, head, field, tvar) \
    for ((var) = TAILQ_FIRST((head)); (var) && ((tvar) = TAILQ_NEXT((var), field), 1); (var) = (tvar))
#endif
#define CNET_NUM_TCBS 64
#define CNET_ENABLE_IP6 0
#include "cnet_tcp.c"
#include <stdio.h>
#include <stdarg.h>

CNE_DEFINE_PER_THREAD(stk_t *, stk);

int cne_log(uint32_t level, const char *func, int line, const char *format, ...)
{
    (void)level, (void)func, (void)line, (void)format;
    return 0;
}
void cnet_add_instance(const char *name, int pri, cfunc_t create, cfunc_t destroy)
{
    (void)name, (void)pri, (void)create, (void)destroy;
}
void cnet_drop_acked_data(struct chnl_buf *cb, int32_t acked) { (void)cb, (void)acked; }
size_t strlcpy(char *dst, const char *src, size_t n)
{
    size_t k = strlen(src);
    if (n) {
        size_t c = k < n - 1 ? k : n - 1;
        memcpy(dst, src, c);
        dst[c] = 0;
    }
    return k;
}
size_t strlcat(char *dst, const char *src, size_t n)
{
    size_t d = strnlen(dst, n);
    return d == n ? n + strlen(src) : d + strlcpy(dst + d, src, n - d);
}

#define PAD 16
#define SENTINEL 0xA5A5A5A5u

int main(void)
{
    static struct stk_s stack;
    static struct tcp_stats stats;
    char tag;
    this_stk        = &stack;
    stack.tcp_stats = &stats;
    while (scanf(" %c", &tag) == 1) {
        struct seg_entry seg;
        struct pcb_entry pcb;
        struct tcb_entry tcb;
        struct chnl ch;
        memset(&seg, 0, sizeof(seg));
        memset(&pcb, 0, sizeof(pcb));
        memset(&tcb, 0, sizeof(tcb));
        memset(&ch, 0, sizeof(ch));
        seg.pcb = &pcb;
        pcb.tcb = &tcb;
        pcb.ch  = &ch;
        tcb.pcb = &pcb;
        if (tag == 'P') {
            unsigned optlen, flags, max_mss, now, fill, b;
            if (scanf("%u %u %u %u %u", &optlen, &flags, &max_mss, &now, &fill) != 5 || optlen > 40)
                return 1;
            uint8_t *buf = calloc(optlen + 1 + PAD, 1);
            for (unsigned k = 0; k < optlen + 1; k++) {
                if (scanf("%2x", &b) != 1)
                    return 1;
                buf[k] = (uint8_t)b;
            }
            memset(buf + optlen + 1, (int)fill, PAD);
            stack.tcp_now = now;
            tcb.max_mss   = (uint16_t)max_mss;
            seg.offset    = (uint8_t)(sizeof(struct cne_tcp_hdr) + optlen);
            seg.flags     = (uint8_t)flags;
            int rc        = tcp_do_options(&seg, buf);
            printf("%d %u %u %u %u %u\n", rc, seg.ts_val, seg.ts_ecr, seg.mss, seg.sflags, seg.req_scale);
            free(buf);
        } else if (tag == 'S') {
            unsigned tf, flags, scale, max_mss, ts_recent, now, iss, nxt;
            if (scanf("%u %u %u %u %u %u %u %u", &tf, &flags, &scale, &max_mss, &ts_recent, &now, &iss, &nxt) != 8)
                return 1;
            uint32_t *words = malloc(40);      /* the routine stores 32-bit words: an aligned buffer */
            uint8_t *out    = (uint8_t *)words;
            memset(out, 0xEE, 40);
            tcb.tflags = (tf & 1 ? TCBF_REQ_SCALE : 0) | (tf & 2 ? TCBF_RCVD_SCALE : 0) | (tf & 4 ? TCBF_REQ_TSTAMP : 0) |
                         (tf & 8 ? TCBF_RCVD_TSTAMP : 0);
            tcb.req_recv_scale = (uint8_t)scale;
            tcb.max_mss        = (uint16_t)max_mss;
            tcb.ts_recent      = ts_recent;
            tcb.snd_iss        = iss;
            tcb.snd_nxt        = nxt;
            stack.tcp_now      = now;
            int32_t optlen     = tcp_send_options(&tcb, out, (uint8_t)flags);
            printf("%d %u ", optlen, tcb.snd_nxt);
            for (int k = 0; k < 40; k++)
                printf("%02x", out[k]);
            printf("\n");
            free(words);
        } else if (tag == 'C') {
            unsigned a, b;
            if (scanf("%u %u", &a, &b) != 2)
                return 1;
            uint32_t x = a, y = b;
            printf("%d\n", (seqLT(x, y) ? 1 : 0) | (seqLEQ(x, y) ? 2 : 0) | (seqGT(x, y) ? 4 : 0) | (seqGEQ(x, y) ? 8 : 0) |
                               (seqEQ(x, y) ? 16 : 0) | (seqNE(x, y) ? 32 : 0) | (tstampLT(x, y) ? 64 : 0) |
                               (tstampLEQ(x, y) ? 128 : 0) | (tstampGEQ(x, y) ? 256 : 0));
        } else if (tag == 'H') {
            unsigned seq, ack, len, sflags, ts_val, ts_ecr, una, max, wnd, cwnd, ts_recent, las, space, now;
            if (scanf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u", &seq, &ack, &len, &sflags, &ts_val, &ts_ecr, &una, &max,
                      &wnd, &cwnd, &ts_recent, &las, &space, &now) != 14)
                return 1;
            seg.mbuf   = NULL;
            seg.seq    = seq;
            seg.ack    = ack;
            seg.len    = (uint16_t)len;
            seg.sflags = (uint16_t)sflags;
            seg.ts_val = ts_val;
            seg.ts_ecr = ts_ecr;
            tcb.snd_una = una;
            tcb.snd_nxt = tcb.snd_max = max;
            tcb.snd_wnd               = wnd;
            tcb.snd_cwnd              = cwnd;
            tcb.ts_recent             = ts_recent;
            tcb.ts_recent_age         = SENTINEL;
            tcb.last_ack_sent         = las;
            tcb.reassemble            = NULL;
            tcb.tflags                = 0;
            ch.ch_snd.cb_cc           = 0;
            ch.ch_rcv.cb_cc           = 0;
            ch.ch_rcv.cb_hiwat        = space;
            stack.tcp_now             = now;
            uint64_t a0 = stats.S_ack_predicted, d0 = stats.S_data_predicted;
            int rc = tcp_header_prediction(&seg, &tcb);
            printf("%d %d %d %u %d\n", (int)(stats.S_ack_predicted - a0), (int)(stats.S_data_predicted - d0),
                   tcb.ts_recent_age != SENTINEL, tcb.ts_recent, rc);
        } else
            return 1;
    }
    return 0;
}
"""


# ---------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------
def build_driver(ref: str, tmp: str, san: bool) -> str:
    for name, text in STANDINS.items():
        p = os.path.join(tmp, name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            f.write(text)
    src = os.path.join(tmp, "tcp_driver.c")
    with open(src, "w") as f:
        f.write(DRIVER)
    inc = [f"-I{tmp}"]
    for d, _, _ in sorted(os.walk(os.path.join(ref, "lib"))):
        inc.append(f"-I{d}")
    exe = os.path.join(tmp, "tcp_driver_san" if san else "tcp_driver")
    defs = ["-D_GNU_SOURCE", '-DCNE_VER_PREFIX="CNDP"', '-DCNE_VER_SUFFIX=""', "-DCNE_VER_YEAR=25", "-DCNE_VER_MONTH=8",
            "-DCNE_VER_MINOR=0", "-DCNE_VER_RELEASE=99"]
    # shift-base is left out: tcb_print_flags, which runs inside a CNE_DEBUG argument list, walks its
    # flag names with 1 << 31 on an int.  Its result is thrown away; every other check is fatal.
    opt = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=shift-base", "-fno-sanitize-recover=all"]
           if san else ["-O1"])
    subprocess.run(["gcc", *opt, "-std=gnu11", "-w", *defs, *inc, "-o", exe, src,
                    "-Wl,--unresolved-symbols=ignore-all", "-lpthread"], check=True)
    return exe


def run_driver(exe: str, lines) -> list:
    r = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), capture_output=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr.decode(errors="replace"))
        raise SystemExit(f"{exe}: exit {r.returncode}")
    out = r.stdout.decode().splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    return out


# ---------------------------------------------------------------------------
# vectors
# ---------------------------------------------------------------------------
def pv(cls, opts, tail, flags, max_mss=1460, now=NOWS[2]):
    opts = bytes(opts)
    assert len(opts) % 4 == 0 and len(opts) <= 40 and now in NOWS and 0 <= tail < 256
    return dict(cls=cls, opts=opts, tail=tail, flags=flags, max_mss=max_mss, now=now)


def parse_classes(rng) -> list:
    SYN, ACK = S.SYN, S.ACK
    v = []
    for kind in (2, 3, 4, 8, 5, 99):
        tails = sorted({0, 1, 2, PROPER[kind], 255})
        for t in tails:                                   # the kind is the header's last byte: its length is the tail
            v.append(pv("last_byte", [1, 1, 1, kind], t, SYN | ACK))
        for ln in tails:                                  # kind and length are the last two bytes
            for t in (0, 255):
                v.append(pv("last_two", [1, 1, kind, ln], t, SYN | ACK))
    val = [0x05, 0xB4, 0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x0E, 0x0F, 0x10]
    for kind in (2, 3, 4, 8):
        for ln in range(13):
            o = [1] * 12 + [kind, ln] + val + [1] * 14 + [4, 2]
            for fl in (SYN | ACK, ACK):
                v.append(pv("mid_len", o, 0, fl))
    for max_mss, mss in ((1460, 1459), (1460, 1460), (1460, 1461), (1460, 0), (1460, 65535), (0, 0), (0, 536), (65535, 65535)):
        for fl in (SYN, SYN | ACK, ACK):
            v.append(pv("mss", [2, 4, mss >> 8, mss & 255], 0, fl, max_mss=max_mss))
    for sc in (0, 14, 15, 255):
        for fl in (SYN, SYN | ACK, ACK, 0):
            v.append(pv("wscale", [3, 3, sc, 1], 0, fl))
    now = NOWS[2]
    for fl in (ACK, 0, SYN, SYN | ACK, S.PSH, S.RST, S.RST | ACK, S.FIN | ACK):
        for ecr in (now - 7, now + 7):
            v.append(pv("ts_ack", bytes([1, 1]) + S.ts_opt(0x01020304, ecr), 0, fl))
    for now in NOWS[:2]:
        for d in (0, 1, -1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1):
            v.append(pv("ts_ecr_now", bytes([1, 1]) + S.ts_opt(9, (now + d) & M32), 0, ACK, now=now))
        v.append(pv("ts_ecr_now", bytes([1, 1]) + S.ts_opt(9, 0), 0, ACK, now=now))
    body = bytes([0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77, 0x88])
    for fl in (ACK, SYN | ACK):
        v.append(pv("ts_len", bytes([8, 8]) + body[:6] + bytes([4, 2, 1, 1]), 0, fl))
        v.append(pv("ts_len", bytes([1, 1, 8, 8]) + body[:6] + bytes([8, 10]) + body + bytes([0, 0, 0, 0]), 0, fl))
        v.append(pv("ts_len", bytes([8, 12]) + body + bytes([1, 1, 4, 2, 1, 1]), 0, fl))
        v.append(pv("ts_len", bytes([1, 1, 8, 12]) + body, 0, fl))          # 2 + 12 = 14 > 12
        v.append(pv("ts_len", bytes([1, 1, 8, 10]) + body, 0, fl))          # 2 + 10 = 12
    for k in range(8):
        g = rng.integers(0, 256, 4 * (1 + k) - 1 - (k & 1) * 2, dtype=np.uint8).tobytes()
        v.append(pv("eol_garbage", (bytes([4, 2]) if k & 1 else b"") + bytes([0]) + g, int(g[0]), SYN | ACK))
    for t in (0, 1, 2, 3, 4, 8, 99, 255):
        v.append(pv("nops40", [1] * 40, t, ACK))
    for kind in (5, 99, 30, 254):
        for ln in (5, 6, 7):                               # from position 2 of 8: one short, exact, one past
            for last, t in ((1, 0), (4, 2), (4, 0), (kind, 3)):
                v.append(pv("unknown_edge", [1, 1, kind, ln, 1, 1, 1, last], t, ACK))
    for o in ([99, 1, 4, 2], [4, 1, 4, 2], [2, 1, 2, 4], [8, 1, 1, 1], [3, 1, 3, 3, 7, 1, 1, 1], [5, 1, 1, 0],
              [99, 1, 1, 1, 99, 1, 0, 0], [2, 1, 4, 5, 0xB4, 1, 1, 1], [8, 1, 10] + [7] * 8 + [1], [3, 1, 0, 0]):
        v.append(pv("len1", o, 0, SYN | ACK))
    # SYN-side strings of the GPU tests' own distribution, and uniformly random bytes
    for k in range(N_SEEDED_SYN):
        now = NOWS[k % 3]
        fl = SYN if k & 1 else SYN | ACK
        o = S._random_opts(rng, True, S._u32(rng), now)
        if o:
            v.append(pv("seeded", o, int(rng.integers(0, 256)), fl, max_mss=int(rng.choice([536, 1460, 9000])), now=now))
    for k in range(N_UNIFORM):
        o = rng.integers(0, 256, 4 * int(rng.integers(1, 11)), dtype=np.uint8).tobytes()
        v.append(pv("uniform", o, int(rng.integers(0, 256)), int(rng.integers(0, 64)),
                    max_mss=int(rng.choice([0, 536, 1460, 65535])), now=NOWS[k % 3]))
    return v


def pred_edges() -> list:
    """Hand-built prediction inputs: (tcb, spec) with spec["opts"]."""
    est = dict(S.TCB_ZERO, rcv_nxt=1000, snd_una=5000, snd_nxt=6000, snd_max=6000, snd_wnd=8192, snd_cwnd=10000,
               ts_recent=500, last_ack_sent=900, rcv_space=30, max_mss=1460, state=S.ESTABLISHED, snd_scale=3, flags=1)
    wrap = dict(est, snd_una=0xFFFFFF00, snd_nxt=0x100, snd_max=0x100)
    ack = dict(seq=1000, ack=5500, wnd=1024, flags=S.ACK, payload=b"", opts=b"")
    data = dict(seq=1000, ack=5000, wnd=1024, flags=S.ACK | S.PSH, payload=bytes(10), opts=b"")
    ts = lambda val: bytes([1, 1]) + S.ts_opt(val, 1)  # noqa: E731
    e = []
    for t in (est, wrap, dict(est, snd_una=0xFFFFFFFF, snd_nxt=0x7FF, snd_max=0x7FF),
              dict(est, snd_una=0x7FFFFFFF, snd_nxt=0x800003E8, snd_max=0x800003E8)):
        for a in (t["snd_una"] - 1, t["snd_una"], t["snd_una"] + 1, t["snd_max"] - 1, t["snd_max"], t["snd_max"] + 1,
                  t["snd_una"] + (1 << 31)):
            e.append(("ack_edge", t, dict(ack, ack=a & M32)))
            e.append(("ack_edge", t, dict(data, ack=a & M32)))
    for d in (-1, 0, 1):
        e.append(("cwnd_edge", dict(est, snd_cwnd=8192 + d), ack))
        e.append(("cwnd_edge", dict(est, snd_cwnd=8192 + d), data))
        e.append(("cwnd_edge", dict(est, snd_wnd=0xFFFF << 14, snd_scale=14, snd_cwnd=((0xFFFF << 14) + d) & M32),
                  dict(ack, wnd=0xFFFF)))
    for space in (30, 1, 0):
        for ln in (max(space - 1, 1), space, space + 1):
            if ln:
                e.append(("len_edge", dict(est, rcv_space=space), dict(data, payload=bytes(ln))))
                e.append(("len_edge", dict(est, rcv_space=space), dict(data, payload=bytes(ln), opts=ts(500))))
    for rec in (500, 0, 0xFFFFFFFF, 0x80000000):
        for d in (-1, 0, 1):
            for base in (ack, data):
                e.append(("ts_edge", dict(est, ts_recent=rec), dict(base, opts=ts((rec + d) & M32))))
    for seq in (1000, 0, 0xFFFFFFFF, 0x80000000):
        for d in (-1, 0, 1, 1 << 31):
            for base in (ack, data):
                e.append(("las_edge", dict(est, rcv_nxt=seq, last_ack_sent=(seq + d) & M32), dict(base, seq=seq, opts=ts(500))))
    for base in (ack, data):
        e.append(("no_ts", est, base))
        e.append(("no_ts", est, dict(base, opts=bytes([1, 1, 1, 1]))))
        e.append(("no_ts", est, dict(base, opts=bytes([4, 2, 1, 1]))))
        e.append(("no_ts", dict(est, last_ack_sent=999), dict(base, opts=bytes([8, 8, 0, 0, 1, 1, 1, 1]))))
    return e


CMP_DELTAS = (0, 1, -1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, -((1 << 31) - 1), -(1 << 31), -((1 << 31) + 1))


def cmp_pairs(rng) -> list:
    pairs = []
    for a in (0, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0x7FFFFFFE, 2, 0x12345678,
              0xFFFFF000, 0x80000FFF):
        for d in CMP_DELTAS:
            pairs.append((a, (a + d) & M32))
    for _ in range(200 - len(pairs)):
        a = int(rng.choice([0, 1 << 31, M32])) + int(rng.integers(-3, 4)) & M32
        pairs.append((a, (a + int(rng.choice(CMP_DELTAS)) + int(rng.integers(-1, 2))) & M32))
    return pairs


def hexline(v, fill: int) -> str:
    return (f"P {len(v['opts'])} {v['flags']} {v['max_mss']} {v['now']} {fill} " + (v["opts"] + bytes([v["tail"]])).hex())


def run_parse(exes, vecs) -> np.ndarray:
    """The compiled parse of `vecs`, n x 6 (rc, ts_val, ts_ecr, mss, sflags, scale);
    equal under both fills and both builds, or the generator stops."""
    outs = [run_driver(exe, [hexline(v, fill) for v in vecs]) for exe in exes for fill in (0x00, 0xFF)]
    for o in outs[1:]:
        bad = [i for i, (x, y) in enumerate(zip(outs[0], o)) if x != y]
        if bad:
            raise SystemExit(f"parse vector {bad[0]} ({vecs[bad[0]]}) depends on bytes past opt_end + 1 or on the build")
    return np.array([[int(x) for x in ln.split()] for ln in outs[0]], np.int64).reshape(len(vecs), 6)


# ---------------------------------------------------------------------------
# output
# ---------------------------------------------------------------------------
def write_npz(path: str, arrays: dict) -> int:
    """np.load-able, compressed, and the same bytes every time (no timestamps)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue(), compresslevel=9)
    return os.path.getsize(path)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("CNDP_REF"), help="a CNDP v25.08.0 source tree (or $CNDP_REF)")
    ap.add_argument("--out-dir", default=GOLD)
    a = ap.parse_args()
    if not a.ref:
        ap.error("--ref or $CNDP_REF is required")
    rng = np.random.default_rng(0x7C90)

    with tempfile.TemporaryDirectory() as tmp:
        exes = (build_driver(a.ref, tmp, False), build_driver(a.ref, tmp, True))

        # ---- prediction candidates first: their option strings are parse vectors too
        pvec = parse_classes(rng)
        cand = [("seeded", *S.random_case(rng, NOWS[2]), NOWS[2]) for _ in range(4 * N_SEEDED_PRED)]
        cand = [(c, t, s, now) for c, t, s, now in cand if t is not None and t["flags"] & 1]
        cand += [(c, t, dict(s), NOWS[2]) for c, t, s in pred_edges()]
        pred, n_seeded = [], 0
        for cls, t, spec, now in cand:
            if cls == "seeded" and n_seeded >= N_SEEDED_PRED:
                continue
            fl, pl, opts = spec["flags"] & 0x3F, bytes(spec["payload"]), bytes(spec["opts"])
            pidx, res = -1, (0, 0, 0, 0, 0, 0)
            if opts:
                pcls = "seeded" if cls == "seeded" else "pred_opts"
                if pl:
                    trial = [pv(pcls, opts, pl[0], fl, t["max_mss"], now)]
                else:       # no payload: the byte behind the options is whatever follows the frame
                    trial = [pv(pcls, opts, 0, fl, t["max_mss"], now), pv(pcls, opts, 2, fl, t["max_mss"], now)]
                r = run_parse(exes[:1], trial)
                pidx = len(pvec)
                pvec += trial
                if len(trial) == 2 and (r[0] != r[1]).any():
                    continue                                  # kept as parse vectors only
                res = tuple(int(x) for x in r[0])
            if res[0] != 0:
                continue
            wnd = spec["wnd"] if fl & S.SYN else (spec["wnd"] << (t["snd_scale"] & 31)) & M32
            entry = S.predic_entry(t, fl, spec["seq"] & M32, wnd, res[4], res[1])
            if not entry and cls == "seeded":
                continue
            n_seeded += cls == "seeded"
            pred.append(dict(cls=cls, tcb=t, spec=spec, pidx=pidx, now=now, sflags=res[4], ts_val=res[1], ts_ecr=res[2],
                             entry=int(entry)))

        # ---- parse
        P = run_parse(exes, pvec)
        # ---- send
        sets = [(1460, 7, 0x0A0B0C0D, 0x01020304, 0x11111111, 0x22222222)]
        for _ in range(3):
            sets.append((int(rng.integers(256, 65536)) | (0x8000 if len(sets) & 1 else 0), int(rng.choice([0, 14, 255, 0x80])),
                         int(rng.integers(0, 1 << 32)) | 0x80000000, int(rng.integers(0, 1 << 32)) | (len(sets) & 1) << 31,
                         int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))))
        svec = [(tf, (S.SYN if b & 1 else 0) | (S.ACK if b & 2 else 0) | (S.RST if b & 4 else 0) | (S.FIN if b & 8 else 0), k)
                for k in range(len(sets)) for tf in range(16) for b in range(16)]
        lines = [f"S {tf} {fl} {sets[k][1]} {sets[k][0]} {sets[k][2]} {sets[k][3]} {sets[k][4]} {sets[k][5]}" for tf, fl, k in svec]
        so = [run_driver(exe, lines) for exe in exes]
        # ---- comparisons
        pairs = cmp_pairs(rng)
        co = [run_driver(exe, [f"C {x} {y}" for x, y in pairs]) for exe in exes]
        # ---- prediction
        lines = []
        for p in pred:
            t, s = p["tcb"], p["spec"]
            lines.append(f"H {s['seq'] & M32} {s['ack'] & M32} {len(s['payload'])} {p['sflags']} {p['ts_val']} {p['ts_ecr']} "
                         f"{t['snd_una']} {t['snd_max']} {t['snd_wnd']} {t['snd_cwnd']} {t['ts_recent']} {t['last_ack_sent']} "
                         f"{t['rcv_space']} {p['now']}")
        ho = [run_driver(exe, lines) for exe in exes]
        for name, o in (("send", so), ("compare", co), ("prediction", ho)):
            if o[0] != o[1]:
                raise SystemExit(f"{name}: the sanitizer build answers differently")
    print("driver: built twice (plain, -fsanitize=address,undefined), every vector run on both, no report, equal answers")

    # ---- arrays
    out = {}
    off = np.zeros(len(pvec) + 1, np.int32)
    off[1:] = np.cumsum([len(v["opts"]) for v in pvec])
    out["p_data"] = np.frombuffer(b"".join(v["opts"] for v in pvec), np.uint8)
    out["p_off"] = off
    out["p_tail"] = np.array([v["tail"] for v in pvec], np.uint8)
    out["p_flags"] = np.array([v["flags"] for v in pvec], np.uint8)
    out["p_max_mss"] = np.array([v["max_mss"] for v in pvec], np.uint16)
    out["p_now"] = np.array([NOWS.index(v["now"]) for v in pvec], np.uint8)
    out["nows"] = np.array(NOWS, np.uint32)
    pcls = sorted({v["cls"] for v in pvec})
    out["p_cls_names"] = np.array(pcls)
    out["p_cls"] = np.array([pcls.index(v["cls"]) for v in pvec], np.uint8)
    out["p_rc"] = P[:, 0].astype(np.int8)
    out["p_ts_val"], out["p_ts_ecr"] = P[:, 1].astype(np.uint32), P[:, 2].astype(np.uint32)
    out["p_mss"], out["p_sflags"], out["p_scale"] = P[:, 3].astype(np.uint16), P[:, 4].astype(np.uint16), P[:, 5].astype(np.uint8)
    assert set(out["p_rc"].tolist()) == {0, -1}

    s_rows = [ln.split() for ln in so[0]]
    out["s_tf"] = np.array([v[0] for v in svec], np.uint8)
    out["s_flags"] = np.array([v[1] for v in svec], np.uint8)
    out["s_set"] = np.array([v[2] for v in svec], np.uint8)
    for j, k in enumerate(("s_max_mss", "s_scale", "s_ts_recent", "s_now", "s_iss", "s_nxt0")):
        out[k] = np.array([x[j] for x in sets], np.uint16 if j == 0 else np.uint8 if j == 1 else np.uint32)
    out["s_optlen"] = np.array([int(r[0]) for r in s_rows], np.uint8)
    out["s_nxt"] = np.array([int(r[1]) for r in s_rows], np.uint32)
    sb = np.array([list(bytes.fromhex(r[2])) for r in s_rows], np.uint8)
    assert (sb[:, 20:] == 0xEE).all() and out["s_optlen"].max() <= 20
    for i in range(len(svec)):
        assert (sb[i, out["s_optlen"][i]:] == 0xEE).all(), "bytes written past optlen"
    out["s_bytes"] = sb[:, :20].copy()

    out["c_a"] = np.array([x for x, _ in pairs], np.uint32)
    out["c_b"] = np.array([y for _, y in pairs], np.uint32)
    out["c_res"] = np.array([int(x) for x in co[0]], np.uint16)
    out["c_names"] = np.array(CMP_NAMES)

    h_rows = np.array([[int(x) for x in ln.split()] for ln in ho[0]], np.int64)
    assert ((h_rows[:, 0] + h_rows[:, 1]) <= 1).all()
    hcls = sorted({p["cls"] for p in pred})
    out["h_cls_names"] = np.array(hcls)
    out["h_cls"] = np.array([hcls.index(p["cls"]) for p in pred], np.uint8)
    out["h_tcb"] = np.array([[p["tcb"][c] for c in TCB_COLS] for p in pred], np.uint32)
    out["h_tcb_cols"] = np.array(TCB_COLS)
    out["h_seg"] = np.array([[p["spec"]["seq"] & M32, p["spec"]["ack"] & M32, p["spec"]["wnd"], p["spec"]["flags"],
                              len(p["spec"]["payload"])] for p in pred], np.uint32)
    out["h_parse"] = np.array([p["pidx"] for p in pred], np.int32)
    out["h_now"] = np.array([NOWS.index(p["now"]) for p in pred], np.uint8)
    out["h_branch"] = (h_rows[:, 0] + 2 * h_rows[:, 1]).astype(np.uint8)
    out["h_ts"] = h_rows[:, 2].astype(np.uint8)
    out["h_entry"] = np.array([p["entry"] for p in pred], np.uint8)
    # ts_recent afterwards is ts_val exactly where it was taken
    for p, r in zip(pred, h_rows):
        assert r[3] == (p["ts_val"] if r[2] else p["tcb"]["ts_recent"])

    # ---- the conditions the tests rely on
    counts = {c: int((out["p_cls"] == i).sum()) for i, c in enumerate(pcls)}
    for c in ("last_byte", "last_two", "mid_len", "mss", "wscale", "ts_ack", "ts_ecr_now", "ts_len", "eol_garbage", "nops40",
              "unknown_edge", "len1", "seeded", "uniform", "pred_opts"):
        assert counts.get(c, 0) >= 8, (c, counts)
    hcounts = {c: int((out["h_cls"] == i).sum()) for i, c in enumerate(hcls)}
    for c in ("ack_edge", "cwnd_edge", "len_edge", "ts_edge", "las_edge", "no_ts", "seeded"):
        assert hcounts.get(c, 0) >= 8, (c, hcounts)
    called = out["h_entry"] == 1
    assert set(out["h_branch"][called].tolist()) == {0, 1, 2} and set(out["h_ts"][called].tolist()) == {0, 1}
    assert hcounts["ts_edge"] == 24 and called[out["h_cls"] == hcls.index("seeded")].all()
    assert len(set(out["p_now"].tolist())) <= 3

    os.makedirs(a.out_dir, exist_ok=True)
    one, two = os.path.join(a.out_dir, "tcp_options_ref.npz"), os.path.join(a.out_dir, "tcp_predict_ref.npz")
    size = write_npz(one, out)
    sizes = {one: size}
    if size >= LIMIT:
        hk = {k: v for k, v in out.items() if k.startswith("h_")}
        sizes = {one: write_npz(one, {k: v for k, v in out.items() if k not in hk}), two: write_npz(two, hk)}
    elif os.path.exists(two):
        os.remove(two)
    print(f"parse: {len(pvec)} vectors, {int((out['p_rc'] == -1).sum())} returned -1; by class: {counts}")
    print(f"send: {len(svec)} vectors, option lengths {sorted(set(out['s_optlen'].tolist()))}")
    print(f"compare: {len(pairs)} pairs x {len(CMP_NAMES)} comparisons")
    print(f"prediction: {len(pred)} vectors; by class: {hcounts}; ack {int((out['h_branch'] == 1).sum())}, "
          f"data {int((out['h_branch'] == 2).sum())}, neither {int((out['h_branch'] == 0).sum())}; "
          f"ts_recent taken {int(out['h_ts'].sum())}; {int((~called).sum())} hand-built edges fail the entry test")
    for p, sz in sizes.items():
        print(f"{p}: {sz} bytes")
        assert sz < LIMIT, "cut N_SEEDED_PRED / N_SEEDED_SYN / N_UNIFORM"
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Generate tests/golden/tcp_cksum_ref.npz: IPv4 + TCP byte strings and the
result the reference's own cne_ipv4_udptcp_cksum_verify (net/cne_ip.h:340-349)
gives for each -- the call tcp_input makes for every segment that found a PCB.

    python tools/gen_tcp_cksum_golden.py --ref /path/to/cndp

A few lines of C (below) are compiled against the reference header in a
temporary directory and run once; only data -- the byte strings and the
recorded verdicts -- is written.  Vectors: IHL 5..15 x TCP length {20, 21, 35,
36, 37, 60, 83, 84, 85, 1460} x {checksum correct, off by one, a correct segment
whose checksum field is zero (the urgent pointer makes the sum come out so)},
plus all-zero strings, total_length < IHL * 4, and a total_length that claims
more bytes than the string holds (the missing bytes are zero, as under the
stage's bounded view).  The 1460-byte payloads repeat a 61-byte random pattern,
which keeps the file small.  Arrays: data (u8, the strings end to end), off
(n + 1 starts), l3_len (m->l3_len: where the TCP header is), verify (0 or -1),
kind (the vector's class), desc (text).
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tcp_cksum_ref.npz")
TCP_LENS = (20, 21, 35, 36, 37, 60, 83, 84, 85, 1460)

C_SRC = r"""
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <cne_ip.h>
int main(void)
{
    static uint8_t buf[65536 + 256];
    uint32_t hdr[2];
    while (fread(hdr, 4, 2, stdin) == 2) {
        memset(buf, 0, sizeof(buf));
        if (hdr[0] > 65536 || fread(buf, 1, hdr[0], stdin) != hdr[0])
            return 1;
        printf("%d\n", cne_ipv4_udptcp_cksum_verify((const struct cne_ipv4_hdr *)buf, buf + hdr[1]));
    }
    return 0;
}
"""


def fold(s: int) -> int:
    while s >> 16:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def tcp_sum(ip: bytes, tcp: bytes) -> int:
    d = bytes(ip[12:20]) + bytes([0, ip[9]]) + len(tcp).to_bytes(2, "big") + bytes(tcp)
    d += b"\0" * (len(d) & 1)
    return fold(sum(int.from_bytes(d[k:k + 2], "big") for k in range(0, len(d), 2)))


def segment(rng, ihl: int, l4: int, mode: str) -> bytes:
    hl = ihl * 4
    ip = bytearray(hl)
    ip[0] = 0x40 | ihl
    ip[2:4] = (hl + l4).to_bytes(2, "big")
    ip[8], ip[9] = 64, 6
    ip[12:20] = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
    for k in range(20, hl):
        ip[k] = 1
    if l4 > 256:
        pat = rng.integers(0, 256, 61, dtype=np.uint8).tobytes()
        tcp = bytearray((pat * (l4 // 61 + 1))[:l4])
        tcp[:20] = rng.integers(0, 256, 20, dtype=np.uint8).tobytes()
    else:
        tcp = bytearray(rng.integers(0, 256, l4, dtype=np.uint8).tobytes())
    tcp[12] = 0x50
    tcp[16:18] = b"\0\0"
    if mode == "zero":
        tcp[18:20] = b"\0\0"
        tcp[18:20] = (0xFFFF - tcp_sum(ip, tcp)).to_bytes(2, "big")
    else:
        c = (~tcp_sum(ip, tcp)) & 0xFFFF or 0xFFFF
        if mode == "off1":
            c = (c + 1) & 0xFFFF
        tcp[16:18] = c.to_bytes(2, "big")
    return bytes(ip) + bytes(tcp)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("CNDP_REF"), help="a CNDP v25.08.0 source tree (or $CNDP_REF)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if not a.ref:
        ap.error("--ref or $CNDP_REF is required")
    rng = np.random.default_rng(0x7C9)
    kinds = {"ok": "ok", "off1": "off_by_one", "zero": "zero_field_valid"}
    vecs = []  # (bytes, l3_len, kind, desc)
    for ihl in range(5, 16):
        for l4 in TCP_LENS:
            for mode in ("ok", "off1", "zero"):
                vecs.append((segment(rng, ihl, l4, mode), ihl * 4, kinds[mode], f"ihl{ihl}/tcp={l4}/{mode}"))
    for ln in (40, 41, 64):
        vecs.append((bytes(ln), 20, "all_zero", f"all-zero/{ln}"))
    for ihl, tot in ((5, 19), (15, 40), (6, 0)):
        d = bytearray(segment(rng, ihl, 36, "ok"))
        d[2:4] = tot.to_bytes(2, "big")
        vecs.append((bytes(d), ihl * 4, "tot_lt_ihl", f"short/ihl{ihl}/tot={tot}"))
    for extra in (1, 7, 300):   # total_length claims bytes the string does not hold
        d = bytearray(segment(rng, 5, 37, "ok"))
        d[2:4] = (len(d) + extra).to_bytes(2, "big")
        vecs.append((bytes(d), 20, "claims_more", f"claims+{extra}"))
    # a zero tail that is really there: the sum of the longer segment, cut short
    d = bytearray(segment(rng, 5, 48, "ok"))
    d[-8:] = bytes(8)
    d[36:38] = b"\0\0"
    d[36:38] = ((~tcp_sum(d[:20], d[20:])) & 0xFFFF or 0xFFFF).to_bytes(2, "big")
    vecs.append((bytes(d[:-8]), 20, "claims_more", "claims+8/valid-over-zeros"))

    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "ck.c"), os.path.join(tmp, "ck")
        with open(src, "w") as f:
            f.write(C_SRC)
        inc = [f"-I{a.ref}/{d}" for d in ("lib/include", "lib/include/net", "lib/core/pktmbuf", "lib/core/mempool",
                                          "lib/core/log", "lib/core/osal", "lib/core/mmap")]
        subprocess.run(["gcc", "-O1", "-std=gnu11", "-w", *inc, "-o", exe, src], check=True)
        blob = b"".join(np.array([len(v), l3], np.uint32).tobytes() + v for v, l3, _, _ in vecs)
        r = subprocess.run([exe], input=blob, capture_output=True, check=True)
    verify = np.array([int(x) for x in r.stdout.split()], np.int8)
    assert len(verify) == len(vecs)
    off = np.zeros(len(vecs) + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v, _, _, _ in vecs])
    np.savez_compressed(a.out, data=np.frombuffer(b"".join(v for v, _, _, _ in vecs), np.uint8), off=off,
                        l3_len=np.array([l3 for _, l3, _, _ in vecs], np.uint16), verify=verify,
                        kind=np.array([k for _, _, k, _ in vecs]), desc=np.array([k for _, _, _, k in vecs]))
    print(f"{a.out}: {len(vecs)} vectors, {int((verify == 0).sum())} verify, {os.path.getsize(a.out)} bytes")
    for k in sorted(set(kinds.values()) | {"all_zero", "tot_lt_ihl", "claims_more"}):
        sel = np.array([v[2] == k for v in vecs])
        print(f"  {k}: {int(sel.sum())} vectors, {int((verify[sel] == 0).sum())} verify")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Generate tests/golden/udp_cksum_ref.npz: IPv4 + UDP byte strings and the
result the reference's own cne_ipv4_udptcp_cksum_verify (net/cne_ip.h:340-349)
gives for each.

    python tools/gen_udp_cksum_golden.py [--ref /path/to/cndp]

A few lines of C (below) are compiled against the reference header in a
temporary directory and run once; only data -- the byte strings and the
recorded verdicts -- is written.  Vectors: IHL 5..15 x L4 length {8, 9, 15, 16,
17, 63, 64, 65, 1472} x checksum {correct, off by one, zero field}, plus
all-zero strings, total_length < IHL * 4, and a total_length that claims more
bytes than the string holds (the missing bytes are zero, as under the stage's
bounded view).  Arrays: data (u8, the strings end to end), off (n + 1 starts),
l3_len (m->l3_len: where the UDP header is), verify (0 or -1), kind (text).
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "udp_cksum_ref.npz")
L4_LENS = (8, 9, 15, 16, 17, 63, 64, 65, 1472)

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


def datagram(rng, ihl: int, l4: int, mode: str) -> bytes:
    hl = ihl * 4
    ip = bytearray(hl)
    ip[0] = 0x40 | ihl
    ip[2:4] = (hl + l4).to_bytes(2, "big")
    ip[8], ip[9] = 64, 17
    ip[12:20] = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
    for k in range(20, hl):
        ip[k] = 1
    udp = bytearray(rng.integers(0, 256, l4, dtype=np.uint8).tobytes())
    udp[4:6] = l4.to_bytes(2, "big")
    udp[6:8] = b"\0\0"
    if mode != "zero":
        d = bytes(ip[12:20]) + bytes([0, 17]) + l4.to_bytes(2, "big") + bytes(udp)
        d += b"\0" * (len(d) & 1)
        c = (~fold(sum(int.from_bytes(d[k:k + 2], "big") for k in range(0, len(d), 2)))) & 0xFFFF or 0xFFFF
        if mode == "off1":
            c = (c + 1) & 0xFFFF
        udp[6:8] = c.to_bytes(2, "big")
    return bytes(ip) + bytes(udp)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("CNDP_REF", "/root/reference"))
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    rng = np.random.default_rng(0x55D9)
    vecs = []  # (bytes, l3_len, kind)
    for ihl in range(5, 16):
        for l4 in L4_LENS:
            for mode in ("ok", "off1", "zero"):
                vecs.append((datagram(rng, ihl, l4, mode), ihl * 4, f"ihl{ihl}/l4={l4}/{mode}"))
    for ln in (28, 29, 64):
        vecs.append((bytes(ln), 20, f"all-zero/{ln}"))
    for ihl, tot in ((5, 19), (15, 40), (6, 0)):
        d = bytearray(datagram(rng, ihl, 16, "ok"))
        d[2:4] = tot.to_bytes(2, "big")
        vecs.append((bytes(d), ihl * 4, f"short/ihl{ihl}/tot={tot}"))
    for extra in (1, 7, 300):   # total_length claims bytes the string does not hold
        d = bytearray(datagram(rng, 5, 33, "ok"))
        d[2:4] = (len(d) + extra).to_bytes(2, "big")
        vecs.append((bytes(d), 20, f"claims+{extra}"))
    # a zero tail that is really there: the sum of the longer datagram, cut short
    d = bytearray(datagram(rng, 5, 40, "zero"))
    d[-8:] = bytes(8)
    full = bytes(d[12:20]) + bytes([0, 17]) + (40).to_bytes(2, "big") + bytes(d[20:])
    c = (~fold(sum(int.from_bytes(full[k:k + 2], "big") for k in range(0, len(full), 2)))) & 0xFFFF or 0xFFFF
    d[26:28] = c.to_bytes(2, "big")
    vecs.append((bytes(d[:-8]), 20, "claims+8/valid-over-zeros"))

    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "ck.c"), os.path.join(tmp, "ck")
        with open(src, "w") as f:
            f.write(C_SRC)
        inc = [f"-I{a.ref}/{d}" for d in ("lib/include", "lib/include/net", "lib/core/pktmbuf", "lib/core/mempool",
                                          "lib/core/log", "lib/core/osal", "lib/core/mmap")]
        subprocess.run(["gcc", "-O1", "-std=gnu11", "-w", *inc, "-o", exe, src], check=True)
        blob = b"".join(np.array([len(v), l3], np.uint32).tobytes() + v for v, l3, _ in vecs)
        r = subprocess.run([exe], input=blob, capture_output=True, check=True)
    verify = np.array([int(x) for x in r.stdout.split()], np.int8)
    assert len(verify) == len(vecs)
    off = np.zeros(len(vecs) + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v, _, _ in vecs])
    np.savez_compressed(a.out, data=np.frombuffer(b"".join(v for v, _, _ in vecs), np.uint8), off=off,
                        l3_len=np.array([l3 for _, l3, _ in vecs], np.uint16), verify=verify,
                        kind=np.array([k for _, _, k in vecs]))
    print(f"{a.out}: {len(vecs)} vectors, {int((verify == 0).sum())} verify, {os.path.getsize(a.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Generate tests/golden/ip4_output_cksum_ref.npz: IPv4 header + L4 byte strings
and what the reference's own cne_ipv4_cksum and cne_ipv4_udptcp_cksum
(net/cne_ip.h:209-215, 275-325) return for each -- the two checksum steps of
ip4_output (lib/cnet/ipv4/ip4_output.c:100-112).

    python tools/gen_ip4_output_golden.py [--ref /path/to/cndp]

A few lines of C (below) are compiled against the reference header in a
temporary directory and run once; only data -- the byte strings and the
recorded results -- is written.  Every string is a 20-byte header as
ip4_output has it when it calls the two functions (hdr_checksum 0, packet_id
set) followed by the L4 bytes.  UDP strings carry the header udp_output writes
(dgram_len = the L4 length, dgram_cksum 0), so a transmit call can reproduce
them; TCP strings carry a random checksum field, which the reference sums as
it stands.  Vectors: L4 lengths {8, 9, 10, 11, 23, 24, 25, 63, 64, 65, 255, 256,
257, 1471, 1472, 1480} x protocol {17, 6}, a few hundred random ones, and per
protocol twelve whose last 16-bit word is chosen so that the complemented sum
is 0 (kind "zero-sum/..."): UDP must record 0xFFFF there, TCP 0.  Arrays: data
(u8, the strings end to end), off (n + 1 starts), proto (u8), ip_cksum and
l4_cksum (u16, the return values as a little-endian host holds them), kind.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ip4_output_cksum_ref.npz")
L4_LENS = (8, 9, 10, 11, 23, 24, 25, 63, 64, 65, 255, 256, 257, 1471, 1472, 1480)

C_SRC = r"""
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <cne_ip.h>
int main(void)
{
    static uint8_t buf[65536 + 256];
    uint32_t len;
    while (fread(&len, 4, 1, stdin) == 1) {
        memset(buf, 0, sizeof(buf));
        if (len < 20 || len > 65536 || fread(buf, 1, len, stdin) != len)
            return 1;
        const struct cne_ipv4_hdr *ip = (const struct cne_ipv4_hdr *)buf;
        printf("%u %u\n", (unsigned)cne_ipv4_cksum(ip), (unsigned)cne_ipv4_udptcp_cksum(ip, buf + 20));
    }
    return 0;
}
"""


def fold(s: int) -> int:
    while s >> 16:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def string(rng, proto: int, l4: int, zero_sum: bool = False) -> bytes:
    ip = bytearray(20)
    ip[0], ip[1] = 0x45, int(rng.integers(0, 256))
    ip[2:4] = (20 + l4).to_bytes(2, "big")
    ip[4:6] = rng.integers(0, 256, 2, dtype=np.uint8).tobytes()
    ip[8], ip[9] = int(rng.integers(1, 256)), proto
    ip[12:20] = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
    d = bytearray(rng.integers(0, 256, l4, dtype=np.uint8).tobytes())
    if proto == 17:
        d[4:6] = l4.to_bytes(2, "big")
        d[6:8] = b"\0\0"
    if zero_sum:    # the last 16-bit word cancels the rest: the one's complement sum is 0xFFFF
        assert l4 % 2 == 0 and l4 >= (10 if proto == 17 else 22)
        d[-2:] = b"\0\0"
        ph = bytes(ip[12:20]) + bytes([0, proto]) + l4.to_bytes(2, "big")
        s = fold(sum(int.from_bytes((ph + bytes(d))[k:k + 2], "big") for k in range(0, 12 + l4, 2)))
        d[-2:] = ((0xFFFF - s) or 0xFFFF).to_bytes(2, "big")
    return bytes(ip) + bytes(d)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("CNDP_REF", "/root/reference"))
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    rng = np.random.default_rng(0x1D4E)
    vecs = []  # (bytes, proto, kind)
    for proto in (17, 6):
        for l4 in L4_LENS:
            vecs.append((string(rng, proto, l4), proto, f"p{proto}/l4={l4}"))
        for k in range(160):
            l4 = int(rng.integers(8, 1481))
            vecs.append((string(rng, proto, l4), proto, f"p{proto}/random/l4={l4}"))
        for l4 in (10, 12, 22, 24, 26, 64, 66, 256, 258, 1000, 1472, 1480):
            if proto == 6 and l4 < 22:
                l4 += 20
            vecs.append((string(rng, proto, l4, zero_sum=True), proto, f"zero-sum/p{proto}/l4={l4}"))

    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "ck.c"), os.path.join(tmp, "ck")
        with open(src, "w") as f:
            f.write(C_SRC)
        inc = [f"-I{a.ref}/{d}" for d in ("lib/include", "lib/include/net", "lib/core/pktmbuf", "lib/core/mempool",
                                          "lib/core/log", "lib/core/osal", "lib/core/mmap")]
        subprocess.run(["gcc", "-O1", "-std=gnu11", "-w", *inc, "-o", exe, src], check=True)
        blob = b"".join(np.array([len(v)], np.uint32).tobytes() + v for v, _, _ in vecs)
        r = subprocess.run([exe], input=blob, capture_output=True, check=True)
    res = np.array([[int(x) for x in ln.split()] for ln in r.stdout.decode().splitlines()], np.uint16)
    assert res.shape == (len(vecs), 2)
    off = np.zeros(len(vecs) + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v, _, _ in vecs])
    np.savez_compressed(a.out, data=np.frombuffer(b"".join(v for v, _, _ in vecs), np.uint8), off=off,
                        proto=np.array([p for _, p, _ in vecs], np.uint8), ip_cksum=res[:, 0], l4_cksum=res[:, 1],
                        kind=np.array([k for _, _, k in vecs]))
    zs = [i for i, (_, _, k) in enumerate(vecs) if k.startswith("zero-sum")]
    print(f"{a.out}: {len(vecs)} vectors, {len(zs)} zero-sum "
          f"(UDP -> {sorted(set(res[[i for i in zs if vecs[i][1] == 17], 1].tolist()))}, "
          f"TCP -> {sorted(set(res[[i for i in zs if vecs[i][1] == 6], 1].tolist()))}), {os.path.getsize(a.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())

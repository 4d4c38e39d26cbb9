#!/usr/bin/env python3
"""Generate tests/golden/ip4_fwd_cksum_ref.npz: (time_to_live, hdr_checksum)
pairs and what the reference's own ipv4_adjust_cksum
(lib/cnet/ipv4/cnet_ipv4.h:159-170) makes of each.

    python tools/gen_ip4_forward_golden.py [--ref /path/to/cndp]

The function's text is lifted from the reference header at generation time into
a temporary directory, compiled there against net/cne_ip.h (struct
cne_ipv4_hdr) with a few lines of C around it (below), and run once; only data
-- the pairs and the recorded results -- is written.  Vectors: TTL {0, 1, 255}
x checksum {0x0000, 0xFFFF, 0xFEFF, 0xFF00, 0x00FF, 0x0100, 0x0001} (the
carry's edges), then 4096 random pairs.  Arrays (u8 / u16, the checksum as a
little-endian host loads the field): ttl, cksum, ttl_out, cksum_out.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ip4_fwd_cksum_ref.npz")
TTLS = (0, 1, 255)
CKSUMS = (0x0000, 0xFFFF, 0xFEFF, 0xFF00, 0x00FF, 0x0100, 0x0001)

C_HEAD = r"""
#include <endian.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <cne_ip.h>
"""
C_MAIN = r"""
int main(void)
{
    uint16_t v[2];
    while (fread(v, 2, 2, stdin) == 2) {
        struct cne_ipv4_hdr h;
        memset(&h, 0, sizeof(h));
        h.time_to_live = (uint8_t)v[0];
        h.hdr_checksum = v[1];
        ipv4_adjust_cksum(&h);
        printf("%u %u\n", (unsigned)h.time_to_live, (unsigned)h.hdr_checksum);
    }
    return 0;
}
"""


def lift(ref: str) -> str:
    with open(os.path.join(ref, "lib", "cnet", "ipv4", "cnet_ipv4.h")) as f:
        txt = f.read()
    m = re.search(r"static inline void\s+ipv4_adjust_cksum\(struct cne_ipv4_hdr \*hdr\)\s*\{.*?\n\}", txt, re.S)
    if not m:
        raise SystemExit("ipv4_adjust_cksum not found in the reference's cnet_ipv4.h")
    return m.group(0)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("CNDP_REF", "/root/reference"))
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    rng = np.random.default_rng(0x1F4D)
    pairs = [(t, c) for t in TTLS for c in CKSUMS]
    pairs += list(zip(rng.integers(0, 256, 4096).tolist(), rng.integers(0, 65536, 4096).tolist()))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "adj.c"), os.path.join(tmp, "adj")
        with open(src, "w") as f:
            f.write(C_HEAD + lift(a.ref) + C_MAIN)
        inc = [f"-I{a.ref}/{d}" for d in ("lib/include", "lib/include/net", "lib/core/pktmbuf", "lib/core/mempool",
                                          "lib/core/log", "lib/core/osal", "lib/core/mmap")]
        subprocess.run(["gcc", "-O1", "-std=gnu11", "-w", *inc, "-o", exe, src], check=True)
        blob = np.array(pairs, np.uint16).tobytes()
        r = subprocess.run([exe], input=blob, capture_output=True, check=True)
    res = np.array([int(x) for x in r.stdout.split()], np.int64).reshape(-1, 2)
    assert len(res) == len(pairs)
    p = np.array(pairs, np.int64)
    np.savez_compressed(a.out, ttl=p[:, 0].astype(np.uint8), cksum=p[:, 1].astype(np.uint16),
                        ttl_out=res[:, 0].astype(np.uint8), cksum_out=res[:, 1].astype(np.uint16))
    print(f"{a.out}: {len(pairs)} pairs, {os.path.getsize(a.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Generate tests/golden/cndpfwd_l3_ref.npz: route operations, addresses and
what the reference's own FIB (lib/usr/clib/fib: cne_fib.c, dir24_8.c;
lib/usr/clib/rib: cne_rib.c) and lib/include/cne_inet4.h answer for them when
they are driven the way examples/cndpfwd/l3-fwd.c drives them.

    python tools/gen_cndpfwd_l3_golden.py [--ref /path/to/cndp]

The three sources are compiled from the reference tree at generation time in a
temporary directory, with an empty cne_build_config.h, a bsd/string.h that
gives strlcpy, and stubs in the driver for cne_log, cne_printf, __cne_panic and
for the node pool the RIB takes its nodes from (mempool_create / _get / _put /
_destroy and mmap_alloc / _addr / _free over malloc); the program is run once
and only data is written.  Tests never run this tool.

Contents:
  op_ip (u32, host order), op_depth (u8), op_mac (u8[6]), op_port (u16), op_del
  (u8)    the operations in order: an add through inet_mtoh64 and
          `tx_port << 48 | mac` into a CNE_FIB_DUMMY FIB made as l3fwd_fib_init
          makes it, or (op_del = 1) a cne_fib_delete.  About 300 adds with depths
          from {1, 8, 9, 16, 23, 24, 25, 31, 32} (no /0, so addresses miss), the
          prefixes drawn from a pool of 32 addresses that nest (all with the top
          bit set), host bits set beyond the prefix, ports from {0, 1, 7, 255,
          256, 0x7FFF}, random MACs; some prefixes added twice (the later next
          hop replaces the earlier) and 40 deleted again
  addr (u32, host order)   2048 addresses: inside routes in force with the bits
          beyond the prefix randomised, near misses (one bit inside a prefix
          flipped), random ones (half with the top bit clear: certain misses)
  nh (u64), mac (u8[6]), tx_port (u16)   per address: cne_fib_lookup_bulk's next
          hop (bursts of 256), inet_h64tom of it and (uint16_t)(nh >> 48)
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "cndpfwd_l3_ref.npz")
DEPTHS = (1, 8, 9, 16, 23, 24, 25, 31, 32)
PORTS = (0, 1, 7, 255, 256, 0x7FFF)
SRCS = ("lib/usr/clib/fib/cne_fib.c", "lib/usr/clib/fib/dir24_8.c", "lib/usr/clib/rib/cne_rib.c")
INCS = ("lib/include", "lib/usr/clib/fib", "lib/usr/clib/rib", "lib/core/log", "lib/core/mmap", "lib/core/mempool",
        "lib/core/osal", "lib/core/cne", "lib/core/pktmbuf")

BSD_STRING_H = r"""
#ifndef GOLDEN_BSD_STRING_H
#define GOLDEN_BSD_STRING_H
#include <stddef.h>
static inline size_t strlcpy(char *d, const char *s, size_t n)
{
    size_t l = 0;
    while (s[l])
        l++;
    if (n) {
        size_t c = l < n - 1 ? l : n - 1;
        for (size_t i = 0; i < c; i++)
            d[i] = s[i];
        d[c] = 0;
    }
    return l;
}
#endif
"""

# stdin: u32 n_ops, n_ops x {u32 ip, u32 depth, u32 del, u32 port, u8 mac[6], u8 pad[2]}, u32 n_addr,
# n_addr x u32; stdout: one line per address: nh, six octets, tx_port.
DRIVER_C = r"""
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mempool.h>
#include <cne_mmap.h>
#include <cne_fib.h>
#include <cne_inet4.h>
#include <net/cne_ether.h>

int cne_log(uint32_t level, const char *func, int line, const char *format, ...) { (void)level; (void)func; (void)line; (void)format; return 0; }
int cne_printf(const char *fmt, ...) { (void)fmt; return 0; }
void __cne_panic(const char *funcname, int line, const char *format, ...) { fprintf(stderr, "panic %s:%d %s\n", funcname, line, format); abort(); }

/* the RIB's node pool: objects of cfg.objsz bytes, zeroed, from malloc */
struct pool { size_t objsz; };
mempool_t *mempool_create(struct mempool_cfg *c) { struct pool *p = calloc(1, sizeof(*p)); p->objsz = c->objsz; return (mempool_t *)p; }
void mempool_destroy(mempool_t *mp) { free(mp); }
int mempool_get(mempool_t *mp, void **obj) { *obj = calloc(1, ((struct pool *)mp)->objsz); return *obj ? 0 : -1; }
void mempool_put(mempool_t *mp, void *obj) { (void)mp; free(obj); }
mmap_t *mmap_alloc(uint32_t cnt, uint32_t sz, mmap_type_t t) { (void)cnt; (void)sz; (void)t; return malloc(16); }
void *mmap_addr(mmap_t *mm) { return mm; }
int mmap_free(mmap_t *mm) { free(mm); return 0; }

static uint32_t rd(void) { uint32_t v; if (fread(&v, 4, 1, stdin) != 1) exit(2); return v; }

int main(void)
{
    struct cne_fib_conf config; /* l3-fwd.c:98-103 */
    memset(&config, 0, sizeof(config));
    config.max_routes = 1 << 16;
    config.default_nh = 0xFFFFFFFFFFFF;
    config.type = CNE_FIB_DUMMY;
    struct cne_fib *fib = cne_fib_create("l3fwd_fib", &config);
    if (!fib) return 3;
    uint32_t nops = rd();
    for (uint32_t i = 0; i < nops; i++) {
        uint32_t ip = rd(), depth = rd(), del = rd(), port = rd();
        struct ether_addr eaddr;
        uint8_t m[8];
        uint64_t eaddr_uint;
        if (fread(m, 8, 1, stdin) != 1) return 2;
        memcpy(eaddr.ether_addr_octet, m, 6);
        int r;
        if (del) {
            r = cne_fib_delete(fib, ip, (uint8_t)depth);
        } else {
            inet_mtoh64(&eaddr, &eaddr_uint);                      /* l3-fwd.c:64 */
            uint64_t nexthop = ((uint64_t)port << 48) | eaddr_uint; /* :67 */
            r = cne_fib_add(fib, ip, (uint8_t)depth, nexthop);
        }
        if (r < 0) { fprintf(stderr, "op %u failed: %d\n", i, r); return 4; }
    }
    uint32_t na = rd();
    uint32_t *ips = calloc(na ? na : 1, sizeof(*ips));
    uint64_t *nh = calloc(na ? na : 1, sizeof(*nh));
    for (uint32_t i = 0; i < na; i++)
        ips[i] = rd();
    for (uint32_t i = 0; i < na; i += 256) { /* a burst at a time */
        uint32_t k = na - i < 256 ? na - i : 256;
        if (cne_fib_lookup_bulk(fib, ips + i, nh + i, (int)k) < 0) return 5;
    }
    for (uint32_t i = 0; i < na; i++) {
        struct ether_addr e;
        inet_h64tom(nh[i], &e);                                    /* l3-fwd.c:88-89 */
        uint16_t tx_port = (uint16_t)(nh[i] >> 48);
        printf("%llu %u %u %u %u %u %u %u\n", (unsigned long long)nh[i], e.ether_addr_octet[0], e.ether_addr_octet[1],
               e.ether_addr_octet[2], e.ether_addr_octet[3], e.ether_addr_octet[4], e.ether_addr_octet[5], tx_port);
    }
    return 0;
}
"""


def masks(lens):
    lens = np.asarray(lens, np.uint64)
    return ((np.uint64(0xFFFFFFFF) << (np.uint64(32) - lens)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def make_ops(rng):
    pool = (rng.integers(0, 1 << 31, 32, dtype=np.uint64) | (1 << 31)).astype(np.uint32)
    pool[1] = pool[0] ^ 0x00000001          # neighbours that part at /32, /25, /24, /23, /16 and /9
    pool[2] = pool[0] ^ 0x00000080
    pool[3] = pool[0] ^ 0x00000100
    pool[4] = pool[0] ^ 0x00000200
    pool[5] = pool[0] ^ 0x00010000
    pool[6] = pool[0] ^ 0x00800000
    ops = []                                # (ip, depth, del, port, mac)
    for _ in range(300):
        depth = int(rng.choice(DEPTHS))
        ip = int(rng.choice(pool)) | (int(rng.integers(0, 1 << 32)) & ~int(masks([depth])[0]) & 0xFFFFFFFF)
        ops.append((ip, depth, 0, int(rng.choice(PORTS)), rng.integers(0, 256, 6, dtype=np.uint8)))
    live = {}
    for ip, depth, _, _, _ in ops:
        live[(ip & int(masks([depth])[0]), depth)] = ip
    keys = list(live)
    for k in rng.permutation(len(keys))[:40]:   # deleted again: their addresses fall back to a parent or miss
        prefix, depth = keys[k]
        ops.append((live[keys[k]], depth, 1, 0, np.zeros(6, np.uint8)))
        del live[keys[k]]
    return ops, sorted(live)


def make_addrs(rng, live, deleted):
    pd = np.array(live + deleted, np.uint64)
    k1, k2 = 1200, 400
    pick = pd[rng.integers(0, len(pd), k1)]
    m = masks(pick[:, 1])
    a1 = (pick[:, 0].astype(np.uint32) & m) | (rng.integers(0, 1 << 32, k1, dtype=np.uint64).astype(np.uint32) & ~m)
    pick = pd[rng.integers(0, len(pd), k2)]
    m = masks(pick[:, 1])
    a2 = (pick[:, 0].astype(np.uint32) & m) | (rng.integers(0, 1 << 32, k2, dtype=np.uint64).astype(np.uint32) & ~m)
    for k in range(k2):                     # near misses: one bit inside the prefix flipped
        a2[k] ^= np.uint32(1 << (32 - int(rng.integers(1, int(pick[k, 1]) + 1))))
    k3 = 2048 - k1 - k2
    a3 = rng.integers(0, 1 << 32, k3, dtype=np.uint64).astype(np.uint32)
    a3[::2] &= np.uint32(0x7FFFFFFF)
    return np.concatenate([a1, a2, a3])


def build(ref: str, tmp: str) -> str:
    os.makedirs(os.path.join(tmp, "bsd"))
    open(os.path.join(tmp, "cne_build_config.h"), "w").close()
    with open(os.path.join(tmp, "bsd", "string.h"), "w") as f:
        f.write(BSD_STRING_H)
    with open(os.path.join(tmp, "bsd", "bsd.h"), "w") as f:
        f.write("#include <bsd/string.h>\n")
    with open(os.path.join(tmp, "driver.c"), "w") as f:
        f.write(DRIVER_C)
    exe = os.path.join(tmp, "l3_golden")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-w", f"-I{tmp}", *[f"-I{ref}/{d}" for d in INCS], "-o", exe,
                    os.path.join(tmp, "driver.c"), *[os.path.join(ref, s) for s in SRCS], "-lpthread"], check=True)
    return exe


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("CNDP_REF", "/root/reference"))
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    rng = np.random.default_rng(0x13F0D)
    ops, live = make_ops(rng)
    deleted = [(ip & int(masks([d])[0]), d) for ip, d, dele, _, _ in ops if dele]
    addr = make_addrs(rng, live, deleted)
    addr = addr[rng.permutation(len(addr))]
    blob = np.uint32(len(ops)).tobytes()
    for ip, depth, dele, port, mac in ops:
        blob += np.array([ip, depth, dele, port], np.uint32).tobytes() + mac.tobytes() + b"\0\0"
    blob += np.uint32(len(addr)).tobytes() + addr.tobytes()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(a.ref, tmp)
        r = subprocess.run([exe], input=blob, capture_output=True, check=True)
    rows = np.array([[int(x) for x in ln.split()] for ln in r.stdout.decode().splitlines()], np.uint64)
    assert rows.shape == (len(addr), 8)
    out = {"op_ip": np.array([o[0] for o in ops], np.uint32), "op_depth": np.array([o[1] for o in ops], np.uint8),
           "op_del": np.array([o[2] for o in ops], np.uint8), "op_port": np.array([o[3] for o in ops], np.uint16),
           "op_mac": np.stack([o[4] for o in ops]).astype(np.uint8), "addr": addr, "nh": rows[:, 0],
           "mac": rows[:, 1:7].astype(np.uint8), "tx_port": rows[:, 7].astype(np.uint16)}
    np.savez_compressed(a.out, **out)
    miss = int(np.count_nonzero(rows[:, 0] == 0xFFFFFFFFFFFF))
    print(f"{len(ops)} operations ({len(deleted)} deletes, {len(live)} routes in force), {len(addr)} addresses, {miss} miss, "
          f"{len(np.unique(rows[:, 0]))} distinct next hops")
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())

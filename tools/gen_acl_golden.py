#!/usr/bin/env python3
"""Generate tests/golden/acl_ref.npz: rule sets, packet address pairs and the
acl_results the reference's own ACL library (lib/usr/clib/acl: cne_acl.c,
acl_bld.c, acl_gen.c, acl_run_scalar.c, tb_mem.c) leaves for them when it is
driven the way examples/cndpfwd/acl-func.c drives it.

    python tools/gen_acl_golden.py [--ref /path/to/cndp]

The five sources are compiled from the reference tree at generation time in a
temporary directory, with an empty cne_build_config.h, a bsd/string.h that
gives strlcpy, and stubs for cne_log, cne_printf, __cne_panic and
cne_cpu_get_flag_enabled (returning 0, which selects the scalar runner); the
program is run once per rule set and only data -- the rules, the packets and
the recorded results -- is written.  Tests never run this tool.

Rule sets (arrays <set>_src_addr, _dst_addr (u32, host order), _src_msk,
_dst_msk, _deny (u8); packets <set>_psrc, _pdst (u32, host order); results
<set>_res (u32)):
  a   add_init_rules' 4226 rules (written out here from acl-func.c:404-484's
      description, and compared with cndp_acl_add_init_rules by the tests), 2048
      packets: drawn from the rules of each of the four kinds, dst-deny and
      src-deny at once, allow pairs with the wrong partner, random addresses
  b   300 random rules: prefix lengths from {0, 1, 7, 8, 9, 16, 17, 24, 31, 32}
      on each side (never /0:/0, and both sides at most /1 only from index 200
      on), addresses from a pool of 12 so that rules nest
      and repeat, host bits set beyond the prefix; 2048 packets: drawn from the
      rules with the bits beyond the prefix randomised, near misses (one bit
      inside a prefix flipped), and packets no rule can match (every pool
      address has its top bit set, these have it clear on both sides)
  b0  b with a /0:/0 allow rule inserted in the middle (index 150), same packets:
      every packet matches, the earlier rules still win
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "acl_ref.npz")
LENS = (0, 1, 7, 8, 9, 16, 17, 24, 31, 32)
ACL_SRCS = ("cne_acl.c", "acl_bld.c", "acl_gen.c", "acl_run_scalar.c", "tb_mem.c")
INCS = ("lib/include", "lib/usr/clib/acl", "lib/core/osal", "lib/core/log", "lib/core/cne", "lib/usr/clib/utils")

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

# stdin: u32 n_rules, n_rules x {src, src_msk, dst, dst_msk, deny}, u32 n_pkts,
# n_pkts x {src, dst}; stdout: one result per line.  The rule and the field
# definitions are the ones acl-func.c:44-85, :165-185 sets up.
DRIVER_C = r"""
#include <endian.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cne_acl.h>
#include <cne_cpuflags.h>
#include <cne_log.h>

int cne_log(uint32_t level, const char *func, int line, const char *format, ...) { (void)level; (void)func; (void)line; (void)format; return 0; }
int cne_printf(const char *fmt, ...) { (void)fmt; return 0; }
void __cne_panic(const char *funcname, int line, const char *format, ...) { fprintf(stderr, "panic %s:%d %s\n", funcname, line, format); abort(); }
int cne_cpu_get_flag_enabled(enum cne_cpu_flag_t feature) { (void)feature; return 0; }

enum { PROTO_FIELD_IPV4, SRC_FIELD_IPV4, DST_FIELD_IPV4, NUM_FIELDS_IPV4 };
CNE_ACL_RULE_DEF(acl4_rule, NUM_FIELDS_IPV4);

static uint32_t rd(void) { uint32_t v; if (fread(&v, 4, 1, stdin) != 1) exit(2); return v; }

int main(void)
{
    struct cne_acl_param prm = {.name = "GOLDEN", .rule_size = CNE_ACL_RULE_SZ(NUM_FIELDS_IPV4), .max_rule_num = 100000};
    struct cne_acl_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.num_categories = 1;
    cfg.num_fields = 3;
    cfg.defs[0] = (struct cne_acl_field_def){.type = CNE_ACL_FIELD_TYPE_BITMASK, .size = 1, .field_index = 0, .input_index = 0, .offset = 0};
    cfg.defs[1] = (struct cne_acl_field_def){.type = CNE_ACL_FIELD_TYPE_MASK, .size = 4, .field_index = 1, .input_index = 1, .offset = 3};
    cfg.defs[2] = (struct cne_acl_field_def){.type = CNE_ACL_FIELD_TYPE_MASK, .size = 4, .field_index = 2, .input_index = 2, .offset = 7};
    struct cne_acl_ctx *ctx = cne_acl_create(&prm);
    if (!ctx) return 3;
    uint32_t nr = rd();
    struct acl4_rule *rules = calloc(nr ? nr : 1, sizeof(*rules));
    for (uint32_t i = 0; i < nr; i++) {
        uint32_t src = rd(), sm = rd(), dst = rd(), dm = rd(), deny = rd();
        rules[i].data.userdata = i + (deny ? 0xf0000000u : 1u);
        rules[i].data.category_mask = -1;
        rules[i].data.priority = CNE_ACL_MAX_PRIORITY - i;
        rules[i].field[PROTO_FIELD_IPV4].value.u8 = 0;
        rules[i].field[PROTO_FIELD_IPV4].mask_range.u8 = 0;
        rules[i].field[SRC_FIELD_IPV4].value.u32 = src;
        rules[i].field[SRC_FIELD_IPV4].mask_range.u8 = (uint8_t)sm;
        rules[i].field[DST_FIELD_IPV4].value.u32 = dst;
        rules[i].field[DST_FIELD_IPV4].mask_range.u8 = (uint8_t)dm;
    }
    int r = cne_acl_add_rules(ctx, (const struct cne_acl_rule *)rules, nr);
    if (r) { fprintf(stderr, "add_rules %d\n", r); return 4; }
    r = cne_acl_build(ctx, &cfg);
    if (r) { fprintf(stderr, "build %d\n", r); return 5; }
    uint32_t np = rd();
    uint8_t *buf = calloc(np ? np : 1, 16);
    const uint8_t **ptrs = calloc(np ? np : 1, sizeof(*ptrs));
    uint32_t *res = calloc(np ? np : 1, sizeof(*res));
    for (uint32_t i = 0; i < np; i++) {
        uint32_t s = htobe32(rd()), d = htobe32(rd());
        buf[16 * i] = (uint8_t)(i * 7u); /* the proto byte: ignored by every rule */
        memcpy(buf + 16 * i + 3, &s, 4);
        memcpy(buf + 16 * i + 7, &d, 4);
        ptrs[i] = buf + 16 * i;
    }
    for (uint32_t i = 0; i < np; i += 256) { /* BURST_SIZE at a time */
        uint32_t k = np - i < 256 ? np - i : 256;
        r = cne_acl_classify(ctx, ptrs + i, res + i, k, 1);
        if (r) { fprintf(stderr, "classify %d\n", r); return 6; }
    }
    for (uint32_t i = 0; i < np; i++)
        printf("%u\n", res[i]);
    return 0;
}
"""


def ipv4(a, b, c, d):
    return a << 24 | b << 16 | c << 8 | d


def masks(lens):
    lens = np.asarray(lens, np.uint64)
    return ((np.uint64(0xFFFFFFFF) << (np.uint64(32) - lens)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def init_rules():
    r = [(0, 0, ipv4(100, i, 0, 0), 24, 1) for i in range(100)]
    r += [(ipv4(10 + i, 0, 0, 0), 8, 0, 0, 1) for i in range(15)]
    r += [(ipv4(101, 0, i, 0), 24, 0, 0, 1) for i in range(15)]
    r += [(ipv4(210, 0, i >> 8, i & 255), 32, ipv4(110, 0, i >> 8, i & 255), 32, 0) for i in range(4096)]
    return np.array(r, np.uint32)


def from_rules(rng, rules, k):
    """k packets, each inside a randomly picked rule: the bits beyond the prefix are random."""
    pick = rules[rng.integers(0, len(rules), k)]
    ms, md = masks(pick[:, 1]), masks(pick[:, 3])
    rs, rd = rng.integers(0, 1 << 32, k, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, k, dtype=np.uint64).astype(np.uint32)
    return (pick[:, 0] & ms) | (rs & ~ms), (pick[:, 2] & md) | (rd & ~md), pick


def set_a(rng):
    rules = init_rules()
    src, dst = [], []
    for lo, hi, k in ((0, 100, 350), (100, 115, 300), (115, 130, 300), (130, 4226, 500)):
        s, d, _ = from_rules(rng, rules[lo:hi], k)
        src.append(s)
        dst.append(d)
    s, _, _ = from_rules(rng, rules[100:130], 100)       # a src deny and a dst deny at once: the dst rule is earlier
    _, d, _ = from_rules(rng, rules[0:100], 100)
    src.append(s)
    dst.append(d)
    i, j = rng.integers(0, 4096, 150), rng.integers(0, 4096, 150)   # allow pairs with the wrong partner
    src.append(rules[130 + i, 0])
    dst.append(rules[130 + j, 2])
    k = 2048 - sum(len(x) for x in src)
    src.append(rng.integers(0, 1 << 32, k, dtype=np.uint64).astype(np.uint32))
    dst.append(rng.integers(0, 1 << 32, k, dtype=np.uint64).astype(np.uint32))
    return rules, np.concatenate(src), np.concatenate(dst)


def set_b(rng):
    pool = (rng.integers(0, 1 << 31, 12, dtype=np.uint64) | (1 << 31)).astype(np.uint32)
    pool[1] = pool[0] ^ 0x00000100          # neighbours that part at /24, /17 and /9
    pool[2] = pool[0] ^ 0x00008000
    pool[3] = pool[0] ^ 0x00800000
    rules = []
    while len(rules) < 300:
        sm, dm = int(rng.choice(LENS)), int(rng.choice(LENS))
        if (sm == 0 and dm == 0) or (max(sm, dm) <= 1 and len(rules) < 200):
            continue        # the rules that take every pool address come late, or they would decide everything
        rules.append((int(rng.choice(pool)), sm, int(rng.choice(pool)), dm, int(rng.integers(0, 2))))
    rules = np.array(rules, np.uint32)
    s1, d1, _ = from_rules(rng, rules, 1400)
    s2, d2, pick = from_rules(rng, rules, 300)           # near misses: one bit inside a prefix flipped
    for k in range(300):
        sm, dm = int(pick[k, 1]), int(pick[k, 3])
        if sm and (not dm or rng.integers(0, 2)):
            s2[k] ^= np.uint32(1 << (32 - int(rng.integers(1, sm + 1))))
        else:
            d2[k] ^= np.uint32(1 << (32 - int(rng.integers(1, dm + 1))))
    s3 = rng.integers(0, 1 << 31, 348, dtype=np.uint64).astype(np.uint32)
    d3 = rng.integers(0, 1 << 31, 348, dtype=np.uint64).astype(np.uint32)
    return rules, np.concatenate([s1, s2, s3]), np.concatenate([d1, d2, d3])


def build(ref: str, tmp: str) -> str:
    os.makedirs(os.path.join(tmp, "bsd"))
    open(os.path.join(tmp, "cne_build_config.h"), "w").close()
    with open(os.path.join(tmp, "bsd", "string.h"), "w") as f:
        f.write(BSD_STRING_H)
    with open(os.path.join(tmp, "bsd", "bsd.h"), "w") as f:
        f.write("#include <bsd/string.h>\n")
    with open(os.path.join(tmp, "driver.c"), "w") as f:
        f.write(DRIVER_C)
    exe = os.path.join(tmp, "acl_golden")
    srcs = [os.path.join(ref, "lib", "usr", "clib", "acl", s) for s in ACL_SRCS]
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-w", f"-I{tmp}", *[f"-I{ref}/{d}" for d in INCS], "-o", exe,
                    os.path.join(tmp, "driver.c"), *srcs], check=True)
    return exe


def run(exe: str, rules, psrc, pdst):
    blob = np.uint32(len(rules)).tobytes() + np.ascontiguousarray(rules, np.uint32).tobytes()
    blob += np.uint32(len(psrc)).tobytes() + np.stack([psrc, pdst], 1).astype(np.uint32).tobytes()
    r = subprocess.run([exe], input=blob, capture_output=True, check=True)
    res = np.array([int(x) for x in r.stdout.split()], np.uint32)
    assert len(res) == len(psrc)
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("CNDP_REF", "/root/reference"))
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    rng = np.random.default_rng(0xAC1)
    sets = {}
    for name, (rules, psrc, pdst) in (("a", set_a(rng)), ("b", set_b(rng))):
        perm = rng.permutation(len(psrc))
        sets[name] = (rules, psrc[perm], pdst[perm])
    rb, ps, pd = sets["b"]
    sets["b0"] = (np.concatenate([rb[:150], np.array([(0, 0, 0, 0, 0)], np.uint32), rb[150:]]), ps, pd)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(a.ref, tmp)
        for name, (rules, psrc, pdst) in sets.items():
            res = run(exe, rules, psrc, pdst)
            out.update({f"{name}_src_addr": rules[:, 0], f"{name}_src_msk": rules[:, 1].astype(np.uint8),
                        f"{name}_dst_addr": rules[:, 2], f"{name}_dst_msk": rules[:, 3].astype(np.uint8),
                        f"{name}_deny": rules[:, 4].astype(np.uint8), f"{name}_psrc": psrc, f"{name}_pdst": pdst,
                        f"{name}_res": res})
            print(f"set {name}: {len(rules)} rules, {len(psrc)} packets, {int(np.count_nonzero(res))} match, "
                  f"{int(np.count_nonzero(res & 0xF0000000))} of them deny, {len(np.unique(res))} distinct results")
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())

/* The per-frame rule behind include/cndp_cfwd.h, shared by cfwd.c (host, plain
 * C) and cndp_cfwd.hip (the kernel), so that the two cannot drift. */
#ifndef CNDP_CFWD_INTERNAL_H
#define CNDP_CFWD_INTERNAL_H

#include <stdint.h>

#include "../../include/cndp_cfwd.h"

#if defined(__HIPCC__)
#define CFWD_HD __host__ __device__
#else
#define CFWD_HD
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* What the rule reads of a frame: bytes 0-11 as three little-endian dwords,
 * byte 22, bytes 24-25 and bytes 30-33 as little-endian loads give them. */
struct cfwd_frame {
    uint32_t d0, d1, d2;
    uint32_t ttl, ck, dst;
};

/* What it leaves: the same fields as they are to be stored (FWD: d0-d2; L3FWD:
 * ttl, ck, d0 and the low half of d1, all of d0-d2 when echoed), and the outputs. */
struct cfwd_edit {
    uint32_t d0, d1, d2;
    uint32_t ttl, ck;
    uint64_t nh;
    uint32_t tx, echo;
};

/* jcfg_lport_by_index(port) != NULL */
static inline CFWD_HD int cfwd_known(uint32_t port, uint64_t m0, uint64_t m1, uint64_t m2, uint64_t m3)
{
    const uint64_t m = port < 64u ? m0 : port < 128u ? m1 : port < 192u ? m2 : m3;
    return port < 256u && ((m >> (port & 63u)) & 1u);
}

/* One frame of _l3fwd_test (main.c:277-299) or _fwd_test (main.c:180-191).
 * t24 / t8 are a DIR-24-8 image of 8-byte entries in lpm4()'s format (entry =
 * nh << 1, or (group << 1) | 1 when extended; tbl8 entries (nh << 1) | 1); they
 * are read in L3FWD mode only.  The tbl24 load comes first so that the TTL and
 * checksum arithmetic runs while it is in flight. */
static inline CFWD_HD void cfwd_rule(uint32_t mode, const struct cfwd_frame *f, const uint64_t *t24, const uint64_t *t8,
                                     uint64_t m0, uint64_t m1, uint64_t m2, uint64_t m3, uint32_t in_lport,
                                     struct cfwd_edit *o)
{
    uint64_t nh = 0;
    uint32_t port, ttl = f->ttl, ck = f->ck;
    if (mode == CNDP_CFWD_L3FWD) {
        const uint32_t ip = __builtin_bswap32(f->dst); /* main.c:282 */
        uint64_t e = t24[ip >> 8];
        /* ipv4_adjust_cksum, main.c:230-236; htobe16(0xFEFF) is 0xFFFE on the little-endian host */
        ttl = (ttl - 1u) & 0xffu;
        const uint32_t c = (ck ^ 0xFFFFu) + 0xFFFEu;
        ck = ~(c + (c >> 16)) & 0xFFFFu;
        if (e & 1u)
            e = t8[(e >> 1) * 256u + (ip & 0xffu)];
        nh = e >> 1;
        port = (uint32_t)(nh >> 48) & 0xFFFFu; /* l3-fwd.c:89 */
    } else {
        port = (f->d1 >> 8) & 0xffu; /* get_dst_lport: p[5], before the swap */
    }
    const int known = cfwd_known(port, m0, m1, m2, m3);
    if (mode == CNDP_CFWD_L3FWD && known) {
        /* MAC_REWRITE with inet_h64tom(nh): octet[0] = bits 47..40 ... octet[5] = bits 7..0 */
        o->d0 = __builtin_bswap32((uint32_t)(nh >> 16));
        o->d1 = (f->d1 & 0xFFFF0000u) | (uint32_t)((nh >> 8) & 0xffu) | (uint32_t)(nh & 0xffu) << 8;
        o->d2 = f->d2;
    } else {
        /* MAC_SWAP: bytes 6-11 in front of bytes 0-5 */
        o->d0 = (f->d1 >> 16) | (f->d2 << 16);
        o->d1 = (f->d2 >> 16) | (f->d0 << 16);
        o->d2 = (f->d0 >> 16) | (f->d1 << 16);
    }
    o->ttl = ttl;
    o->ck = ck;
    o->nh = nh;
    o->tx = known ? port : in_lport;
    o->echo = !known;
}

/* argument checks shared by the host twin and the GPU call: 0 or -EINVAL.  A
 * FIB given in L3FWD mode must have 8-byte entries. */
int cfwd_io_check(struct cne_fib *fib, const struct cndp_batch *b, uint32_t mode, const struct cndp_cfwd_io *io);

#ifdef __cplusplus
}
#endif
#endif

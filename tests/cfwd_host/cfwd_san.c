/* cfwd.c under -fsanitize=address,undefined over real FIBs (fib.c, rib.c):
 * the helpers' packing and refusals, both modes over heap slabs sized exactly
 * to their last byte (packed slots, odd byte offsets, every cut of the last
 * frame), selection, the argument checks, random route changes with bursts
 * between.  Prints PASS and exits 0; any check that fails exits 1, a sanitizer
 * report aborts. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cndp_amd/csrc/cfwd_internal.h"
#include "../../cndp_amd/csrc/fib_internal.h"

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            exit(1);                                                 \
        }                                                            \
    } while (0)

/* the FIBs' device side lives in cndp_gpu.hip; this program has no device */
int cndp_tbl_dev_sync(struct cndp_tbl *t, void *s) { (void)t, (void)s; return -ENODEV; }
void cndp_tbl_dev_free(struct cndp_tbl *t) { (void)t; }
int cndp_tbl_lookup4_host(struct cndp_tbl *t, const uint32_t *i, uint64_t *n, uint32_t c) { (void)t, (void)i, (void)n, (void)c; return -ENODEV; }
int cndp_tbl_lookup6_host(struct cndp_tbl *t, const uint8_t *i, uint64_t *n, uint32_t c) { (void)t, (void)i, (void)n, (void)c; return -ENODEV; }
int cndp_tbl_lookup4_dev(struct cndp_tbl *t, const uint32_t *i, uint64_t *n, uint32_t c, void *s) { (void)t, (void)i, (void)n, (void)c, (void)s; return -ENODEV; }
int cndp_tbl_lookup6_dev(struct cndp_tbl *t, const uint8_t *i, uint64_t *n, uint32_t c, void *s) { (void)t, (void)i, (void)n, (void)c, (void)s; return -ENODEV; }

static uint32_t rnd_state = 777;
static uint32_t rnd(uint32_t m)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return (rnd_state >> 8) % m;
}

enum { N = 67, SLOT = 64 };

/* frame i of a burst: MACs 02:00:00:00:00:<i % 5> <- 02:11:22:33:44:55, TTL i, checksum i * 257, dst ip */
static void mkframe(uint8_t *p, uint32_t i, uint32_t ip)
{
    memset(p, 0xA5, SLOT);
    const uint8_t hdr[12] = {2, 0, 0, 0, 0, (uint8_t)(i % 5), 2, 0x11, 0x22, 0x33, 0x44, 0x55};
    memcpy(p, hdr, 12);
    p[22] = (uint8_t)i;
    p[24] = (uint8_t)i, p[25] = (uint8_t)i;
    p[30] = (uint8_t)(ip >> 24), p[31] = (uint8_t)(ip >> 16), p[32] = (uint8_t)(ip >> 8), p[33] = (uint8_t)ip;
}

static uint32_t dst_of(uint32_t i)
{
    static const uint32_t d[6] = {0x0a010203u, 0x0a010280u, 0x0a010281u, 0x0b000001u, 0x0c000001u, 0x0a020001u};
    return d[i % 6];
}

int main(void)
{
    const uint8_t macA[6] = {2, 0xaa, 0, 0, 0, 1}, macB[6] = {2, 0xbb, 0, 0, 0, 2}, macC[6] = {2, 0xcc, 0, 0, 0, 3};
    CHECK(cndp_cfwd_nexthop(macA, 7) == 0x000702aa00000001ull && cndp_cfwd_nexthop(NULL, 7) == 0);
    CHECK(cndp_cfwd_nexthop(macB, 0xFFFF) == 0xFFFF02bb00000002ull);
    CHECK(cndp_cfwd_fib_create(NULL) == NULL);
    struct cne_fib *fib = cndp_cfwd_fib_create("l3fwd_fib");
    CHECK(fib && fib->type == CNE_FIB_DUMMY && fib->def_nh == CNDP_CFWD_DEFAULT_NH && fib->t.nh_sz == 3);
    CHECK(cndp_cfwd_route_add(NULL, 0, 0, macA, 0) == -EINVAL && cndp_cfwd_route_add(fib, 0, 0, NULL, 0) == -EINVAL);
    CHECK(cndp_cfwd_route_add(fib, 0, 0, macA, 0x8000) == -EINVAL && cndp_cfwd_route_add(fib, 0, 33, macA, 0) == -EINVAL);
    CHECK(cndp_cfwd_route_add(fib, 0x0a010200u, 24, macA, 1) == 0);      /* 10.1.2/24 -> port 1 */
    CHECK(cndp_cfwd_route_add(fib, 0x0a010280u, 25, macB, 2) == 0);      /* 10.1.2.128/25 -> port 2 (tbl8) */
    CHECK(cndp_cfwd_route_add(fib, 0x0a010281u, 32, macC, 0x7FFF) == 0); /* 10.1.2.129/32 -> port 0x7FFF */
    CHECK(cndp_cfwd_route_add(fib, 0x0b000000u, 8, macC, 9) == 0);       /* 11/8 -> port 9, not in the mask */
    CHECK(cndp_cfwd_route_add(fib, 0x0a020000u, 16, macB, 256) == 0 && cne_fib_delete(fib, 0x0a020000u, 16) == 0);

    struct cne_fib_conf c4;
    memset(&c4, 0, sizeof(c4));
    c4.type = CNE_FIB_DIR24_8, c4.max_routes = 64, c4.dir24_8.nh_sz = CNE_FIB_DIR24_8_4B, c4.dir24_8.num_tbl8 = 16;
    struct cne_fib *f4 = cne_fib_create("narrow", &c4);
    c4.dir24_8.nh_sz = CNE_FIB_DIR24_8_8B;
    c4.default_nh = CNDP_CFWD_DEFAULT_NH;
    struct cne_fib *f8 = cne_fib_create("wide", &c4);
    CHECK(f4 && f8 && cndp_cfwd_route_add(f8, 0x0a010281u, 32, macC, 0x7FFF) == 0);

    struct cndp_cfwd_io io;
    memset(&io, 0, sizeof(io));
    uint64_t nh[N], stats[CNDP_CFWD_NSTATS] = {0, 0};
    uint16_t tx[N], bin[N];
    uint8_t echoed[N], sel[N];
    io.in_lport = 3;
    io.lport_mask[0] = 1u << 0 | 1u << 1 | 1u << 2 | 1u << 3;
    io.nh = nh, io.tx_lport = tx, io.echoed = echoed, io.bin_of = bin, io.n_bins = 4, io.stats = stats;

    /* argument checks */
    struct cndp_batch b;
    memset(&b, 0, sizeof(b));
    uint8_t one[SLOT];
    mkframe(one, 1, dst_of(0));
    b.n = 1, b.slab = one, b.slab_len = SLOT, b.stride = SLOT;
    CHECK(cndp_cfwd_host(fib, NULL, CNDP_CFWD_L3FWD, &io) == -EINVAL && cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, NULL) == -EINVAL);
    CHECK(cndp_cfwd_host(fib, &b, 2, &io) == -EINVAL && cndp_cfwd_host(NULL, &b, CNDP_CFWD_L3FWD, &io) == -EINVAL);
    CHECK(cndp_cfwd_host(f4, &b, CNDP_CFWD_L3FWD, &io) == -EINVAL);
    io.n_bins = 3;
    CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == -EINVAL);
    io.n_bins = CNDP_PART_BINS_MAX + 1;
    CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == -EINVAL);
    io.n_bins = 4, io.in_lport = 256;
    CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == -EINVAL);
    io.in_lport = 3, io.tx_lport = NULL;
    CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == -EINVAL);
    io.tx_lport = tx, b.slab = NULL;
    CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == -EINVAL);
    b.slab = one, b.slab_len = 1ull << 63;
    CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == -EINVAL);
    b.slab_len = SLOT;
    uint8_t keep[SLOT];
    memcpy(keep, one, SLOT);
    CHECK(memcmp(one, keep, SLOT) == 0 && stats[0] == 0 && stats[1] == 0); /* a refused call writes nothing */
    b.n = 0, b.slab = NULL;
    CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == 0 && cndp_cfwd_host(NULL, &b, CNDP_CFWD_FWD, &io) == 0);

    /* one frame through the 8-byte DIR-24-8 FIB: the same answer as the DUMMY one */
    b.n = 1, b.slab = one;
    CHECK(cndp_cfwd_host(f8, &b, CNDP_CFWD_L3FWD, &io) == 0 && nh[0] == CNDP_CFWD_DEFAULT_NH && tx[0] == 0);
    CHECK(one[22] == 0 && one[0] == 0xff && one[5] == 0xff && one[6] == 2 && one[11] == 0x55);

    /* every cut of the slab inside the last frame, packed slots on an exact heap block */
    for (int mode = CNDP_CFWD_FWD; mode <= (int)CNDP_CFWD_L3FWD; mode++)
        for (uint32_t cut = 0; cut <= 36; cut++) {
            const size_t len = (size_t)(N - 1) * SLOT + cut;
            uint8_t *slab = malloc(len ? len : 1), *orig = malloc(len ? len : 1);
            CHECK(slab && orig);
            for (uint32_t i = 0; i < N; i++) {
                uint8_t f[SLOT];
                mkframe(f, i, dst_of(i));
                const size_t at = (size_t)i * SLOT, take = at >= len ? 0 : len - at < SLOT ? len - at : SLOT;
                memcpy(slab + at, f, take);
                sel[i] = i % 7 != 3;
            }
            memcpy(orig, slab, len);
            b.n = N, b.slab = slab, b.slab_len = len, b.stride = SLOT, b.offsets = NULL, b.data_off = 0;
            io.sel = cut & 1 ? sel : NULL;
            stats[0] = stats[1] = 0;
            CHECK(cndp_cfwd_host(fib, &b, (uint32_t)mode, &io) == 0);
            uint64_t taken = 0;
            for (uint32_t i = 0; i < N; i++) {
                const uint8_t *p = slab + (size_t)i * SLOT, *o = orig + (size_t)i * SLOT;
                if (io.sel && !sel[i]) {
                    CHECK(tx[i] == CNDP_CFWD_LPORT_NONE && bin[i] == 4 && nh[i] == 0 && echoed[i] == 0);
                    CHECK(i == N - 1 || memcmp(p, o, SLOT) == 0);
                    continue;
                }
                taken++;
                CHECK(bin[i] == tx[i] && tx[i] < 4);
                if (i == N - 1)
                    continue; /* the cut frame: the sanitizer watches its edge, tests/test_cfwd_host.py its bytes */
                CHECK(memcmp(p + 26, o + 26, SLOT - 26) == 0 && memcmp(p + 12, o + 12, 10) == 0 && p[23] == o[23]);
                if (mode == (int)CNDP_CFWD_FWD) {
                    CHECK(nh[i] == 0 && memcmp(p, o + 6, 6) == 0 && memcmp(p + 6, o, 6) == 0 && p[22] == o[22]);
                    CHECK(tx[i] == (i % 5 < 4 ? i % 5 : 3) && echoed[i] == (i % 5 == 4));
                    continue;
                }
                CHECK(p[22] == (uint8_t)(o[22] - 1));
                const uint32_t ck = o[24] | (uint32_t)o[25] << 8, c = (ck ^ 0xFFFFu) + 0xFFFEu, want = ~(c + (c >> 16)) & 0xFFFFu;
                CHECK((p[24] | (uint32_t)p[25] << 8) == want);
                switch (i % 6) {
                case 0: /* 10.1.2.3 by the /24 */
                    CHECK(nh[i] == cndp_cfwd_nexthop(macA, 1) && tx[i] == 1 && !echoed[i] && !memcmp(p, macA, 6) && !memcmp(p + 6, o + 6, 6));
                    break;
                case 1: /* 10.1.2.128 by the /25 */
                    CHECK(nh[i] == cndp_cfwd_nexthop(macB, 2) && tx[i] == 2 && !memcmp(p, macB, 6));
                    break;
                case 2: /* 10.1.2.129 by the /32: port 0x7FFF is unknown, echoed */
                    CHECK(nh[i] == cndp_cfwd_nexthop(macC, 0x7FFF) && tx[i] == 3 && echoed[i] && !memcmp(p, o + 6, 6) && !memcmp(p + 6, o, 6));
                    break;
                case 3: /* 11.0.0.1: port 9 is not in the mask */
                    CHECK(tx[i] == 3 && echoed[i] && !memcmp(p, o + 6, 6));
                    break;
                default: /* 12.0.0.1 and 10.2.0.1 (route deleted): a miss goes to port 0, broadcast */
                    CHECK(nh[i] == CNDP_CFWD_DEFAULT_NH && tx[i] == 0 && !echoed[i] && p[0] == 0xff && p[5] == 0xff && !memcmp(p + 6, o + 6, 6));
                }
            }
            CHECK(stats[0] + stats[1] == taken);
            free(slab);
            free(orig);
        }

    /* odd byte offsets, the last frame ending with the block */
    {
        uint64_t offs[N];
        size_t at = 1;
        for (uint32_t i = 0; i < N; i++) {
            offs[i] = at - 1;
            at += 34 + 2 * rnd(8);
        }
        const size_t len = (size_t)offs[N - 1] + 1 + 34;
        uint8_t *slab = malloc(len);
        CHECK(slab);
        for (uint32_t i = 0; i < N; i++) {
            uint8_t f[SLOT];
            mkframe(f, i, dst_of(i));
            memcpy(slab + offs[i] + 1, f, 34);
        }
        b.n = N, b.slab = slab, b.slab_len = len, b.stride = 0, b.offsets = offs, b.data_off = 1;
        io.sel = NULL;
        CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == 0);
        for (uint32_t i = 0; i < N; i++)
            CHECK(slab[offs[i] + 1 + 22] == (uint8_t)(i - 1) && (i % 6 != 0 || !memcmp(slab + offs[i] + 1, macA, 6)));
        /* a frame that starts past the end and one whose offset wraps: read as zeros, nothing written */
        offs[0] = len + 5, offs[1] = ~0ull - 3;
        CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == 0 && nh[0] == CNDP_CFWD_DEFAULT_NH && nh[1] == CNDP_CFWD_DEFAULT_NH);
        free(slab);
    }

    /* random route changes with bursts between: every answer is a port of the mask */
    uint8_t *slab = malloc((size_t)N * SLOT);
    CHECK(slab);
    b.n = N, b.slab = slab, b.slab_len = (size_t)N * SLOT, b.stride = SLOT, b.offsets = NULL, b.data_off = 0;
    for (int it = 0; it < 3000; it++) {
        const uint32_t k = rnd(4), ip = 0x0a010000u + (rnd(4) << 8) + rnd(4) * 64u;
        static const uint8_t depths[5] = {16, 24, 26, 31, 32};
        const uint8_t depth = depths[rnd(5)];
        int rc = 0;
        if (k < 2) {
            rc = cndp_cfwd_route_add(fib, ip, depth, k ? macA : macB, (uint16_t)rnd(6));
        } else if (k == 2) {
            rc = cne_fib_delete(fib, ip, depth);
            rc = rc == -ENOENT ? 0 : rc;
        } else {
            for (uint32_t i = 0; i < N; i++)
                mkframe(slab + (size_t)i * SLOT, i, 0x0a010000u + (rnd(4) << 8) + rnd(256));
            CHECK(cndp_cfwd_host(fib, &b, CNDP_CFWD_L3FWD, &io) == 0);
            for (uint32_t i = 0; i < N; i++)
                CHECK(tx[i] < 4 && (echoed[i] == 0 || tx[i] == 3));
        }
        CHECK(rc == 0);
    }
    free(slab);
    cne_fib_free(fib);
    cne_fib_free(f4);
    cne_fib_free(f8);
    puts("PASS");
    return 0;
}

/* fib_near.c under -fsanitize=address,undefined over real FIBs (fib.c, rib.c):
 * the sequences of tests/test_fib_near_image.py -- an empty FIB, nested routes
 * in one /8, three /8s, deletes that free a /16 page and a /8 slot, re-adds
 * that reuse them, a route set over the cap -- with the near lookup compared
 * with the plain tbl24 / tbl8 lookup after each.  Prints PASS and exits 0; a
 * check that fails exits 1, a sanitizer report aborts. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static uint32_t rnd_state = 99;
static uint32_t rnd32(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    const uint32_t hi = rnd_state >> 16;
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return (hi << 16) | (rnd_state >> 16);
}

struct route {
    uint32_t ip;
    uint8_t depth;
    uint32_t nh;
};

static uint64_t plain(const struct cndp_fib_image *im, uint32_t ip)
{
    uint32_t e = ((const uint32_t *)im->tbl24)[ip >> 8];
    if (e & 1u)
        e = ((const uint32_t *)im->tbl8)[(size_t)(e >> 1) * 256 + (ip & 0xff)];
    return e >> 1;
}

/* the near lookup equals the plain one on the routes' edges and a random sample */
static void compare(struct cne_fib *f, const struct route *r, uint32_t nr)
{
    enum { N = 1 << 16 };
    static uint32_t ips[N];
    static uint64_t nh[N];
    uint32_t n = 0;
    for (uint32_t k = 0; k < nr; k++) {
        const uint32_t last = r[k].ip | (r[k].depth == 32 ? 0u : (0xffffffffu >> r[k].depth));
        const uint32_t e[6] = {r[k].ip - 1, r[k].ip, r[k].ip + 1, last - 1, last, last + 1};
        memcpy(ips + n, e, sizeof(e));
        n += 6;
    }
    while (n < N) {
        const uint32_t x = rnd32();
        /* half of the sample inside the routed /8s */
        ips[n] = (n & 1u) && nr ? (r[x % nr].ip & 0xff000000u) | (x & 0x00ffffffu) : x;
        n++;
    }
    CHECK(cndp_fib_near_lookup(f, ips, nh, N) == 0);
    struct cndp_fib_image im;
    CHECK(cndp_fib_image(f, &im) == 0 && im.nh_sz == 2);
    for (uint32_t k = 0; k < N; k++)
        CHECK(nh[k] == plain(&im, ips[k]));
}

static struct cne_fib *mkfib(const char *name, int nh_sz)
{
    struct cne_fib_conf c;
    memset(&c, 0, sizeof(c));
    c.type = CNE_FIB_DIR24_8;
    c.default_nh = 77;
    c.max_routes = 1024;
    c.dir24_8.nh_sz = nh_sz;
    c.dir24_8.num_tbl8 = 256;
    return cne_fib_create(name, &c);
}

int main(void)
{
    struct cndp_fib_near_info in;
    struct cne_fib *f = mkfib("near", CNE_FIB_DIR24_8_4B);
    CHECK(f);
    CHECK(cndp_fib_near_refresh(NULL) == -EINVAL && cndp_fib_near_info(f, NULL) == -EINVAL);
    CHECK(cndp_fib_near_info(f, &in) == -ENOENT);
    /* empty: the default route only, one page */
    compare(f, NULL, 0);
    CHECK(cndp_fib_near_info(f, &in) == 0 && in.kib == 1 && in.fits == 1 && in.cap_kib == CNDP_NEAR_CAP_KIB);
    /* nested in one /8, then two more /8s */
    const struct route rs[] = {{0x14000000, 8, 1},  {0x14100000, 12, 2}, {0x14100000, 16, 3}, {0x14108000, 17, 4},
                               {0x1410C800, 24, 5}, {0x1410C880, 25, 6}, {0x1410C881, 32, 7}, {0x1E010000, 16, 8},
                               {0x28020300, 24, 9}};
    enum { NR = sizeof(rs) / sizeof(rs[0]) };
    for (uint32_t k = 0; k < NR; k++) {
        CHECK(cne_fib_add(f, rs[k].ip, rs[k].depth, rs[k].nh) == 0);
        compare(f, rs, k + 1);
    }
    /* 20/8: /16 pages for 20.16 only (20.16/16 holds the /17.. /32); 30.1/16 is uniform; 40.2/16 a page */
    CHECK(cndp_fib_near_info(f, &in) == 0 && in.mid_used == 3 && in.pages_used == 2 && in.kib == 6);
    /* a /16 uniform again: its page freed, and with it 40/8's slot */
    CHECK(cne_fib_delete(f, 0x28020300, 24) == 0);
    compare(f, rs, NR);
    CHECK(cndp_fib_near_info(f, &in) == 0 && in.mid_used == 2 && in.pages_used == 1 && in.kib == 6);
    /* a /8 uniform again: its slot freed */
    CHECK(cne_fib_delete(f, 0x1E010000, 16) == 0);
    compare(f, rs, NR);
    CHECK(cndp_fib_near_info(f, &in) == 0 && in.mid_used == 1);
    /* re-adds reuse the freed slots and page: the high-water marks stay */
    CHECK(cne_fib_add(f, 0x28020300, 24, 9) == 0 && cne_fib_add(f, 0x1E010000, 16, 8) == 0);
    compare(f, rs, NR);
    CHECK(cndp_fib_near_info(f, &in) == 0 && in.mid_used == 3 && in.mid_hwm == 3 && in.pages_used == 2 &&
          in.page_hwm == 2 && in.kib == 6 && in.fits == 1);
    /* over the cap: 40 /24s in 40 /8s, 1 + (3 + 40) + (2 + 40) pages; still exact, reported as not fitting */
    struct route big[NR + 40];
    memcpy(big, rs, sizeof(rs));
    for (uint32_t k = 0; k < 40; k++) {
        big[NR + k] = (struct route){((50 + k) << 24) | (k << 16) | (k << 8), 24, 100 + k};
        CHECK(cne_fib_add(f, big[NR + k].ip, 24, big[NR + k].nh) == 0);
    }
    compare(f, big, NR + 40);
    CHECK(cndp_fib_near_info(f, &in) == 0 && in.fits == 0 && in.kib == 86 && in.mid_used == 43);
    /* random churn over many /8s: every slot and page id stays inside its array */
    for (uint32_t it = 0; it < 300; it++) {
        const uint32_t x = rnd32();
        const uint8_t d = (uint8_t)(8 + x % 25);
        const uint32_t ip = (rnd32() & 0xff3f0000u) | (x & 0xff00u) | (rnd32() & 0xffu);
        const uint32_t net = d == 32 ? ip : ip & ~(0xffffffffu >> d);
        if (x & 0x10000u)
            (void)cne_fib_delete(f, net, d);
        else
            (void)cne_fib_add(f, net, d, 200 + it % 50);
        if (it % 25 == 0)
            compare(f, big, NR + 40);
    }
    compare(f, big, NR + 40);
    cne_fib_free(f);
    /* a table the directory does not exist for */
    struct cne_fib *f8 = mkfib("wide", CNE_FIB_DIR24_8_8B);
    CHECK(f8 && cndp_fib_near_refresh(f8) == -ENOTSUP && cndp_fib_near_info(f8, &in) == -ENOENT);
    cne_fib_free(f8);
    puts("PASS");
    return 0;
}

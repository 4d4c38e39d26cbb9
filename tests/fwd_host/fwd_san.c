/* fwd.c under -fsanitize=address,undefined over real FIBs: argument checks,
 * set / clear sequences at both ends of the object arrays, the 1-wide rule's
 * every outcome, random changes with lookups between.  Prints PASS and exits 0;
 * any check that fails exits 1, a sanitizer report aborts. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cndp_amd/csrc/fwd_internal.h"

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

static uint32_t rnd_state = 4242;
static uint32_t rnd(uint32_t m)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return (rnd_state >> 8) % m;
}

static struct cne_fib *mkfib(const char *name, enum cne_fib_type type, int nh_sz, uint64_t def)
{
    struct cne_fib_conf c;
    memset(&c, 0, sizeof(c));
    c.type = type;
    c.default_nh = def;
    c.max_routes = 1024;
    c.dir24_8.nh_sz = nh_sz;
    c.dir24_8.num_tbl8 = 64;
    return cne_fib_create(name, &c);
}

static uint32_t be(uint32_t host) { return __builtin_bswap32(host); }

int main(void)
{
    enum { ARP_N = 16, RT_N = 8 };
    struct cne_fib *arp = mkfib("arp-fib", CNE_FIB_DIR24_8, CNE_FIB_DIR24_8_4B, ARP_N + 1);
    struct cne_fib *rt4 = mkfib("rt4-fib", CNE_FIB_DIR24_8, CNE_FIB_DIR24_8_4B, RT_N + 1);
    struct cne_fib *f8 = mkfib("wide", CNE_FIB_DIR24_8, CNE_FIB_DIR24_8_8B, 0);
    struct cne_fib *dummy = mkfib("dummy", CNE_FIB_DUMMY, CNE_FIB_DIR24_8_4B, 0);
    CHECK(arp && rt4 && f8 && dummy);
    cndp_fwd_tbl_t *t = NULL;
    CHECK(cndp_fwd_create(NULL, rt4, ARP_N, RT_N, &t) == -EINVAL);
    CHECK(cndp_fwd_create(arp, NULL, ARP_N, RT_N, &t) == -EINVAL);
    CHECK(cndp_fwd_create(f8, rt4, ARP_N, RT_N, &t) == -EINVAL);
    CHECK(cndp_fwd_create(arp, dummy, ARP_N, RT_N, &t) == -EINVAL);
    CHECK(cndp_fwd_create(arp, rt4, 0, RT_N, &t) == -EINVAL);
    CHECK(cndp_fwd_create(arp, rt4, ARP_N, CNDP_FWD_OBJS_MAX + 1, &t) == -EINVAL);
    CHECK(cndp_fwd_create(arp, rt4, ARP_N, RT_N, NULL) == -EINVAL);
    CHECK(cndp_fwd_create(arp, rt4, ARP_N, RT_N, &t) == 0);
    CHECK(cndp_fwd_max_netif(t) == -1);

    const uint8_t mac0[6] = {2, 0x11, 0x22, 0x33, 0x44, 0}, mac255[6] = {2, 0x11, 0x22, 0x33, 0x44, 255};
    CHECK(cndp_fwd_netif_set(t, 0, mac0) == 0 && cndp_fwd_netif_set(t, 255, mac255) == 0);
    CHECK(cndp_fwd_netif_set(t, 256, mac0) == -EINVAL);
    struct cndp_fwd_arp a = {.netif_idx = 0, .ha = {2, 0xaa, 0, 0, 0, 1}};
    struct cndp_fwd_rt r = {.gateway = 0x0a010001u, .netif_idx = 255};
    CHECK(cndp_fwd_arp_set(t, ARP_N, &a) == -EINVAL && cndp_fwd_arp_set(t, 0, NULL) == -EINVAL);
    CHECK(cndp_fwd_rt_set(t, RT_N, &r) == -EINVAL && cndp_fwd_rt_set(t, 0, NULL) == -EINVAL);
    a.netif_idx = 256;
    CHECK(cndp_fwd_arp_set(t, 1, &a) == -EINVAL);
    a.netif_idx = 0;
    r.netif_idx = 256;
    CHECK(cndp_fwd_rt_set(t, 1, &r) == -EINVAL);
    r.netif_idx = 255;
    CHECK(cndp_fwd_arp_clear(t, 1) == -ENOENT && cndp_fwd_rt_clear(t, 1) == -ENOENT);
    CHECK(cndp_fwd_arp_clear(t, ARP_N) == -EINVAL && cndp_fwd_rt_clear(t, RT_N) == -EINVAL);
    /* both ends of both arrays */
    CHECK(cndp_fwd_arp_set(t, 1, &a) == 0 && cndp_fwd_arp_set(t, ARP_N - 1, &a) == 0 && cndp_fwd_arp_set(t, 0, &a) == 0);
    CHECK(cndp_fwd_rt_set(t, 1, &r) == 0 && cndp_fwd_rt_set(t, RT_N - 1, &r) == 0 && cndp_fwd_rt_set(t, 0, &r) == 0);
    CHECK(cndp_fwd_max_netif(t) == 255);

    /* 10.1.0.1 direct; 10.2/16 via gateway 10.1.0.1 (stored as its own FIB key);
     * 10.3/16 route 2 not set; 10.4.0.1 ARP value at capacity; the rest default */
    CHECK(cne_fib_add(arp, 0x0a010001u, 32, 1) == 0 && cne_fib_add(rt4, 0x0a020000u, 16, 1) == 0);
    CHECK(cne_fib_add(rt4, 0x0a030000u, 16, 2) == 0 && cne_fib_add(arp, 0x0a040001u, 32, ARP_N) == 0);
    uint32_t dst[5] = {be(0x0a010001u), be(0x0a020304u), be(0x0a030304u), be(0x0a040001u), be(0xc0000201u)};
    struct cndp_fwd_result o[5];
    CHECK(cndp_fwd_lookup(t, dst, 5, o) == 0);
    CHECK(o[0].edge == 2 && !memcmp(o[0].s_addr, mac0, 6) && !memcmp(o[0].d_addr, a.ha, 6));
    CHECK(o[1].edge == 257 && !memcmp(o[1].s_addr, mac255, 6) && !memcmp(o[1].d_addr, a.ha, 6));
    for (int k = 2; k < 5; k++)
        CHECK(o[k].edge == CNDP_FWD_EDGE_ARP_REQUEST && o[k].s_addr[0] == 0 && o[k].d_addr[5] == 0);
    CHECK(cndp_fwd_arp_clear(t, 1) == 0);
    CHECK(cndp_fwd_lookup(t, dst, 2, o) == 0 && o[0].edge == 1 && o[1].edge == 1);
    CHECK(cndp_fwd_lookup(t, NULL, 0, NULL) == 0 && cndp_fwd_lookup(t, NULL, 1, o) == -EINVAL);
    CHECK(cndp_fwd_lookup(NULL, dst, 1, o) == -EINVAL);

    /* random changes, lookups between: every answer names a set object's netif */
    for (int it = 0; it < 4000; it++) {
        uint32_t k = rnd(8);
        a.netif_idx = (uint16_t)rnd(4);
        a.ha[5] = (uint8_t)rnd(256);
        r.netif_idx = (uint16_t)rnd(4);
        r.gateway = 0x0a010000u + rnd(4);
        int rc = 0;
        if (k == 0)
            rc = cndp_fwd_arp_set(t, rnd(ARP_N), &a);
        else if (k == 1)
            rc = cndp_fwd_arp_clear(t, rnd(ARP_N));
        else if (k == 2)
            rc = cndp_fwd_rt_set(t, rnd(RT_N), &r);
        else if (k == 3)
            rc = cndp_fwd_rt_clear(t, rnd(RT_N));
        else if (k == 4)
            rc = cne_fib_add(arp, 0x0a010000u + rnd(4), 32, rnd(ARP_N + 2));
        else if (k == 5)
            rc = cne_fib_add(rt4, 0x0a020000u + (rnd(4) << 8), 24, rnd(RT_N + 2));
        else if (k == 6) {
            rc = cne_fib_delete(arp, 0x0a010000u + rnd(4), 32);
            rc = rc == -ENOENT ? 0 : rc;
        } else {
            uint32_t d[8];
            struct cndp_fwd_result q[8];
            for (int j = 0; j < 8; j++)
                d[j] = be(rnd(2) ? 0x0a010000u + rnd(4) : 0x0a020000u + (rnd(4) << 8) + rnd(256));
            CHECK(cndp_fwd_lookup(t, d, 8, q) == 0);
            for (int j = 0; j < 8; j++)
                CHECK(q[j].edge == 1 || (q[j].edge >= 2 && q[j].edge < 2 + 4) || q[j].edge == 257);
        }
        CHECK(rc == 0 || rc == -ENOENT);
    }
    int mx = cndp_fwd_max_netif(t);
    CHECK(mx >= -1 && mx < 256);
    cndp_fwd_free(t);
    cndp_fwd_free(NULL);

    /* the largest capacities allocate and free */
    CHECK(cndp_fwd_create(arp, rt4, CNDP_FWD_OBJS_MAX, 1, &t) == 0);
    CHECK(cndp_fwd_arp_set(t, CNDP_FWD_OBJS_MAX - 1, &a) == 0);
    cndp_fwd_free(t);
    cne_fib_free(arp);
    cne_fib_free(rt4);
    cne_fib_free(f8);
    cne_fib_free(dummy);
    puts("PASS");
    return 0;
}

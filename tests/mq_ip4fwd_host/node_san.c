/* cndp_fwd_node_host (fwd.c) under -fsanitize=address,undefined over real FIBs
 * and mbufs whose buffers are heap blocks of exactly buf_len bytes, so that any
 * access past what the node may read or write is a sanitizer report: argument
 * checks, bursts of 1 ... 256 with their tails, the group rules, every l2_len
 * (0, 2, 14, 18, 22, and above data_off), every alignment of the frame, frames
 * that cross the readable end byte by byte (buf_len, and readable_end), members
 * that are not taken.  Prints PASS and exits 0; a check that fails exits 1, a
 * sanitizer report aborts. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cndp_amd/csrc/fwd_internal.h"
#include "../../include/cndp_mqcnet.h"

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

static struct cne_fib *mkfib(const char *name, uint64_t def)
{
    struct cne_fib_conf c;
    memset(&c, 0, sizeof(c));
    c.type = CNE_FIB_DIR24_8;
    c.default_nh = def;
    c.max_routes = 1024;
    c.dir24_8.nh_sz = CNE_FIB_DIR24_8_4B;
    c.dir24_8.num_tbl8 = 64;
    return cne_fib_create(name, &c);
}

/* pktmbuf_t as the node reads it (pktmbuf.h:102-204), 64 bytes */
struct mbuf {
    uint64_t pooldata;
    uint8_t *buf_addr;
    uint32_t hash, meta_index;
    uint16_t data_off, lport, buf_len, data_len;
    uint32_t packet_type;
    uint16_t refcnt, rsvd16;
    uint64_t tx_offload, ol_flags, udata64;
};
_Static_assert(sizeof(struct mbuf) == 64, "pktmbuf_t is 64 bytes");

enum { NMB = 256 };
static struct mbuf mb[NMB];
static void *ptr[NMB];
static uint16_t edge[NMB];

/* mbuf k: a buffer of exactly buf_len bytes, an IPv4 header for dst at data_off */
static void mk(int k, uint16_t buf_len, uint16_t data_off, uint32_t l2, uint32_t dst_host, uint8_t ttl)
{
    free(mb[k].buf_addr);
    memset(&mb[k], 0, sizeof(mb[k]));
    mb[k].buf_addr = malloc(buf_len ? buf_len : 1);
    CHECK(mb[k].buf_addr);
    for (uint32_t j = 0; j < buf_len; j++)
        mb[k].buf_addr[j] = (uint8_t)rnd(256);
    mb[k].buf_len = buf_len;
    mb[k].data_off = data_off;
    mb[k].data_len = 46;
    mb[k].tx_offload = l2 | 20u << 7;
    uint8_t h[20] = {0x45, 0, 0, 46, 0, 0, 0, 0, ttl, 17, 0x12, 0x34};
    h[16] = (uint8_t)(dst_host >> 24), h[17] = (uint8_t)(dst_host >> 16), h[18] = (uint8_t)(dst_host >> 8), h[19] = (uint8_t)dst_host;
    for (uint32_t j = 0; j < 20; j++)
        if ((uint32_t)data_off + j < buf_len)
            mb[k].buf_addr[data_off + j] = h[j];
    ptr[k] = &mb[k];
}

#define DIRECT 0x0a010002u /* ARP object 2, netif 1 */
#define ROUTED 0x0a020005u /* route 1 via 10.1.0.1 (ARP object 1, netif 0), netif 2 */
#define ROUTED2 0x0a030101u /* route 2 via 10.9.0.2 (ARP object 12), netif 3 */
#define MISS 0xc0000201u

int main(void)
{
    enum { ARP_N = 16, RT_N = 8 };
    struct cne_fib *arp = mkfib("arp-fib", ARP_N + 1), *rt4 = mkfib("rt4-fib", RT_N + 1);
    CHECK(arp && rt4);
    cndp_fwd_tbl_t *t = NULL;
    CHECK(cndp_fwd_create(arp, rt4, ARP_N, RT_N, &t) == 0);
    const uint8_t mac[4][6] = {{2, 0x11, 0, 0, 0, 0}, {2, 0x11, 0, 0, 0, 1}, {2, 0x11, 0, 0, 0, 2}, {2, 0x11, 0, 0, 0, 3}};
    for (uint32_t k = 0; k < 4; k++)
        CHECK(cndp_fwd_netif_set(t, k, mac[k]) == 0);
    struct cndp_fwd_arp a1 = {.netif_idx = 0, .ha = {2, 0xaa, 0, 0, 0, 1}}, a2 = {.netif_idx = 1, .ha = {2, 0xaa, 0, 0, 0, 2}};
    struct cndp_fwd_arp a12 = {.netif_idx = 3, .ha = {2, 0xbb, 0, 0, 0, 12}}, a0 = {.netif_idx = 3, .ha = {2, 0xee, 0, 0, 0, 7}};
    struct cndp_fwd_rt r1 = {.gateway = 0x0a010001u, .netif_idx = 2}, r2 = {.gateway = 0x0a090002u, .netif_idx = 3};
    CHECK(cndp_fwd_arp_set(t, 1, &a1) == 0 && cndp_fwd_arp_set(t, 2, &a2) == 0 && cndp_fwd_arp_set(t, 12, &a12) == 0);
    CHECK(cndp_fwd_arp_set(t, 7, &a0) == 0 && cne_fib_add(arp, 0, 32, 7) == 0); /* what an unreadable destination reads as */
    CHECK(cndp_fwd_rt_set(t, 1, &r1) == 0 && cndp_fwd_rt_set(t, 2, &r2) == 0);
    CHECK(cne_fib_add(arp, 0x0a010001u, 32, 1) == 0 && cne_fib_add(arp, 0x0a010002u, 32, 2) == 0);
    CHECK(cne_fib_add(arp, 0x0a090002u, 32, 12) == 0);
    CHECK(cne_fib_add(rt4, 0x0a020000u, 16, 1) == 0 && cne_fib_add(rt4, 0x0a030000u, 16, 2) == 0);
    const uint32_t G = CNDP_MQ_EDGE_FWD_GATEWAY;

    /* arguments */
    mk(0, 512, 206, 14, DIRECT, 64);
    CHECK(cndp_fwd_node_host(NULL, ptr, 1, edge, NULL) == -EINVAL && cndp_fwd_node_host(t, NULL, 1, edge, NULL) == -EINVAL);
    CHECK(cndp_fwd_node_host(t, ptr, 1, NULL, NULL) == -EINVAL && cndp_fwd_node_host(t, ptr, 257, edge, NULL) == -EINVAL);
    CHECK(cndp_fwd_node_host(t, NULL, 0, NULL, NULL) == 0);
    CHECK(mb[0].data_off == 206 && mb[0].buf_addr[206 + 8] == 64);

    /* one mbuf, every field */
    CHECK(cndp_fwd_node_host(t, ptr, 1, edge, NULL) == 0 && edge[0] == 1 + 2);
    CHECK(mb[0].data_off == 192 && mb[0].data_len == 60 && mb[0].buf_addr[206 + 8] == 63);
    CHECK(!memcmp(mb[0].buf_addr + 192, a2.ha, 6) && !memcmp(mb[0].buf_addr + 198, mac[1], 6));
    /* ipv4_adjust_cksum on 0x3412 as loaded: ~0x3412 + 0xFFFE, folded, inverted */
    {
        const int32_t c = (int32_t)(0x3412 ^ 0xffff) + 0xfffe;
        const uint16_t ck = (uint16_t)~(uint32_t)(c + (c >> 16));
        CHECK(mb[0].buf_addr[206 + 10] == (uint8_t)ck && mb[0].buf_addr[206 + 11] == (uint8_t)(ck >> 8));
    }

    /* the group rules: a direct hit keeps the routed members off their routes; four gateways
     * take lane 0's ha; the same four one by one take their own */
    const uint32_t grp[4] = {DIRECT, ROUTED, ROUTED2, MISS};
    for (int k = 0; k < 4; k++)
        mk(k, 512, 206, 14, grp[k], 9);
    CHECK(cndp_fwd_node_host(t, ptr, 4, edge, NULL) == 0);
    CHECK(edge[0] == 3 && edge[1] == 1 && edge[2] == 1 && edge[3] == 1);
    const uint32_t gws[4] = {ROUTED, ROUTED2, ROUTED2, ROUTED};
    for (int k = 0; k < 4; k++)
        mk(k, 512, 206, 14, gws[k], 9);
    CHECK(cndp_fwd_node_host(t, ptr, 4, edge, NULL) == 0);
    CHECK(edge[0] == (4 | G) && edge[1] == (5 | G) && edge[2] == (5 | G) && edge[3] == (4 | G));
    CHECK(!memcmp(mb[1].buf_addr + 192, a1.ha, 6) && !memcmp(mb[1].buf_addr + 198, mac[3], 6));
    for (int k = 0; k < 4; k++) {
        mk(k, 512, 206, 14, gws[k], 9);
        CHECK(cndp_fwd_node_host(t, ptr + k, 1, edge + k, NULL) == 0);
    }
    CHECK(edge[1] == (5 | G) && !memcmp(mb[1].buf_addr + 192, a12.ha, 6));
    /* members not taken: NULL as lane 0 leaves the followers their own gateway's ha */
    for (int k = 0; k < 4; k++)
        mk(k, 512, 206, 14, gws[k], 9);
    ptr[0] = NULL;
    CHECK(cndp_fwd_node_host(t, ptr, 4, edge, NULL) == 0);
    CHECK(edge[0] == CNDP_FWD_EDGE_NONE && edge[1] == (5 | G) && !memcmp(mb[1].buf_addr + 192, a12.ha, 6));
    CHECK(mb[0].data_off == 206);

    /* every burst size 1 ... 256 once, random destinations, l2_len and alignment */
    const uint32_t dsts[6] = {DIRECT, ROUTED, ROUTED2, MISS, 0x0a010001u, 0x0a040101u};
    const uint32_t l2s[5] = {0, 2, 14, 18, 22};
    for (uint32_t n = 1; n <= 256; n += (n < 70 ? 1 : 31)) {
        for (uint32_t k = 0; k < n; k++)
            mk((int)k, 300, (uint16_t)(100 + rnd(8)), l2s[rnd(5)], dsts[rnd(6)], (uint8_t)rnd(256));
        CHECK(cndp_fwd_node_host(t, ptr, n, edge, NULL) == 0);
        for (uint32_t k = 0; k < n; k++)
            CHECK(edge[k] == 1 || ((edge[k] & CNDP_MQ_EDGE_FWD_MASK) >= 2 && (edge[k] & CNDP_MQ_EDGE_FWD_MASK) < 6));
    }

    /* l2_len above data_off: the TTL / checksum edit and the edge, nothing else */
    mk(0, 64, 10, 14, DIRECT, 5);
    mk(1, 64, 0, 1, ROUTED, 5);
    mk(2, 200, 100, 127, DIRECT, 5);
    uint8_t keep[64];
    memcpy(keep, mb[0].buf_addr, 64);
    CHECK(cndp_fwd_node_host(t, ptr, 3, edge, NULL) == 0);
    CHECK(edge[0] == 3 && edge[1] == (4 | G) && edge[2] == 3);
    CHECK(mb[0].data_off == 10 && mb[0].data_len == 46 && mb[1].data_off == 0 && mb[2].data_off == 100);
    keep[18] = 4;
    keep[20] = mb[0].buf_addr[20], keep[21] = mb[0].buf_addr[21];
    CHECK(!memcmp(keep, mb[0].buf_addr, 64));

    /* the frame across buf_len, one byte at a time, for every l2_len: the block ends where the
     * buffer does, so a byte too far is a report */
    for (uint32_t li = 0; li < 5; li++)
        for (uint16_t x = 0; x <= 24; x++)
            for (int w = 1; w <= 4; w += 3) {
                for (int k = 0; k < w; k++)
                    mk(k, (uint16_t)(40 + x), 40, l2s[li], (k & 1) ? ROUTED : DIRECT, 3);
                CHECK(cndp_fwd_node_host(t, ptr, (uint32_t)w, edge, NULL) == 0);
                CHECK(mb[0].data_off == 40 - l2s[li]);
                if (x < 17) /* the destination's first byte unreadable: 0.0.0.0, ARP object 7 */
                    CHECK(edge[0] == 3 + 2);
                if (x >= 20)
                    CHECK(edge[0] == 1 + 2);
            }
    /* data_off at and past buf_len: nothing readable */
    mk(0, 40, 40, 14, DIRECT, 3);
    mk(1, 40, 60, 14, DIRECT, 3);
    CHECK(cndp_fwd_node_host(t, ptr, 2, edge, NULL) == 0 && edge[0] == 5 && edge[1] == 5 && mb[1].data_off == 46);

    /* readable_end: mbufs in one block, the region's end moving through the last one */
    {
        enum { FR = 256, N4 = 4 };
        for (uint32_t cut = 0; cut <= FR; cut += (cut < 64 || cut > 150 ? 1 : 13)) {
            uint8_t *blk = malloc(3 * FR + cut);
            CHECK(blk);
            void *p4[N4];
            for (int k = 0; k < N4; k++) {
                struct mbuf m;
                memset(&m, 0, sizeof(m));
                m.buf_addr = blk + k * FR + 64;
                m.buf_len = FR - 64;
                m.data_off = 100;
                m.data_len = 46;
                m.tx_offload = 14;
                p4[k] = blk + k * FR;
                if (k < 3 || cut >= 64)
                    memcpy(p4[k], &m, 64);
                for (uint32_t j = 64; j < FR && (k < 3 || j < cut); j++)
                    blk[k * FR + j] = (uint8_t)(j == 164 + 16 ? 10 : j == 164 + 17 ? 1 : j == 164 + 19 ? 2 : 0);
            }
            CHECK(cndp_fwd_node_host(t, p4, N4, edge, blk + 3 * FR + cut) == 0);
            CHECK(edge[0] == 3 && edge[1] == 3 && edge[2] == 3);
            CHECK(cut > 164 ? edge[3] != CNDP_FWD_EDGE_NONE : edge[3] == CNDP_FWD_EDGE_NONE);
            free(blk);
        }
    }

    for (int k = 0; k < NMB; k++)
        free(mb[k].buf_addr);
    cndp_fwd_free(t);
    cne_fib_free(arp);
    cne_fib_free(rt4);
    puts("PASS");
    return 0;
}

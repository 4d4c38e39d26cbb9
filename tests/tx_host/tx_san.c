/* tx.c under -fsanitize=address,undefined over the real PCB and forwarding tables
 * and real FIBs: argument checks, the attribute and counter calls at both ends
 * of their ranges, udp_output + ip4_output over buffers whose headers land at
 * every alignment, every headroom around the three prepends, a slab that ends
 * inside the last frame, random table changes with calls between.  Prints PASS
 * and exits 0; any check that fails exits 1, a sanitizer report aborts. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cndp_amd/csrc/tx_internal.h"

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

static uint32_t be(uint32_t host) { return __builtin_bswap32(host); }

/* one's complement sum of [p, p + n) as big-endian words, folded */
static uint32_t csum(const uint8_t *p, uint32_t n, uint32_t s)
{
    for (uint32_t k = 0; k + 1 < n; k += 2)
        s += (uint32_t)p[k] << 8 | p[k + 1];
    if (n & 1u)
        s += (uint32_t)p[n - 1] << 8;
    while (s >> 16)
        s = (s >> 16) + (s & 0xffffu);
    return s;
}

enum { ARP_N = 16, RT_N = 8, N = 64, SLOT = 2048 };

int main(void)
{
    struct cne_fib *arp = mkfib("arp-fib", ARP_N + 1), *rt4 = mkfib("rt4-fib", RT_N + 1);
    CHECK(arp && rt4);
    cndp_fwd_tbl_t *ft = NULL;
    cndp_pcb_tbl_t *pt = NULL;
    CHECK(cndp_fwd_create(arp, rt4, ARP_N, RT_N, &ft) == 0 && cndp_pcb_create(8, &pt) == 0);

    /* attributes: defaults, both ends, a deleted entry, one added after a look */
    struct cndp_pcb_entry e = {.laddr = be(0x0a020007u), .lport = 0x8813, .opt_flag = CNDP_UDP_CHKSUM_FLAG};
    struct cndp_pcb_tx a = {0, 0, 0};
    CHECK(cndp_pcb_tx_get(pt, 0, &a) == -EINVAL && cndp_pcb_tx_set(pt, 0, &a) == -EINVAL);
    CHECK(cndp_pcb_add(pt, &e) == 0);
    CHECK(cndp_pcb_tx_get(pt, 0, &a) == 0 && a.tos == 0 && a.ttl == 64 && a.ip_proto == 17);
    CHECK(cndp_pcb_tx_get(NULL, 0, &a) == -EINVAL && cndp_pcb_tx_get(pt, 0, NULL) == -EINVAL);
    CHECK(cndp_pcb_tx_set(NULL, 0, &a) == -EINVAL && cndp_pcb_tx_set(pt, 0, NULL) == -EINVAL);
    e.opt_flag = 0;
    e.laddr = be(0x0a030007u);
    for (int k = 1; k < 8; k++)
        CHECK(cndp_pcb_add(pt, &e) == k);
    a.tos = 0xff, a.ttl = 1, a.ip_proto = 6;
    CHECK(cndp_pcb_tx_set(pt, 7, &a) == 0 && cndp_pcb_tx_set(pt, 8, &a) == -EINVAL);
    a.ip_proto = 1;
    CHECK(cndp_pcb_tx_set(pt, 6, &a) == 0);
    CHECK(cndp_pcb_tx_get(pt, 7, &a) == 0 && a.tos == 0xff && a.ttl == 1 && a.ip_proto == 6);
    CHECK(cndp_pcb_del(pt, 5) == 0 && cndp_pcb_tx_get(pt, 5, &a) == -ENOENT && cndp_pcb_tx_set(pt, 5, &a) == -ENOENT);

    /* counters */
    uint16_t id = 1;
    CHECK(cndp_fwd_netif_ident_get(ft, 0, &id) == 0 && id == 0);
    CHECK(cndp_fwd_netif_ident_get(ft, 255, &id) == 0 && id == 0);
    CHECK(cndp_fwd_netif_ident_get(ft, 256, &id) == -EINVAL && cndp_fwd_netif_ident_get(ft, 0, NULL) == -EINVAL);
    CHECK(cndp_fwd_netif_ident_set(ft, 256, 1) == -EINVAL && cndp_fwd_netif_ident_set(NULL, 0, 1) == -EINVAL);
    CHECK(cndp_fwd_netif_ident_set(ft, 255, 0xfff0) == 0 && cndp_fwd_netif_ident_set(ft, 2, 0xfff0) == 0);

    /* 10.2/16 -> route 1 on netif 2, 10.3/16 -> route 2 on netif 255; 10.1.0.1 has an ARP entry */
    const uint8_t mac2[6] = {2, 0x11, 0x22, 0x33, 0x44, 2};
    struct cndp_fwd_arp ae = {.netif_idx = 0, .ha = {2, 0xaa, 0, 0, 0, 1}};
    struct cndp_fwd_rt r1 = {.gateway = 0, .netif_idx = 2}, r2 = {.gateway = 0, .netif_idx = 255};
    CHECK(cndp_fwd_netif_set(ft, 2, mac2) == 0 && cndp_fwd_arp_set(ft, 1, &ae) == 0);
    CHECK(cndp_fwd_rt_set(ft, 1, &r1) == 0 && cndp_fwd_rt_set(ft, 2, &r2) == 0);
    CHECK(cne_fib_add(arp, 0x0a010001u, 32, 1) == 0);
    CHECK(cne_fib_add(rt4, 0x0a020000u, 16, 1) == 0 && cne_fib_add(rt4, 0x0a030000u, 16, 2) == 0);

    static uint32_t pcb[N], faddr[N], laddr[N], ports[N];
    static uint16_t len[N], edge[N], bin[N];
    static uint64_t offs[N];
    uint64_t stats[CNDP_TX_NSTATS] = {0};
    struct cndp_tx_io io = {.pcb = pcb, .faddr = faddr, .laddr = laddr, .ports = ports, .len = len, .tx_edge = edge,
                            .bin_of = bin, .n_bins = 256, .stats = stats};
    /* argument checks */
    uint8_t *slab = malloc((size_t)N * SLOT);
    CHECK(slab);
    CHECK(cndp_tx_output_host(NULL, pt, 0, slab, SLOT, SLOT, NULL, 64, 1, &io) == -EINVAL);
    CHECK(cndp_tx_output_host(ft, NULL, 0, slab, SLOT, SLOT, NULL, 64, 1, &io) == -EINVAL);
    CHECK(cndp_tx_output_host(ft, pt, 2, slab, SLOT, SLOT, NULL, 64, 1, &io) == -EINVAL);
    CHECK(cndp_tx_output_host(ft, pt, 0, NULL, SLOT, SLOT, NULL, 64, 1, &io) == -EINVAL);
    CHECK(cndp_tx_output_host(ft, pt, 0, slab, SLOT, SLOT, NULL, 64, 1, NULL) == -EINVAL);
    CHECK(cndp_tx_output_host(ft, pt, 0, NULL, 0, 0, NULL, 0, 0, &io) == 0);
    io.n_bins = 255; /* the table's largest netif */
    CHECK(cndp_tx_output_host(ft, pt, 0, slab, SLOT, SLOT, NULL, 64, 1, &io) == -EINVAL);
    io.n_bins = 256;
    io.ports = NULL;
    CHECK(cndp_tx_output_host(ft, pt, CNDP_TX_UDP, slab, SLOT, SLOT, NULL, 64, 1, &io) == -EINVAL);
    CHECK(cndp_tx_output_host(ft, pt, CNDP_TX_IP4, slab, SLOT, SLOT, NULL, 64, 1, &io) == 0);
    io.ports = ports;

    /* every headroom, both modes, offsets that put the headers at every
     * alignment, an exactly sized slab that ends inside the last payload */
    static const uint32_t heads[] = {0, 7, 8, 19, 20, 27, 28, 33, 34, 41, 42, 43, 45, 64, 256};
    for (unsigned hk = 0; hk < sizeof(heads) / sizeof(heads[0]); hk++)
        for (uint32_t mode = 0; mode < 2; mode++)
            for (uint32_t cut = 0; cut < 3; cut++) {
                const uint32_t h = heads[hk];
                uint64_t at = 0;
                for (int i = 0; i < N; i++) {
                    pcb[i] = i % 10 == 9 ? CNDP_PCB_NONE : (uint32_t)(i % 9); /* 8: outside the vector; 5: deleted */
                    faddr[i] = be(i & 1 ? 0x0a010001u : 0xc0000201u);
                    laddr[i] = be(i % 4 == 3 ? 0x0a090001u : i % 4 == 2 ? 0x0a030007u : 0x0a020007u);
                    ports[i] = rnd(1u << 16) | rnd(1u << 16) << 16;
                    len[i] = (uint16_t)(i < 6 ? (uint32_t)i : rnd(1400));
                    offs[i] = at;
                    at += h + len[i] + rnd(5);
                }
                uint64_t slab_len = cut == 0 ? at : offs[N - 1] + h + (cut == 1 ? 0 : len[N - 1] / 2);
                uint8_t *sl = malloc(slab_len ? slab_len : 1); /* exactly sized: a byte past it is a report */
                CHECK(sl);
                memset(sl, 0x5a, slab_len);
                const uint64_t sent0 = stats[CNDP_TX_STAT_SENT];
                CHECK(cndp_tx_output_host(ft, pt, mode, sl, slab_len, 0, offs, h, N, &io) == 0);
                const uint32_t need = mode == CNDP_TX_UDP ? 42u : 34u;
                CHECK((stats[CNDP_TX_STAT_SENT] > sent0) == (h >= need));
                for (int i = 0; i < N; i++) {
                    const int live = pcb[i] < 8 && pcb[i] != 5;
                    CHECK(live ? edge[i] != CNDP_TX_EDGE_NONE : edge[i] == CNDP_TX_EDGE_NONE);
                    CHECK(edge[i] <= 1 || edge[i] == 2 + 2 || edge[i] == 255 + 2 || edge[i] == CNDP_TX_EDGE_NONE);
                    CHECK(bin[i] == (edge[i] >= 2 && edge[i] != CNDP_TX_EDGE_NONE ? edge[i] - 2 : edge[i] == 1 ? 256 : 257));
                    /* a sent UDP datagram that lies inside the slab verifies: header and, with the flag, payload */
                    if (mode == CNDP_TX_UDP && edge[i] >= 2 && edge[i] != CNDP_TX_EDGE_NONE &&
                        offs[i] + h + len[i] <= slab_len) {
                        const uint8_t *ip = sl + offs[i] + h - 28;
                        CHECK(csum(ip, 20, 0) == 0xffff);
                        if (pcb[i] == 0) {
                            uint8_t ps[12];
                            memcpy(ps, ip + 12, 8);
                            ps[8] = 0, ps[9] = 17, ps[10] = ip[24], ps[11] = ip[25];
                            CHECK(csum(ip + 20, 8u + len[i], csum(ps, 12, 0)) == 0xffff);
                        }
                    }
                }
                free(sl);
            }
    CHECK(stats[CNDP_TX_STAT_SENT] && stats[CNDP_TX_STAT_ARP_REQUEST] && stats[CNDP_TX_STAT_DROP_HEADROOM] &&
          stats[CNDP_TX_STAT_DROP_NOROUTE] && stats[CNDP_TX_STAT_DROP_PROTO] && stats[CNDP_TX_STAT_CKSUM]);
    CHECK(cndp_fwd_netif_ident_get(ft, 2, &id) == 0 && id != 0xfff0);

    /* random table changes, calls between */
    for (int it = 0; it < 600; it++) {
        uint32_t k = rnd(6);
        int rc = 0;
        a.tos = (uint8_t)rnd(256), a.ttl = (uint8_t)rnd(256), a.ip_proto = rnd(3) == 0 ? 6 : 17;
        r1.netif_idx = (uint16_t)rnd(4);
        if (k == 0)
            rc = cndp_pcb_tx_set(pt, rnd(8), &a);
        else if (k == 1)
            rc = cndp_fwd_rt_set(ft, rnd(RT_N), &r1);
        else if (k == 2)
            rc = cndp_fwd_rt_clear(ft, rnd(RT_N));
        else if (k == 3)
            rc = cndp_fwd_netif_ident_set(ft, rnd(4), (uint16_t)rnd(65536));
        else if (k == 4)
            rc = cne_fib_add(rt4, 0x0a020000u + (rnd(4) << 8), 24, rnd(RT_N + 2));
        else {
            for (int i = 0; i < 8; i++)
                pcb[i] = rnd(10), laddr[i] = be(0x0a020000u + (rnd(4) << 8) + 7), len[i] = (uint16_t)rnd(64), offs[i] = 128u * i;
            rc = cndp_tx_output_host(ft, pt, rnd(2), slab, 8 * 128, 0, offs, 42 + rnd(8), 8, &io);
        }
        CHECK(rc == 0 || rc == -ENOENT);
    }
    free(slab);
    cndp_pcb_free(pt);
    cndp_fwd_free(ft);
    cndp_pcb_free(NULL);
    cne_fib_free(arp);
    cne_fib_free(rt4);
    puts("PASS");
    return 0;
}

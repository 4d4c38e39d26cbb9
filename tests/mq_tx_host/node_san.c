/* cndp_ip4_output_node_host (tx.c) under -fsanitize=address,undefined over the
 * real PCB and forwarding tables and real FIBs: argument checks, both modes over
 * mbufs whose headers, metadata and buffers are exactly sized allocations (a
 * byte in front of or behind one is a report), every headroom around the three
 * prepends, every payload length and alignment of mtod, readable_end and
 * stage_max clips, a metadata hook that answers NULL, userptr values that name
 * no PCB, counters that wrap.  Prints PASS and exits 0; any check that fails
 * exits 1, a sanitizer report aborts. */
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

static uint32_t rnd_state = 4242;
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

enum { ARP_N = 16, RT_N = 8, N = 64 };

/* an mbuf as three exactly sized allocations: header + default metadata (104 bytes), buffer */
struct mb {
    uint8_t *m, *buf;
    uint16_t H, blen, dlen;
};

static void mb_make(struct mb *b, uint16_t H, uint16_t blen, uint16_t dlen, uint64_t userptr, uint32_t faddr,
                    uint32_t laddr)
{
    b->m = aligned_alloc(64, 128); /* 104 used; the allocator rounds: the checks below cover the rest */
    b->buf = malloc(blen ? blen : 1);
    CHECK(b->m && b->buf);
    memset(b->m, 0, 128);
    memset(b->buf, 0x5a, blen);
    for (uint32_t k = H; k < blen && k < (uint32_t)H + dlen; k++)
        b->buf[k] = (uint8_t)rnd(256);
    b->H = H, b->blen = blen, b->dlen = dlen;
    const uint64_t ba = (uint64_t)(uintptr_t)b->buf, txo = 0x5aull << 24 | 8u << 16 | 20u << 7 | 14u;
    const uint16_t fport = (uint16_t)rnd(65536), lport = 0x8813;
    memcpy(b->m + PCB_MB_BUF_ADDR, &ba, 8);
    memcpy(b->m + PCB_MB_DATA_OFF, &H, 2);
    memcpy(b->m + PCB_MB_BUF_LEN, &blen, 2);
    memcpy(b->m + PCB_MB_DATA_LEN, &dlen, 2);
    memcpy(b->m + PCB_MB_TX_OFFLOAD, &txo, 8);
    memcpy(b->m + PCB_MB_USERPTR, &userptr, 8);
    memcpy(b->m + 64 + 2, &fport, 2);
    memcpy(b->m + 64 + 4, &faddr, 4);
    memcpy(b->m + 64 + PCB_MD_LADDR + 2, &lport, 2);
    memcpy(b->m + 64 + PCB_MD_LADDR + 4, &laddr, 4);
}

static void mb_free(struct mb *b)
{
    free(b->m);
    free(b->buf);
}

static uint16_t mb_u16(const struct mb *b, int o)
{
    uint16_t v;
    memcpy(&v, b->m + o, 2);
    return v;
}

static void *md_null_odd(const void *m)
{
    uint16_t dl;
    memcpy(&dl, (const uint8_t *)m + PCB_MB_DATA_LEN, 2);
    return (dl & 1u) ? NULL : (void *)((uintptr_t)m + 64);
}

int main(void)
{
    struct cne_fib *arp = mkfib("arp-fib", ARP_N + 1), *rt4 = mkfib("rt4-fib", RT_N + 1);
    CHECK(arp && rt4);
    cndp_fwd_tbl_t *ft = NULL;
    cndp_pcb_tbl_t *pt = NULL;
    CHECK(cndp_fwd_create(arp, rt4, ARP_N, RT_N, &ft) == 0 && cndp_pcb_create(8, &pt) == 0);
    /* PCB 0: UDP with the checksum flag; 1-4 without; 5 deleted; 6 protocol 1; 7 TCP */
    struct cndp_pcb_entry e = {.laddr = be(0x0a020007u), .lport = 0x8813, .opt_flag = CNDP_UDP_CHKSUM_FLAG};
    CHECK(cndp_pcb_add(pt, &e) == 0);
    e.opt_flag = 0;
    for (int k = 1; k < 8; k++)
        CHECK(cndp_pcb_add(pt, &e) == k);
    struct cndp_pcb_tx a = {.tos = 0xff, .ttl = 1, .ip_proto = 6};
    CHECK(cndp_pcb_tx_set(pt, 7, &a) == 0);
    a.ip_proto = 1;
    CHECK(cndp_pcb_tx_set(pt, 6, &a) == 0 && cndp_pcb_del(pt, 5) == 0);
    /* 10.2/16 -> route 1 on netif 2, 10.3/16 -> route 2 on netif 255; 10.1.0.1 has an ARP entry */
    const uint8_t mac2[6] = {2, 0x11, 0x22, 0x33, 0x44, 2};
    struct cndp_fwd_arp ae = {.netif_idx = 0, .ha = {2, 0xaa, 0, 0, 0, 1}};
    struct cndp_fwd_rt r1 = {.gateway = 0, .netif_idx = 2}, r2 = {.gateway = 0, .netif_idx = 255};
    CHECK(cndp_fwd_netif_set(ft, 2, mac2) == 0 && cndp_fwd_arp_set(ft, 1, &ae) == 0);
    CHECK(cndp_fwd_rt_set(ft, 1, &r1) == 0 && cndp_fwd_rt_set(ft, 2, &r2) == 0);
    CHECK(cne_fib_add(arp, 0x0a010001u, 32, 1) == 0);
    CHECK(cne_fib_add(rt4, 0x0a020000u, 16, 1) == 0 && cne_fib_add(rt4, 0x0a030000u, 16, 2) == 0);
    CHECK(cndp_fwd_netif_ident_set(ft, 2, 0xfff0) == 0 && cndp_fwd_netif_ident_set(ft, 255, 0xfff0) == 0);

    static struct mb mb[N];
    static void *ptr[257];
    static uint16_t edge[257];
    /* argument checks */
    mb_make(&mb[0], 64, 256, 18, 0, be(0x0a010001u), be(0x0a020007u));
    ptr[0] = mb[0].m;
    CHECK(cndp_ip4_output_node_host(NULL, pt, 0, ptr, 1, edge, NULL, 0, NULL) == -EINVAL);
    CHECK(cndp_ip4_output_node_host(ft, NULL, 0, ptr, 1, edge, NULL, 0, NULL) == -EINVAL);
    CHECK(cndp_ip4_output_node_host(ft, pt, 2, ptr, 1, edge, NULL, 0, NULL) == -EINVAL);
    CHECK(cndp_ip4_output_node_host(ft, pt, 0, NULL, 1, edge, NULL, 0, NULL) == -EINVAL);
    CHECK(cndp_ip4_output_node_host(ft, pt, 0, ptr, 1, NULL, NULL, 0, NULL) == -EINVAL);
    CHECK(cndp_ip4_output_node_host(ft, pt, 0, ptr, 257, edge, NULL, 0, NULL) == -EINVAL);
    CHECK(cndp_ip4_output_node_host(ft, pt, 0, NULL, 0, NULL, NULL, 0, NULL) == 0);
    CHECK(mb_u16(&mb[0], PCB_MB_DATA_OFF) == 64 && mb_u16(&mb[0], PCB_MB_DATA_LEN) == 18); /* a refused call touches nothing */
    mb_free(&mb[0]);

    /* every headroom around the prepends, both modes, every alignment of mtod (the buffer's own
     * alignment moves with its size), payloads of every small length and a few large ones; the buffer
     * ends exactly behind the payload, or (cut) inside it */
    static const uint16_t heads[] = {0, 7, 8, 19, 20, 27, 28, 33, 34, 41, 42, 43, 45, 50, 64, 207};
    uint64_t seen[8] = {0};
    for (unsigned hk = 0; hk < sizeof(heads) / sizeof(heads[0]); hk++)
        for (uint32_t mode = 0; mode < 2; mode++)
            for (uint32_t cut = 0; cut < 2; cut++) {
                const uint16_t H = heads[hk];
                for (int i = 0; i < N; i++) {
                    const uint16_t len = (uint16_t)(i < 24 ? (uint32_t)i : i < 60 ? rnd(1473) : 1472u);
                    const uint64_t up = i % 10 == 9 ? (1ull << 32) | 1u : (uint64_t)(i % 9); /* 8: outside the vector; 5: deleted */
                    mb_make(&mb[i], H, (uint16_t)(H + (cut ? len / 2 : len)), len, up,
                            be(i & 1 ? 0x0a010001u : 0xc0000201u),
                            be(i % 4 == 3 ? 0x0a090001u : i % 4 == 2 ? 0x0a030007u : 0x0a020007u));
                    ptr[i] = mb[i].m;
                }
                CHECK(cndp_ip4_output_node_host(ft, pt, mode, ptr, N, edge, NULL, 0, NULL) == 0);
                const uint32_t need = TX_IMG_END(mode);
                for (int i = 0; i < N; i++) {
                    const uint32_t pi = (uint32_t)(i % 9);
                    const int live = i % 10 != 9 && pi < 8 && pi != 5;
                    CHECK(live == (edge[i] != CNDP_TX_EDGE_NONE));
                    const uint16_t doff = mb_u16(&mb[i], PCB_MB_DATA_OFF), dlen = mb_u16(&mb[i], PCB_MB_DATA_LEN);
                    if (!live) {
                        CHECK(doff == H && dlen == mb[i].dlen);
                        mb_free(&mb[i]);
                        continue;
                    }
                    const uint32_t own = edge[i] & CNDP_MQ_EDGE_TX_MASK, cause = CNDP_MQ_EDGE_TX_CAUSE(edge[i]);
                    CHECK(own <= 1 || own == 2 + 2 || own == 255 + 2);
                    CHECK((own == 0) == (cause != 0) && (uint32_t)(H - doff) == (uint32_t)(dlen - mb[i].dlen));
                    seen[own >= 2 ? 0 : own == 1 ? 5 : cause]++;
                    if (edge[i] & CNDP_MQ_EDGE_TX_CKSUM)
                        seen[6]++;
                    if (own) {
                        CHECK(H >= need && doff == H - need);
                        const uint8_t *ip = mb[i].buf + doff + 14;
                        CHECK(csum(ip, 20, 0) == 0xffff);
                        /* an uncut UDP datagram of PCB 0 verifies */
                        if (mode == CNDP_TX_UDP && pi == 0 && !cut) {
                            uint8_t ps[12];
                            memcpy(ps, ip + 12, 8);
                            ps[8] = 0, ps[9] = 17, ps[10] = ip[24], ps[11] = ip[25];
                            CHECK((edge[i] & CNDP_MQ_EDGE_TX_CKSUM) && csum(ip + 20, 8u + mb[i].dlen, csum(ps, 12, 0)) == 0xffff);
                        }
                    } else
                        CHECK(cause == CNDP_MQ_TX_CAUSE_HEADROOM ? H < need
                                                                 : cause == CNDP_MQ_TX_CAUSE_NOROUTE ? i % 4 == 3 : pi == 6);
                    mb_free(&mb[i]);
                }
            }
    CHECK(seen[0] && seen[5] && seen[CNDP_MQ_TX_CAUSE_HEADROOM] && seen[CNDP_MQ_TX_CAUSE_NOROUTE] &&
          seen[CNDP_MQ_TX_CAUSE_PROTO] && seen[6]);
    uint16_t id = 0xfff0;
    CHECK(cndp_fwd_netif_ident_get(ft, 2, &id) == 0 && id != 0xfff0);

    /* the metadata hook answers NULL for odd lengths: NOMD, nothing written */
    for (int i = 0; i < N; i++) {
        mb_make(&mb[i], 64, (uint16_t)(64 + i), (uint16_t)i, 0, be(0x0a010001u), be(0x0a020007u));
        ptr[i] = mb[i].m;
    }
    CHECK(cndp_ip4_output_node_host(ft, pt, CNDP_TX_UDP, ptr, N, edge, NULL, 0, md_null_odd) == 0);
    for (int i = 0; i < N; i++) {
        if (i & 1)
            CHECK(edge[i] == CNDP_MQ_TX_CAUSE_NOMD << 9 && mb_u16(&mb[i], PCB_MB_DATA_OFF) == 64 && mb[i].buf[63] == 0x5a);
        else
            CHECK((edge[i] & CNDP_MQ_EDGE_TX_MASK) == 4 && mb_u16(&mb[i], PCB_MB_DATA_OFF) == 22);
        mb_free(&mb[i]);
    }

    /* clips: stage_max shorter than the payload, and a region that ends inside the last payload:
     * mbufs in one arena, headers in front, the buffers behind them */
    {
        enum { K = 8, BL = 512 };
        uint8_t *arena = aligned_alloc(64, K * 128 + K * BL);
        CHECK(arena);
        for (uint32_t pass = 0; pass < 3; pass++) {
            memset(arena, 0, K * 128 + K * BL);
            for (int i = 0; i < K; i++) {
                uint8_t *m = arena + 128 * i, *buf = arena + K * 128 + BL * i;
                const uint64_t ba = (uint64_t)(uintptr_t)buf, up = 0;
                const uint16_t H = 100, blen = BL, dlen = 412, lport = 0x8813;
                const uint32_t fa = be(0x0a010001u), la = be(0x0a020007u);
                for (int k = 0; k < 412; k++)
                    buf[H + k] = (uint8_t)rnd(256);
                memcpy(m + PCB_MB_BUF_ADDR, &ba, 8);
                memcpy(m + PCB_MB_DATA_OFF, &H, 2);
                memcpy(m + PCB_MB_BUF_LEN, &blen, 2);
                memcpy(m + PCB_MB_DATA_LEN, &dlen, 2);
                memcpy(m + PCB_MB_USERPTR, &up, 8);
                memcpy(m + 64 + 4, &fa, 4);
                memcpy(m + 64 + PCB_MD_LADDR + 2, &lport, 2);
                memcpy(m + 64 + PCB_MD_LADDR + 4, &la, 4);
                ptr[i] = m;
            }
            ptr[K] = NULL; /* a NULL entry is not taken */
            const uint8_t *end = pass == 1 ? arena + K * 128 + K * BL - 200 : NULL;
            CHECK(cndp_ip4_output_node_host(ft, pt, CNDP_TX_UDP, ptr, K + 1, edge, end, pass == 2 ? 64 : 0, NULL) == 0);
            CHECK(edge[K] == CNDP_TX_EDGE_NONE);
            for (int i = 0; i < K; i++) {
                const uint8_t *ip = arena + K * 128 + BL * i + 100 - 28;
                uint8_t ps[12];
                memcpy(ps, ip + 12, 8);
                ps[8] = 0, ps[9] = 17, ps[10] = ip[24], ps[11] = ip[25];
                const int whole = pass == 0 || (pass == 1 && i < K - 1);
                CHECK((edge[i] & CNDP_MQ_EDGE_TX_MASK) == 4 && (edge[i] & CNDP_MQ_EDGE_TX_CKSUM));
                CHECK((csum(ip + 20, 8u + 412u, csum(ps, 12, 0)) == 0xffff) == whole);
            }
        }
        free(arena);
    }
    cndp_pcb_free(pt);
    cndp_fwd_free(ft);
    cne_fib_free(arp);
    cne_fib_free(rt4);
    printf("PASS\n");
    return 0;
}

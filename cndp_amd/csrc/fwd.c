/*
 * fwd.c -- the forwarding table of include/cndp_fwd.h: what ip4_forward reads of
 * this_cnet (the ARP and route FIBs, the object arrays fib_info_lookup indexes,
 * the netif MACs), the node's 1-wide rule on the host (ip4_forward.c:271-318),
 * the whole node over one burst of mbufs (cndp_fwd_node_host, cndp_mqcnet.h)
 * and the object image the device stage mirrors.  Plain C, no HIP: it also
 * builds into stand-alone programs (tests/fwd_host, tests/mq_ip4fwd_host).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/cndp_mqcnet.h"
#include "fwd_internal.h"

static int fib_ok(const struct cne_fib *f)
{
    return f && f->type == CNE_FIB_DIR24_8 && !f->t.is_trie && f->t.nh_sz == CNE_FIB_DIR24_8_4B && f->t.tbl24 &&
           f->t.tbl8;
}

int cndp_fwd_create(struct cne_fib *arp_fib, struct cne_fib *rt4_fib, uint32_t arp_objs, uint32_t rt_objs,
                    cndp_fwd_tbl_t **out)
{
    if (!out || !fib_ok(arp_fib) || !fib_ok(rt4_fib) || arp_objs == 0 || arp_objs > CNDP_FWD_OBJS_MAX ||
        rt_objs == 0 || rt_objs > CNDP_FWD_OBJS_MAX)
        return -EINVAL;
    struct cndp_fwd_tbl *t = calloc(1, sizeof(*t));
    if (!t)
        return -ENOMEM;
    t->img_words = FWD_IMG_WORDS(arp_objs, rt_objs);
    t->img = calloc(t->img_words, sizeof(uint32_t));
    if (!t->img || pthread_mutex_init(&t->lock, NULL)) {
        free(t->img);
        free(t);
        return -ENOMEM;
    }
    t->arp_fib = arp_fib;
    t->rt4_fib = rt4_fib;
    t->arp_cap = arp_objs;
    t->rt_cap = rt_objs;
    t->img[0] = arp_objs;
    t->img[1] = rt_objs;
    t->img[2] = (uint32_t)t->img_words; /* < 2^27 */
    t->gen = 1;
    t->d_lo = 0;
    t->d_hi = t->img_words;
    *out = t;
    return 0;
}

void cndp_fwd_free(cndp_fwd_tbl_t *t)
{
    if (!t)
        return;
    if (t->dev && t->dev_release)
        t->dev_release(t->dev);
    if (t->xdev && t->xdev_release)
        t->xdev_release(t->xdev);
    pthread_mutex_destroy(&t->lock);
    free(t->img);
    free(t);
}

/* call with the lock held: words [at, at + 2) of the image changed */
static void touched(struct cndp_fwd_tbl *t, const uint32_t *at)
{
    size_t lo = (size_t)(at - t->img);
    if (lo < t->d_lo)
        t->d_lo = lo;
    if (lo + 2 > t->d_hi)
        t->d_hi = lo + 2;
    t->gen++;
}

int cndp_fwd_arp_set(cndp_fwd_tbl_t *t, uint32_t idx, const struct cndp_fwd_arp *e)
{
    if (!t || !e || idx >= t->arp_cap || e->netif_idx >= CNDP_FWD_NETIFS)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    uint32_t *w = fwd_arp(t) + 2u * (size_t)idx;
    if (w[0] & FWD_SET)
        t->nif_refs[(w[0] >> 16) & 0xffu]--;
    t->nif_refs[e->netif_idx]++;
    w[0] = FWD_SET | (uint32_t)e->netif_idx << 16 | e->ha[0] | (uint32_t)e->ha[1] << 8;
    w[1] = e->ha[2] | (uint32_t)e->ha[3] << 8 | (uint32_t)e->ha[4] << 16 | (uint32_t)e->ha[5] << 24;
    touched(t, w);
    pthread_mutex_unlock(&t->lock);
    return 0;
}

int cndp_fwd_arp_clear(cndp_fwd_tbl_t *t, uint32_t idx)
{
    if (!t || idx >= t->arp_cap)
        return -EINVAL;
    int r = 0;
    pthread_mutex_lock(&t->lock);
    uint32_t *w = fwd_arp(t) + 2u * (size_t)idx;
    if (!(w[0] & FWD_SET))
        r = -ENOENT;
    else {
        t->nif_refs[(w[0] >> 16) & 0xffu]--;
        w[0] = w[1] = 0;
        touched(t, w);
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_fwd_rt_set(cndp_fwd_tbl_t *t, uint32_t idx, const struct cndp_fwd_rt *e)
{
    if (!t || !e || idx >= t->rt_cap || e->netif_idx >= CNDP_FWD_NETIFS)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    uint32_t *w = fwd_rt(t) + 2u * (size_t)idx;
    if (w[1] & FWD_SET)
        t->nif_refs[w[1] & 0xffu]--;
    t->nif_refs[e->netif_idx]++;
    w[0] = e->gateway;
    w[1] = FWD_SET | e->netif_idx;
    touched(t, w);
    pthread_mutex_unlock(&t->lock);
    return 0;
}

int cndp_fwd_rt_clear(cndp_fwd_tbl_t *t, uint32_t idx)
{
    if (!t || idx >= t->rt_cap)
        return -EINVAL;
    int r = 0;
    pthread_mutex_lock(&t->lock);
    uint32_t *w = fwd_rt(t) + 2u * (size_t)idx;
    if (!(w[1] & FWD_SET))
        r = -ENOENT;
    else {
        t->nif_refs[w[1] & 0xffu]--;
        w[0] = w[1] = 0;
        touched(t, w);
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_fwd_netif_set(cndp_fwd_tbl_t *t, uint32_t idx, const uint8_t *mac)
{
    static const uint8_t zero[6];
    if (!t || idx >= CNDP_FWD_NETIFS)
        return -EINVAL;
    if (!mac)
        mac = zero;
    pthread_mutex_lock(&t->lock);
    uint32_t *w = fwd_netif(t) + 2u * (size_t)idx;
    w[0] = mac[0] | (uint32_t)mac[1] << 8 | (uint32_t)mac[2] << 16 | (uint32_t)mac[3] << 24;
    w[1] = mac[4] | (uint32_t)mac[5] << 8;
    touched(t, w);
    pthread_mutex_unlock(&t->lock);
    return 0;
}

int fwd_max_netif(const struct cndp_fwd_tbl *t)
{
    for (int k = (int)CNDP_FWD_NETIFS - 1; k >= 0; k--)
        if (t->nif_refs[k])
            return k;
    return -1;
}

int cndp_fwd_max_netif(cndp_fwd_tbl_t *t)
{
    if (!t)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = fwd_max_netif(t);
    pthread_mutex_unlock(&t->lock);
    return r;
}

/* cne_fib_lookup_bulk on the host image, DIR-24-8 4B (dir24_8.h:131-135) */
static uint32_t lpm4(const struct cne_fib *f, uint32_t ip)
{
    uint32_t e = ((const uint32_t *)f->t.tbl24)[ip >> 8];
    if (e & 1u)
        e = ((const uint32_t *)f->t.tbl8)[(size_t)(e >> 1) * CNDP_TBL8_GRP + (ip & 0xffu)];
    return e >> 1;
}

/* fib_info_lookup for one key: the object's two image words, or NULL */
static const uint32_t *arp_obj(const struct cndp_fwd_tbl *t, uint32_t key)
{
    uint32_t idx = lpm4(t->arp_fib, key) & 0xffffffu;
    if (idx >= t->arp_cap)
        return NULL;
    const uint32_t *w = fwd_arp(t) + 2u * (size_t)idx;
    return (w[0] & FWD_SET) ? w : NULL;
}

static const uint32_t *rt_obj(const struct cndp_fwd_tbl *t, uint32_t key)
{
    uint32_t idx = lpm4(t->rt4_fib, key) & 0xffffffu;
    if (idx >= t->rt_cap)
        return NULL;
    const uint32_t *w = fwd_rt(t) + 2u * (size_t)idx;
    return (w[1] & FWD_SET) ? w : NULL;
}

static void fill(const struct cndp_fwd_tbl *t, struct cndp_fwd_result *o, uint32_t netif, const uint32_t *arp)
{
    const uint32_t *m = fwd_netif(t) + 2u * (size_t)netif;
    o->edge = (uint16_t)(netif + CNDP_FWD_EDGE_OUTPUT);
    for (int k = 0; k < 4; k++)
        o->s_addr[k] = (uint8_t)(m[0] >> (8 * k));
    o->s_addr[4] = (uint8_t)m[1];
    o->s_addr[5] = (uint8_t)(m[1] >> 8);
    o->d_addr[0] = (uint8_t)arp[0];
    o->d_addr[1] = (uint8_t)(arp[0] >> 8);
    for (int k = 0; k < 4; k++)
        o->d_addr[2 + k] = (uint8_t)(arp[1] >> (8 * k));
}

int cndp_fwd_lookup(cndp_fwd_tbl_t *t, const uint32_t *dst_be, uint32_t n, struct cndp_fwd_result *out)
{
    if (!t || (n && (!dst_be || !out)))
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    /* the FIBs' host images are painted under their own locks (taken in
     * address order: two tables may hold the same FIBs the other way round) */
    struct cne_fib *f0 = t->arp_fib < t->rt4_fib ? t->arp_fib : t->rt4_fib;
    struct cne_fib *f1 = t->arp_fib < t->rt4_fib ? t->rt4_fib : t->arp_fib;
    pthread_mutex_lock(&f0->t.dev_lock);
    if (f1 != f0)
        pthread_mutex_lock(&f1->t.dev_lock);
    for (uint32_t k = 0; k < n; k++) {
        struct cndp_fwd_result *o = &out[k];
        memset(o, 0, sizeof(*o));
        o->edge = CNDP_FWD_EDGE_ARP_REQUEST;
        const uint32_t key = __builtin_bswap32(dst_be[k]); /* be32toh(hdr->dst_addr) */
        const uint32_t *a = arp_obj(t, key);
        if (a)
            fill(t, o, (a[0] >> 16) & 0xffu, a);
        else {
            const uint32_t *r = rt_obj(t, key);
            if (r && (a = arp_obj(t, r[0])) != NULL) /* the gateway's s_addr as it is stored */
                fill(t, o, r[1] & 0xffu, a);
        }
    }
    if (f1 != f0)
        pthread_mutex_unlock(&f1->t.dev_lock);
    pthread_mutex_unlock(&f0->t.dev_lock);
    pthread_mutex_unlock(&t->lock);
    return 0;
}

/* ---- the node over mbufs on the calling thread (include/cndp_mqcnet.h) ---- */
/* pktmbuf_t fields (pktmbuf.h:102-204) */
#define NB_BUF_ADDR 8
#define NB_DATA_OFF 24
#define NB_BUF_LEN 28
#define NB_DATA_LEN 30
#define NB_TX_OFFLOAD 40

_Static_assert(FWD_EDGE_GATEWAY == CNDP_MQ_EDGE_FWD_GATEWAY, "the rule's gateway bit is the header's");

static inline uint16_t ld16(const uint8_t *p)
{
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
}

/* one member of a group between the node's head (:112-115) and its MAC writes */
struct node_mb {
    uint8_t *m;      /* NULL: not taken */
    uintptr_t f;     /* pktmbuf_mtod at entry: the IPv4 header */
    uintptr_t lim;   /* the first address that is not readable */
    uint32_t l2, adj; /* l2_len; pktmbuf_adjust took place */
    uint32_t dst;
};

/* hdr->dst_addr, ipv4_adjust_cksum, pktmbuf_adjust(m, -l2_len) */
static void node_head(void *mbuf, const void *readable_end, struct node_mb *x)
{
    uint8_t *m = (uint8_t *)mbuf;
    const uintptr_t end = (uintptr_t)readable_end;
    memset(x, 0, sizeof(*x));
    if (!m || (end && (uintptr_t)m + 64u > end))
        return;
    uint64_t buf, txo;
    memcpy(&buf, m + NB_BUF_ADDR, 8);
    memcpy(&txo, m + NB_TX_OFFLOAD, 8);
    const uint16_t doff = ld16(m + NB_DATA_OFF), blen = ld16(m + NB_BUF_LEN), dlen = ld16(m + NB_DATA_LEN);
    x->f = (uintptr_t)buf + doff;
    x->lim = end ? end : (uintptr_t)buf + blen;
    if (end && x->f >= end)
        return; /* the frame lies outside the region */
    x->m = m;
    x->l2 = (uint32_t)(txo & 0x7Fu);
    uint32_t w[3] = {0, 0, 0};
    for (uint32_t j = 0; j < 12; j++)
        if (x->f + 8u + j < x->lim)
            w[j >> 2] |= (uint32_t)*(const uint8_t *)(x->f + 8u + j) << (8u * (j & 3u));
    x->dst = w[2];
    uint32_t ttl, ck;
    fwd_adjust_cksum(w[0], &ttl, &ck);
    if (x->f + 8u < x->lim)
        *(uint8_t *)(x->f + 8u) = (uint8_t)ttl;
    if (x->f + 10u < x->lim)
        *(uint8_t *)(x->f + 10u) = (uint8_t)ck;
    if (x->f + 11u < x->lim)
        *(uint8_t *)(x->f + 11u) = (uint8_t)(ck >> 8);
    x->adj = x->l2 <= doff; /* else pktmbuf_adj_offset answers NULL: the header fields stay */
    if (x->adj) {
        const uint16_t noff = (uint16_t)(doff - x->l2), nlen = (uint16_t)(dlen + x->l2);
        memcpy(m + NB_DATA_OFF, &noff, 2);
        memcpy(m + NB_DATA_LEN, &nlen, 2);
    }
}

int cndp_fwd_node_host(cndp_fwd_tbl_t *t, void *const *mbufs, uint32_t n, uint16_t *edges, const void *readable_end)
{
    if (!t || n > 256u || (n && (!mbufs || !edges)))
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    struct cne_fib *f0 = t->arp_fib < t->rt4_fib ? t->arp_fib : t->rt4_fib;
    struct cne_fib *f1 = t->arp_fib < t->rt4_fib ? t->rt4_fib : t->arp_fib;
    pthread_mutex_lock(&f0->t.dev_lock);
    if (f1 != f0)
        pthread_mutex_lock(&f1->t.dev_lock);
    const struct fwd_fibv arp = {(const uint32_t *)t->arp_fib->t.tbl24, (const uint32_t *)t->arp_fib->t.tbl8, NULL, NULL};
    const struct fwd_fibv rt = {(const uint32_t *)t->rt4_fib->t.tbl24, (const uint32_t *)t->rt4_fib->t.tbl8, NULL, NULL};
    const uint32_t *img = t->img;
    const uint32_t vec = n & ~3u; /* the 4-wide loop's share (:88), then the 1-wide loop (:271) */
    for (uint32_t i = 0; i < n;) {
        const uint32_t w = i < vec ? 4u : 1u;
        struct node_mb x[4];
        struct fwd_member mem[4];
        uint32_t hit = 0;
        for (uint32_t k = 0; k < w; k++) {
            node_head(mbufs[i + k], readable_end, &x[k]);
            fwd_rule_direct(img, &arp, x[k].dst, x[k].m != NULL, &mem[k]);
            hit |= mem[k].a_hit;
        }
        for (uint32_t k = 0; k < w; k++)
            fwd_rule_route(img, &arp, &rt, x[k].m != NULL, hit, &mem[k]);
        const uint32_t gw0 = mem[0].g_hit ? mem[0].g_idx : CNDP_FWD_NONE;
        for (uint32_t k = 0; k < w; k++) {
            if (!x[k].m) {
                edges[i + k] = (uint16_t)CNDP_FWD_EDGE_NONE;
                continue;
            }
            struct fwd_answer o;
            fwd_rule_finish(img, &mem[k], k != 0, gw0, &o);
            edges[i + k] = (uint16_t)o.edge;
            if (o.ha == CNDP_FWD_NONE || !x[k].adj)
                continue;
            /* d_addr at the new mtod + 0, s_addr at + 6, after the TTL / checksum bytes */
            const uint32_t d[3] = {o.d0, o.d1, o.d2};
            const uintptr_t eth = x[k].f - x[k].l2;
            for (uint32_t j = 0; j < 12; j++)
                if (eth + j < x[k].lim)
                    *(uint8_t *)(eth + j) = (uint8_t)(d[j >> 2] >> (8u * (j & 3u)));
        }
        i += w;
    }
    if (f1 != f0)
        pthread_mutex_unlock(&f1->t.dev_lock);
    pthread_mutex_unlock(&f0->t.dev_lock);
    pthread_mutex_unlock(&t->lock);
    return 0;
}

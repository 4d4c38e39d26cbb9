/*
 * tx.c -- the host side of include/cndp_tx.h: the PCB transmit attributes and
 * the image the device stage mirrors, the netifs' identification counters, and
 * udp_output + ip4_output (udp_output.c:33-65, ip4_output.c:48-126) frame by
 * frame over host memory.  Plain C, no HIP: it also builds into a stand-alone
 * program (tests/tx_host).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "tx_internal.h"

/* ---- PCB transmit attributes --------------------------------------------- */
/* call with the lock held: entries added since the last look get their defaults */
static int txa_sync(struct cndp_pcb_tbl *t)
{
    if (!t->txa) {
        t->txa = calloc(t->max, 3);
        if (!t->txa)
            return -ENOMEM;
        t->txa_n = 0;
    }
    for (; t->txa_n < t->count; t->txa_n++) {
        uint8_t *a = t->txa + 3u * (size_t)t->txa_n;
        a[0] = TX_TOS_DEFAULT;
        a[1] = TX_TTL_DEFAULT;
        a[2] = 17;
    }
    return 0;
}

int cndp_pcb_tx_set(cndp_pcb_tbl_t *t, uint32_t idx, const struct cndp_pcb_tx *a)
{
    if (!t || !a)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = idx >= t->count ? -EINVAL : t->closed[idx] ? -ENOENT : txa_sync(t);
    if (!r) {
        uint8_t *w = t->txa + 3u * (size_t)idx;
        w[0] = a->tos;
        w[1] = a->ttl;
        w[2] = a->ip_proto;
        t->gen++;
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_pcb_tx_get(cndp_pcb_tbl_t *t, uint32_t idx, struct cndp_pcb_tx *a)
{
    if (!t || !a)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = idx >= t->count ? -EINVAL : t->closed[idx] ? -ENOENT : txa_sync(t);
    if (!r) {
        const uint8_t *w = t->txa + 3u * (size_t)idx;
        a->tos = w[0];
        a->ttl = w[1];
        a->ip_proto = w[2];
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int tx_pcb_image(struct cndp_pcb_tbl *t)
{
    if (t->ximg_gen == t->gen)
        return 0;
    int r = txa_sync(t);
    if (r)
        return r;
    if (!t->ximg) {
        t->ximg = calloc(TXI_WORDS(t->max), sizeof(uint32_t));
        if (!t->ximg)
            return -ENOMEM;
    }
    t->ximg[0] = t->count;
    t->ximg[1] = t->ximg[2] = t->ximg[3] = 0;
    for (uint32_t i = 0; i < t->count; i++) {
        const uint8_t *a = t->txa + 3u * (size_t)i;
        uint32_t w = 0; /* a deleted entry: its attributes are cleared with it */
        if (!t->closed[i])
            w = TXW_LIVE | ((t->vec[i].opt_flag & CNDP_UDP_CHKSUM_FLAG) ? TXW_CKSUM : 0u) | (uint32_t)a[0] << 16 |
                (uint32_t)a[1] << 8 | a[2];
        t->ximg[TXI_HDR + i] = w;
    }
    t->ximg_gen = t->gen;
    return 0;
}

/* ---- identification counters ---------------------------------------------- */
/* call with the lock held: the host copy is what the last GPU call left */
int tx_ident_current(struct cndp_fwd_tbl *t)
{
    if (t->ident_dev_new && t->xdev_ident_pull)
        return t->xdev_ident_pull(t);
    return 0;
}

int cndp_fwd_netif_ident_set(cndp_fwd_tbl_t *t, uint32_t idx, uint16_t ident)
{
    if (!t || idx >= CNDP_FWD_NETIFS)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = tx_ident_current(t);
    if (!r) {
        t->ident[idx] = ident;
        t->ident_host_new = 1;
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_fwd_netif_ident_get(cndp_fwd_tbl_t *t, uint32_t idx, uint16_t *ident)
{
    if (!t || !ident || idx >= CNDP_FWD_NETIFS)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = tx_ident_current(t);
    if (!r)
        *ident = t->ident[idx];
    pthread_mutex_unlock(&t->lock);
    return r;
}

/* ---- the rule over host memory -------------------------------------------- */
/* cne_fib_lookup_bulk on the host image, DIR-24-8 4B (dir24_8.h:131-135) */
static uint32_t lpm4(const struct cne_fib *f, uint32_t ip)
{
    uint32_t e = ((const uint32_t *)f->t.tbl24)[ip >> 8];
    if (e & 1u)
        e = ((const uint32_t *)f->t.tbl8)[(size_t)(e >> 1) * CNDP_TBL8_GRP + (ip & 0xffu)];
    return e >> 1;
}

struct span {
    uint8_t *slab;
    uint64_t len;
};

static inline uint32_t rd8(const struct span *s, uint64_t o) { return o < s->len ? s->slab[o] : 0u; }
static inline void wr8(const struct span *s, uint64_t o, uint32_t v)
{
    if (o < s->len)
        s->slab[o] = (uint8_t)v;
}
static inline void wr16(const struct span *s, uint64_t o, uint32_t v) /* as a little-endian host stores it */
{
    wr8(s, o, v);
    wr8(s, o + 1, v >> 8);
}
static inline void wr32(const struct span *s, uint64_t o, uint32_t v)
{
    wr16(s, o, v);
    wr16(s, o + 2, v >> 16);
}
static inline uint32_t swap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }
static inline uint32_t reduce(uint32_t s) /* __cne_raw_cksum_reduce */
{
    s = (s >> 16) + (s & 0xffffu);
    s = (s >> 16) + (s & 0xffffu);
    return s & 0xffffu;
}

/* cne_ipv4_udptcp_cksum over the frame as it stands (net/cne_ip.h:275-325) */
static uint32_t udptcp_cksum(const struct span *s, uint64_t l4, uint32_t total, uint32_t proto, uint32_t src,
                             uint32_t dst)
{
    uint32_t c = 0;
    if (total >= 20u) {
        const uint32_t l4_len = total - 20u;
        uint32_t sum = 0; /* at most 32758 words of 16 bits: no overflow */
        for (uint32_t k = 0; k + 1 < l4_len; k += 2)
            sum += rd8(s, l4 + k) | rd8(s, l4 + k + 1) << 8;
        if (l4_len & 1u)
            sum += rd8(s, l4 + l4_len - 1u);
        const uint32_t ph = (src & 0xffffu) + (src >> 16) + (dst & 0xffffu) + (dst >> 16) + (proto << 8) + swap16(l4_len);
        c = reduce(sum) + reduce(ph);
        c = ((c >> 16) + (c & 0xffffu)) & 0xffffu;
    }
    c = ~c & 0xffffu;
    if (c == 0 && proto == 17u)
        c = 0xffffu;
    return c;
}

int cndp_tx_output_host(cndp_fwd_tbl_t *ft, cndp_pcb_tbl_t *pt, uint32_t mode, void *slab, uint64_t slab_len,
                        uint64_t stride, const uint64_t *offsets, uint32_t data_off, uint32_t n,
                        const struct cndp_tx_io *io)
{
    if (!ft || !pt || !io || mode > CNDP_TX_IP4)
        return -EINVAL;
    if (n && (!slab || !io->pcb || !io->faddr || !io->laddr || !io->len || !io->tx_edge ||
              (mode == CNDP_TX_UDP && !io->ports)))
        return -EINVAL;
    pthread_mutex_lock(&ft->lock);
    pthread_mutex_lock(&pt->lock);
    int r = 0;
    if (io->bin_of && ((int64_t)io->n_bins <= (int64_t)fwd_max_netif(ft) || io->n_bins > 65533u))
        r = -EINVAL;
    if (!r)
        r = tx_ident_current(ft);
    if (!r)
        r = tx_pcb_image(pt);
    if (r) {
        pthread_mutex_unlock(&pt->lock);
        pthread_mutex_unlock(&ft->lock);
        return r;
    }
    /* the FIBs' host images are painted under their own locks, taken in address order */
    struct cne_fib *f0 = ft->arp_fib < ft->rt4_fib ? ft->arp_fib : ft->rt4_fib;
    struct cne_fib *f1 = ft->arp_fib < ft->rt4_fib ? ft->rt4_fib : ft->arp_fib;
    pthread_mutex_lock(&f0->t.dev_lock);
    if (f1 != f0)
        pthread_mutex_lock(&f1->t.dev_lock);

    const struct span s = {(uint8_t *)slab, slab_len};
    const uint32_t bin_rest = io->n_bins + 1u;
    uint64_t st[CNDP_TX_NSTATS] = {0};
    for (uint32_t i = 0; i < n; i++) {
        uint32_t edge = CNDP_TX_EDGE_NONE, bin = bin_rest;
        const uint32_t p = io->pcb[i];
        uint32_t w = 0;
        if ((!io->sel || io->sel[i]) && p != CNDP_PCB_NONE && p < pt->count)
            w = pt->ximg[TXI_HDR + p];
        if (w & TXW_LIVE) {
            const uint32_t proto = w & 0xffu, src = io->laddr[i], dst = io->faddr[i];
            const uint64_t base = offsets ? offsets[i] : (uint64_t)i * stride;
            uint32_t h = data_off, dlen = io->len[i];
            edge = CNDP_TX_EDGE_PKT_DROP;
            do {
                if (mode == CNDP_TX_UDP) { /* udp_output */
                    if (h < 8u) {
                        st[CNDP_TX_STAT_DROP_HEADROOM]++;
                        break;
                    }
                    h -= 8u;
                    dlen = (dlen + 8u) & 0xffffu;
                    const uint32_t pp = io->ports[i];
                    wr32(&s, base + h, pp >> 16 | pp << 16); /* src_port = lport, dst_port = fport */
                    wr32(&s, base + h + 4u, swap16(dlen));   /* dgram_len, dgram_cksum = 0 */
                }
                const uint64_t l4 = base + h;
                if (h < 20u) {
                    st[CNDP_TX_STAT_DROP_HEADROOM]++;
                    break;
                }
                h -= 20u;
                dlen = (dlen + 20u) & 0xffffu;
                const uint64_t ip = base + h;
                const uint32_t w0 = 0x45u | ((w >> 16) & 0xffu) << 8 | swap16(dlen) << 16;
                const uint32_t w2 = ((w >> 8) & 0xffu) | proto << 8; /* ttl, proto, hdr_checksum = 0 */
                wr32(&s, ip, w0);
                wr16(&s, ip + 6u, 0); /* fragment_offset; packet_id is not written yet */
                wr32(&s, ip + 8u, w2);
                wr32(&s, ip + 12u, src);
                wr32(&s, ip + 16u, dst);
                const uint32_t ri = lpm4(ft->rt4_fib, __builtin_bswap32(src)) & 0xffffffu;
                const uint32_t *rt = ri < ft->rt_cap ? fwd_rt(ft) + 2u * (size_t)ri : NULL;
                if (!rt || !(rt[1] & FWD_SET)) {
                    st[CNDP_TX_STAT_DROP_NOROUTE]++;
                    break;
                }
                if (h < 14u) {
                    st[CNDP_TX_STAT_DROP_HEADROOM]++;
                    break;
                }
                h -= 14u;
                const uint64_t eth = base + h;
                const uint32_t nif = rt[1] & 0xffu;
                const uint32_t *mac = fwd_netif(ft) + 2u * (size_t)nif;
                wr32(&s, eth + 6u, mac[0]);
                wr16(&s, eth + 10u, mac[1]);
                wr16(&s, eth + 12u, 0x0008u);
                const uint32_t id = ft->ident[nif];
                wr16(&s, ip + 4u, swap16(id));
                ft->ident[nif] = (uint16_t)(id + swap16(dlen)); /* += ip->total_length as loaded */
                const uint32_t hs = (w0 & 0xffffu) + (w0 >> 16) + swap16(id) + (w2 & 0xffffu) + (src & 0xffffu) +
                                    (src >> 16) + (dst & 0xffffu) + (dst >> 16);
                wr16(&s, ip + 10u, ~reduce(hs) & 0xffffu);
                if (proto == 17u) {
                    if (w & TXW_CKSUM) {
                        wr16(&s, l4 + 6u, udptcp_cksum(&s, l4, dlen, proto, src, dst));
                        st[CNDP_TX_STAT_CKSUM]++;
                    }
                } else if (proto == 6u) {
                    wr16(&s, l4 + 16u, udptcp_cksum(&s, l4, dlen, proto, src, dst));
                    st[CNDP_TX_STAT_CKSUM]++;
                } else {
                    st[CNDP_TX_STAT_DROP_PROTO]++;
                    break;
                }
                edge = CNDP_TX_EDGE_ARP_REQUEST;
                bin = io->n_bins;
                const uint32_t ai = lpm4(ft->arp_fib, __builtin_bswap32(dst)) & 0xffffffu;
                const uint32_t *arp = ai < ft->arp_cap ? fwd_arp(ft) + 2u * (size_t)ai : NULL;
                if (arp && (arp[0] & FWD_SET)) {
                    wr16(&s, eth, arp[0]);
                    wr32(&s, eth + 2u, arp[1]);
                    edge = nif + CNDP_TX_EDGE_OUTPUT; /* the route's netif, not the ARP entry's */
                    bin = nif;
                    st[CNDP_TX_STAT_SENT]++;
                } else
                    st[CNDP_TX_STAT_ARP_REQUEST]++;
            } while (0);
        }
        io->tx_edge[i] = (uint16_t)edge;
        if (io->bin_of)
            io->bin_of[i] = (uint16_t)bin;
    }
    if (io->stats)
        for (int k = 0; k < CNDP_TX_NSTATS; k++)
            io->stats[k] += st[k];
    ft->ident_host_new = 1;

    if (f1 != f0)
        pthread_mutex_unlock(&f1->t.dev_lock);
    pthread_mutex_unlock(&f0->t.dev_lock);
    pthread_mutex_unlock(&pt->lock);
    pthread_mutex_unlock(&ft->lock);
    return 0;
}

/* ---- cndp_mqtx.h: udp_output + ip4_output over mbufs on the host ------------ */
static inline void st16(uint8_t *p, uint32_t v) /* as a little-endian host stores it */
{
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
}
static inline void st32(uint8_t *p, uint32_t v)
{
    st16(p, v);
    st16(p + 2, v >> 16);
}

int cndp_ip4_output_node_host(cndp_fwd_tbl_t *ft, cndp_pcb_tbl_t *pt, uint32_t mode, void *const *mbufs, uint32_t n,
                              uint16_t *edges, const void *readable_end, uint32_t stage_max,
                              void *(*metadata)(const void *m))
{
    if (!ft || !pt || mode > CNDP_TX_IP4 || n > 256u || (n && (!mbufs || !edges)))
        return -EINVAL;
    pthread_mutex_lock(&ft->lock);
    pthread_mutex_lock(&pt->lock);
    int r = tx_ident_current(ft);
    if (!r)
        r = tx_pcb_image(pt);
    if (r) {
        pthread_mutex_unlock(&pt->lock);
        pthread_mutex_unlock(&ft->lock);
        return r;
    }
    /* the FIBs' host images are painted under their own locks, taken in address order */
    struct cne_fib *f0 = ft->arp_fib < ft->rt4_fib ? ft->arp_fib : ft->rt4_fib;
    struct cne_fib *f1 = ft->arp_fib < ft->rt4_fib ? ft->rt4_fib : ft->arp_fib;
    pthread_mutex_lock(&f0->t.dev_lock);
    if (f1 != f0)
        pthread_mutex_lock(&f1->t.dev_lock);

    const uintptr_t end = (uintptr_t)readable_end;
    for (uint32_t i = 0; i < n; i++) {
        uint8_t *m = (uint8_t *)mbufs[i];
        edges[i] = (uint16_t)CNDP_TX_EDGE_NONE;
        if (!m || (end && (uintptr_t)m + 64u > end))
            continue;
        uint64_t buf, up;
        uint16_t H, blen, dlen0;
        memcpy(&buf, m + PCB_MB_BUF_ADDR, 8);
        memcpy(&up, m + PCB_MB_USERPTR, 8);
        memcpy(&H, m + PCB_MB_DATA_OFF, 2);
        memcpy(&blen, m + PCB_MB_BUF_LEN, 2);
        memcpy(&dlen0, m + PCB_MB_DATA_LEN, 2);
        uint8_t *const f = (uint8_t *)((uintptr_t)buf + H); /* mtod at submit */
        if (end && (uintptr_t)f > end)
            continue;
        const uint32_t w = up < pt->count ? pt->ximg[TXI_HDR + up] : 0u;
        uint8_t *md = NULL;
        if (w & TXW_LIVE)
            md = metadata ? (uint8_t *)metadata(m) : m + 64;
        uint32_t st = tx_reach_front(w, md == NULL, mode, H);
        if (st == TXS_NONE)
            continue;
        uint32_t edge = CNDP_TX_EDGE_PKT_DROP, proto_drop = 0, cksum = 0;
        uint32_t src = 0, dst = 0, U0 = 0, U1 = 0, rw = 0;
        const uint32_t proto = w & 0xffu, total = tx_total(mode, dlen0);
        uint8_t *l4 = f, *ip;
        if (st != TXS_NOMD) {
            uint16_t fport, lport;
            memcpy(&dst, md + 4, 4);
            memcpy(&src, md + PCB_MD_LADDR + 4, 4);
            memcpy(&fport, md + 2, 2);
            memcpy(&lport, md + PCB_MD_LADDR + 2, 2);
            if (mode == CNDP_TX_UDP && st != TXS_DROP_NOUDP) { /* udp_output */
                l4 = f - 8;
                U0 = (uint32_t)lport | (uint32_t)fport << 16; /* src_port = lport, dst_port = fport */
                U1 = tx_step((dlen0 + 8u) & 0xffffu);          /* dgram_len, dgram_cksum = 0 */
                st32(l4, U0);
                st32(l4 + 4, U1);
            }
        }
        if (st == TX_ROUTE) { /* ip4_output: the header but for packet_id, then the route */
            ip = l4 - 20;
            const uint32_t w0 = 0x45u | ((w >> 16) & 0xffu) << 8 | tx_step(total) << 16;
            const uint32_t w2 = ((w >> 8) & 0xffu) | proto << 8; /* ttl, proto, hdr_checksum = 0 */
            st32(ip, w0);
            st16(ip + 6, 0);
            st32(ip + 8, w2);
            st32(ip + 12, src);
            st32(ip + 16, dst);
            const uint32_t ri = lpm4(ft->rt4_fib, __builtin_bswap32(src)) & 0xffffffu;
            if (ri < ft->rt_cap)
                rw = fwd_rt(ft)[2u * (size_t)ri + 1u];
            st = tx_reach_route(rw, mode, H);
            if (st == TXS_OUT) {
                uint8_t *eth = ip - 14;
                const uint32_t nif = rw & 0xffu;
                const uint32_t *mac = fwd_netif(ft) + 2u * (size_t)nif;
                st32(eth + 6, mac[0]);
                st16(eth + 10, mac[1]);
                st16(eth + 12, 0x0008u);
                const uint32_t id = ft->ident[nif];
                st16(ip + 4, swap16(id));
                ft->ident[nif] = (uint16_t)(id + tx_step(total)); /* += ip->total_length as loaded */
                const uint32_t hs = (w0 & 0xffffu) + (w0 >> 16) + swap16(id) + (w2 & 0xffffu) + (src & 0xffffu) +
                                    (src >> 16) + (dst & 0xffffu) + (dst >> 16);
                st16(ip + 10, ~reduce(hs) & 0xffffu);
                cksum = proto == 17u ? (w & TXW_CKSUM) != 0 : proto == 6u;
                proto_drop = proto != 17u && proto != 6u;
                if (cksum) {
                    /* the readable L4 bytes from mtod on: data_len clipped at the buffer's end, the
                     * region's and stage_max; the rest read as zero and are never written */
                    uint32_t R = dlen0;
                    const uint32_t room = blen > H ? (uint32_t)(blen - H) : 0u;
                    R = R < room ? R : room;
                    if (end && end - (uintptr_t)f < R)
                        R = (uint32_t)(end - (uintptr_t)f);
                    if (stage_max && stage_max < R)
                        R = stage_max;
                    const uint32_t hdr = mode == CNDP_TX_UDP ? 8u : 0u;
                    const uint32_t l4_len = total >= 20u ? total - 20u : 0u;
                    uint32_t body = l4_len > hdr ? l4_len - hdr : 0u, S = 0;
                    body = body < R ? body : R;
                    for (uint32_t k = 0; k < body; k++)
                        S += (k & 1u) ? (uint32_t)f[k] << 8 : (uint32_t)f[k];
                    if (hdr)
                        S += tx_udp_hdr_sum(U0, U1, l4_len);
                    const uint32_t c = tx_l4_cksum(S, total, proto, src, dst);
                    const uint32_t at = proto == 17u ? 6u : 16u; /* from the L4 start */
                    for (uint32_t k = 0; k < 2u; k++)
                        if (at + k < hdr + R)
                            l4[at + k] = (uint8_t)(c >> (8u * k));
                }
                if (!proto_drop) {
                    edge = CNDP_TX_EDGE_ARP_REQUEST;
                    const uint32_t ai = lpm4(ft->arp_fib, __builtin_bswap32(dst)) & 0xffffffu;
                    const uint32_t *arp = ai < ft->arp_cap ? fwd_arp(ft) + 2u * (size_t)ai : NULL;
                    if (arp && (arp[0] & FWD_SET)) {
                        st16(eth, arp[0]);
                        st32(eth + 2, arp[1]);
                        edge = nif + CNDP_TX_EDGE_OUTPUT; /* the route's netif, not the ARP entry's */
                    }
                }
            }
        }
        tx_mbuf_apply(m, mode, st);
        edges[i] = (uint16_t)tx_mq_edge(st, edge, proto_drop, cksum);
    }
    ft->ident_host_new = 1;

    if (f1 != f0)
        pthread_mutex_unlock(&f1->t.dev_lock);
    pthread_mutex_unlock(&f0->t.dev_lock);
    pthread_mutex_unlock(&pt->lock);
    pthread_mutex_unlock(&ft->lock);
    return 0;
}

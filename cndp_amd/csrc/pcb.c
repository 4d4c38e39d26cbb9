/*
 * pcb.c -- the UDP PCB table of include/cndp_l4.h: what udp_input reads of the
 * stack's PCB vector (struct pcb_hd, lib/cnet/pcb/cnet_pcb.h:57-60), its
 * best-match lookup on the host (pcb_v4_lookup, cnet_pcb.c:41-92) and the
 * sorted image the device stage mirrors.  A table that holds the TCP vector
 * (include/cndp_tcp.h) gets a second image, an exact 4-tuple hash plus per-port
 * wildcard runs, which also answers cndp_pcb_lookup_indexed.  Plain C, no HIP:
 * it also builds into stand-alone programs (tests/l4_host, tests/tcp_host).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "pcb_internal.h"
#include "../../include/cndp_mql4.h"

static uint32_t pow2_ceil(uint32_t v)
{
    uint32_t p = 2;
    while (p < v)
        p <<= 1;
    return p;
}

int cndp_pcb_create(uint32_t max_entries, cndp_pcb_tbl_t **out)
{
    if (!out || max_entries == 0 || max_entries > CNDP_PCB_MAX_ENTRIES)
        return -EINVAL;
    struct cndp_pcb_tbl *t = calloc(1, sizeof(*t));
    if (!t)
        return -ENOMEM;
    size_t words = PCB_IMG_HDR + 3u * (size_t)max_entries + pow2_ceil(2u * max_entries) +
                   (max_entries + 1u) / 2u;
    t->vec = calloc(max_entries, sizeof(*t->vec));
    t->closed = calloc(max_entries, 1);
    t->img = calloc(words, sizeof(uint32_t));
    t->user = calloc(max_entries, sizeof(uint64_t));
    if (!t->vec || !t->closed || !t->img || !t->user || pthread_mutex_init(&t->lock, NULL)) {
        free(t->vec);
        free(t->closed);
        free(t->img);
        free(t->user);
        free(t);
        return -ENOMEM;
    }
    for (uint32_t i = 0; i < max_entries; i++)
        t->user[i] = i;
    t->max = max_entries;
    t->flags = PCB_F_PUNT;
    t->gen = 1;
    *out = t;
    return 0;
}

void cndp_pcb_free(cndp_pcb_tbl_t *t)
{
    if (!t)
        return;
    if (t->dev && t->dev_release)
        t->dev_release(t->dev);
    if (t->tdev && t->tdev_release)
        t->tdev_release(t->tdev);
    if (t->xdev && t->xdev_release)
        t->xdev_release(t->xdev);
    pthread_mutex_destroy(&t->lock);
    free(t->txa);
    free(t->ximg);
    free(t->vec);
    free(t->closed);
    free(t->img);
    free(t->timg);
    free(t->user);
    free(t);
}

int cndp_pcb_add(cndp_pcb_tbl_t *t, const struct cndp_pcb_entry *e)
{
    if (!t || !e)
        return -EINVAL;
    int r;
    pthread_mutex_lock(&t->lock);
    if (t->count >= t->max)
        r = -ENOSPC;
    else {
        r = (int)t->count;
        t->vec[t->count] = *e;
        t->closed[t->count] = 0;
        t->count++;
        t->gen++;
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_pcb_del(cndp_pcb_tbl_t *t, uint32_t idx)
{
    if (!t)
        return -EINVAL;
    int r = 0;
    pthread_mutex_lock(&t->lock);
    if (idx >= t->count)
        r = -EINVAL;
    else if (t->closed[idx])
        r = -ENOENT;
    else { /* cnet_pcb_free: memset 0, and the vector keeps the entry */
        memset(&t->vec[idx], 0, sizeof(t->vec[idx]));
        t->closed[idx] = 1;
        __atomic_store_n(&t->user[idx], (uint64_t)idx, __ATOMIC_RELAXED);
        t->gen++;
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_pcb_set_flags(cndp_pcb_tbl_t *t, int punt_enabled, int tcp_enabled)
{
    if (!t)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    uint32_t f = (punt_enabled ? PCB_F_PUNT : 0u) | (tcp_enabled ? PCB_F_TCP : 0u);
    if (f != t->flags) {
        t->flags = f;
        t->gen++;
    }
    pthread_mutex_unlock(&t->lock);
    return 0;
}

int cndp_pcb_count(cndp_pcb_tbl_t *t)
{
    if (!t)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = (int)t->count;
    pthread_mutex_unlock(&t->lock);
    return r;
}

/* pcb_v4_lookup, BEST_MATCH: the vector walked in order, fewest wildcards
 * wins, the first such entry, an exact match ends the walk */
static uint32_t lookup_one(const struct cndp_pcb_tbl *t, const struct cndp_pcb_key *k)
{
    uint32_t match = CNDP_PCB_NONE;
    int matchwild = 3;
    for (uint32_t i = 0; i < t->count; i++) {
        const struct cndp_pcb_entry *e = &t->vec[i];
        if (e->lport != k->lport)
            continue;
        int wild = 0;
        if (e->laddr != 0) {
            if (k->laddr == 0)
                wild++;
            else if (e->laddr != k->laddr)
                continue;
        } else if (k->laddr != 0)
            wild++;
        if (e->faddr != 0) {
            if (k->faddr == 0)
                wild++;
            else if (e->faddr != k->faddr || e->fport != k->fport)
                continue;
        } else if (k->faddr != 0)
            wild++;
        if (wild < matchwild) {
            match = i;
            matchwild = wild;
            if (wild == 0)
                break;
        }
    }
    return match;
}

int cndp_pcb_lookup(cndp_pcb_tbl_t *t, const struct cndp_pcb_key *keys, uint32_t n, uint32_t *idx_out)
{
    if (!t || (n && (!keys || !idx_out)))
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    for (uint32_t k = 0; k < n; k++)
        idx_out[k] = lookup_one(t, &keys[k]);
    pthread_mutex_unlock(&t->lock);
    return 0;
}

/* ---- device image ------------------------------------------------------ */
static int by_port_index(const void *a, const void *b)
{
    uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b; /* lport << 12 | index */
    return x < y ? -1 : x > y;
}

int pcb_image(struct cndp_pcb_tbl *t)
{
    if (t->img_gen == t->gen)
        return 0;
    uint32_t n = t->count;
    uint32_t *key = malloc((n ? n : 1u) * sizeof(uint32_t));
    if (!key)
        return -ENOMEM;
    for (uint32_t i = 0; i < n; i++)
        key[i] = (uint32_t)t->vec[i].lport << 12 | i;
    qsort(key, n, sizeof(uint32_t), by_port_index);
    uint32_t ports = 0;
    for (uint32_t j = 0; j < n; j++)
        ports += j == 0 || (key[j] >> 12) != (key[j - 1] >> 12);
    uint32_t H = pow2_ceil(2u * ports);
    uint32_t *img = t->img;
    uint32_t *laddr = img + PCB_IMG_HDR, *faddr = laddr + n, *pp = faddr + n, *slots = pp + n;
    uint16_t *idxf = (uint16_t *)(slots + H);
    uint32_t words = PCB_IMG_HDR + 3u * n + H + (n + 1u) / 2u;
    memset(img, 0, words * sizeof(uint32_t));
    img[0] = n;
    img[1] = H;
    img[2] = t->flags;
    img[3] = words;
    for (uint32_t j = 0; j < n; j++) {
        uint32_t i = key[j] & 0xfffu;
        const struct cndp_pcb_entry *e = &t->vec[i];
        laddr[j] = e->laddr;
        faddr[j] = e->faddr;
        pp[j] = (uint32_t)e->fport | (uint32_t)e->lport << 16;
        idxf[j] = (uint16_t)(i | ((e->opt_flag & CNDP_UDP_CHKSUM_FLAG) ? PCB_IDXF_CKSUM : 0u));
        if (j == 0 || (key[j] >> 12) != (key[j - 1] >> 12)) {
            uint32_t h = pcb_port_hash(e->lport, H);
            while (slots[h] & PCB_SLOT_VALID)
                h = (h + 1u) & (H - 1u);
            slots[h] = PCB_SLOT_VALID | (uint32_t)e->lport << 12 | j;
        }
    }
    free(key);
    t->img_words = words;
    t->img_gen = t->gen;
    return 0;
}

/* ---- TCP index image (pcb_internal.h) ----------------------------------- */
static int is_full(const struct cndp_pcb_entry *e) { return e->laddr != 0 && e->faddr != 0; }

int pcb_tcp_image(struct cndp_pcb_tbl *t)
{
    if (t->timg_gen == t->gen)
        return 0;
    if (!t->timg) { /* sized for the fullest table: both hashes at 2 * max slots */
        uint32_t hm = pow2_ceil(2u * t->max);
        t->timg = calloc(TCB_IMG_WORDS((size_t)t->max, hm, hm), sizeof(uint32_t));
        if (!t->timg)
            return -ENOMEM;
    }
    uint32_t n = t->count;
    uint32_t *key = malloc((n ? n : 1u) * sizeof(uint32_t));
    if (!key)
        return -ENOMEM;
    uint32_t nfull = 0;
    for (uint32_t i = 0; i < n; i++) { /* lport << 13 | fully specified << 12 | index */
        uint32_t f = (uint32_t)is_full(&t->vec[i]);
        nfull += f;
        key[i] = (uint32_t)t->vec[i].lport << 13 | f << 12 | i;
    }
    qsort(key, n, sizeof(uint32_t), by_port_index);
    uint32_t ports = 0;
    for (uint32_t j = 0; j < n; j++)
        ports += j == 0 || (key[j] >> 13) != (key[j - 1] >> 13);
    uint32_t HE = pow2_ceil(2u * nfull), HP = pow2_ceil(2u * ports);
    uint32_t *img = t->timg;
    uint32_t *laddr = img + TCB_IMG_HDR, *faddr = laddr + n, *pp = faddr + n, *es = pp + n, *ps = es + HE;
    uint16_t *idx = (uint16_t *)(ps + HP);
    uint32_t words = TCB_IMG_WORDS(n, HE, HP);
    memset(img, 0, words * sizeof(uint32_t));
    img[0] = n;
    img[1] = HE;
    img[2] = t->flags;
    img[3] = words;
    img[4] = HP;
    img[5] = nfull;
    for (uint32_t j = 0; j < n; j++) {
        uint32_t i = key[j] & 0xfffu;
        const struct cndp_pcb_entry *e = &t->vec[i];
        laddr[j] = e->laddr;
        faddr[j] = e->faddr;
        pp[j] = (uint32_t)e->fport | (uint32_t)e->lport << 16;
        idx[j] = (uint16_t)i;
        if (j == 0 || (key[j] >> 13) != (key[j - 1] >> 13)) {
            uint32_t h = pcb_port_hash(e->lport, HP);
            while (ps[h] & PCB_SLOT_VALID)
                h = (h + 1u) & (HP - 1u);
            ps[h] = PCB_SLOT_VALID | (uint32_t)e->lport << 12 | j;
        }
        if (is_full(e)) { /* positions rise with the index within a port: the first of equal tuples stays */
            uint32_t x = pcb_tcp_hash(e->laddr, e->faddr, pp[j]), h = x & (HE - 1u);
            int dup = 0;
            while (es[h] & PCB_SLOT_VALID) {
                uint32_t q = es[h] & 0xfffu;
                if (laddr[q] == e->laddr && faddr[q] == e->faddr && pp[q] == pp[j]) {
                    dup = 1;
                    break;
                }
                h = (h + 1u) & (HE - 1u);
            }
            if (!dup)
                es[h] = PCB_SLOT_VALID | (x >> 13) << 12 | j;
        }
    }
    free(key);
    t->timg_words = words;
    t->timg_gen = t->gen;
    return 0;
}

int cndp_pcb_lookup_indexed(cndp_pcb_tbl_t *t, const struct cndp_pcb_key *keys, uint32_t n, uint32_t *idx_out)
{
    if (!t || (n && (!keys || !idx_out)))
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = pcb_tcp_image(t);
    for (uint32_t k = 0; !r && k < n; k++)
        idx_out[k] = pcb_tcp_lookup(t->timg, keys[k].laddr, keys[k].faddr, keys[k].lport, keys[k].fport);
    pthread_mutex_unlock(&t->lock);
    return r;
}

/* ---- cndp_mql4.h: the user values and the two nodes over mbufs on the host --- */
int cndp_pcb_user_set(cndp_pcb_tbl_t *t, uint32_t idx, uint64_t user)
{
    if (!t)
        return -EINVAL;
    int r = 0;
    pthread_mutex_lock(&t->lock);
    if (idx >= t->count)
        r = -EINVAL;
    else /* cndp_gpu_mq_poll reads it without the lock */
        __atomic_store_n(&t->user[idx], user, __ATOMIC_RELAXED);
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_pcb_user_get(cndp_pcb_tbl_t *t, uint32_t idx, uint64_t *user)
{
    if (!t || !user)
        return -EINVAL;
    int r = 0;
    pthread_mutex_lock(&t->lock);
    if (idx >= t->count)
        r = -EINVAL;
    else
        *user = t->user[idx];
    pthread_mutex_unlock(&t->lock);
    return r;
}

/* byte o of a frame with R readable bytes: bytes past them read as zero */
static inline uint32_t fr8(const uint8_t *f, uint32_t R, uint32_t o) { return o < R ? f[o] : 0u; }

static inline uint32_t fr32(const uint8_t *f, uint32_t R, uint32_t o)
{
    return fr8(f, R, o) | fr8(f, R, o + 1u) << 8 | fr8(f, R, o + 2u) << 16 | fr8(f, R, o + 3u) << 24;
}

int cndp_udp_input_node_host(cndp_pcb_tbl_t *t, void *const *mbufs, uint32_t n, uint16_t *edges,
                             const void *readable_end, uint32_t stage_max, void *(*metadata)(const void *m))
{
    if (!t || n > 256u || (n && (!mbufs || !edges)))
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = pcb_image(t);
    if (r) {
        pthread_mutex_unlock(&t->lock);
        return r;
    }
    const uint32_t *img = t->img;
    const uint32_t flags = img[2];
    const uintptr_t end = (uintptr_t)readable_end;
    for (uint32_t i = 0; i < n; i++) {
        uint8_t *m = (uint8_t *)mbufs[i];
        edges[i] = (uint16_t)CNDP_MQ_EDGE_NONE;
        if (!m || (end && (uintptr_t)m + 64u > end))
            continue;
        uint64_t buf, txo;
        uint16_t doff, blen, dlen;
        memcpy(&buf, m + PCB_MB_BUF_ADDR, 8);
        memcpy(&txo, m + PCB_MB_TX_OFFLOAD, 8);
        memcpy(&doff, m + PCB_MB_DATA_OFF, 2);
        memcpy(&blen, m + PCB_MB_BUF_LEN, 2);
        memcpy(&dlen, m + PCB_MB_DATA_LEN, 2);
        const uintptr_t fa = (uintptr_t)buf + doff;
        if (end && fa >= end)
            continue; /* the frame lies outside the region */
        const uint8_t *f = (const uint8_t *)fa;
        /* the readable bytes: data_len, clipped at the buffer's end, the region's and stage_max */
        uint32_t R = dlen;
        const uint32_t room = blen > doff ? (uint32_t)(blen - doff) : 0u;
        R = R < room ? R : room;
        if (end && end - fa < R)
            R = (uint32_t)(end - fa);
        if (stage_max && stage_max < R)
            R = stage_max;
        const uint32_t l3 = (uint32_t)((txo >> 7) & 0x1ffu);
        const uint32_t pe = pcb_ip4_proto(fr8(f, R, 9), flags);
        if (pe) {
            edges[i] = CNDP_MQ_EDGE(CNDP_MQ_NODE_IP4_PROTO, pe - 1u);
            continue;
        }
        uint8_t *md = metadata ? (uint8_t *)metadata(m) : m + 64;
        if (!md) {
            edges[i] = CNDP_MQ_EDGE(CNDP_MQ_NODE_UDP_INPUT, CNDP_UDP_INPUT_PKT_DROP);
            continue;
        }
        const uint32_t faddr = fr32(f, R, 12), laddr = fr32(f, R, 16), ports = fr32(f, R, l3);
        const uint32_t ckf = fr8(f, R, l3 + 6u) | fr8(f, R, l3 + 7u);
        const uint32_t idf = pcb_udp_lookup(img, laddr, faddr, ports >> 16, ports & 0xffffu);
        uint32_t e;
        if (idf == CNDP_PCB_NONE) {
            e = CNDP_MQ_EDGE(CNDP_MQ_NODE_UDP_INPUT,
                             (flags & PCB_F_PUNT) ? CNDP_UDP_INPUT_PKT_PUNT : CNDP_UDP_INPUT_PKT_DROP);
        } else {
            e = CNDP_MQ_EDGE(CNDP_MQ_NODE_UDP_INPUT, CNDP_UDP_INPUT_CHNL_RECV);
            if ((idf & PCB_IDXF_CKSUM) && ckf) {
                const uint32_t ihl = (fr8(f, R, 0) & 0xfu) * 4u, tot = fr8(f, R, 2) << 8 | fr8(f, R, 3);
                uint32_t ok = 0;
                if (tot >= ihl) { /* __ipv4_udptcp_cksum: below it the sum is 0, which fails */
                    const uint32_t L = tot - ihl;
                    uint32_t S = 0;
                    for (uint32_t k = 0; k < L && l3 + k < R; k++)
                        S += (k & 1u) ? (uint32_t)f[l3 + k] << 8 : (uint32_t)f[l3 + k];
                    ok = pcb_udp_cksum_ok(S, pcb_udp_phdr_sum(faddr, laddr, 17u, L));
                }
                if (!ok)
                    e = CNDP_MQ_EDGE(CNDP_MQ_NODE_UDP_INPUT, CNDP_UDP_INPUT_PKT_DROP) | CNDP_MQ_EDGE_L4_CKSUM;
            }
        }
        edges[i] = (uint16_t)e;
        pcb_udp_apply(m, md, e, idf == CNDP_PCB_NONE ? 0u : t->user[idf & PCB_IDXF_IDX], ports, faddr, laddr);
    }
    pthread_mutex_unlock(&t->lock);
    return 0;
}

/* ---- cndp_mqtcp.h: the tcp_input node over mbufs on the host ---------------- */

/* the segment's little-endian 16-bit words summed, a last odd byte as a low byte
 * (cne_raw_cksum's sum before its reduce); below 2^31 for every length */
static inline uint32_t tcp_raw_sum(const uint8_t *p, uint32_t len)
{
    uint32_t S = 0, k = 0;
    for (; k + 2u <= len; k += 2u) {
        uint16_t w;
        memcpy(&w, p + k, 2);
        S += w;
    }
    if (k < len)
        S += p[k];
    return S;
}

/* cndp_tcp_input_node_host's walk with t->lock held.  hits (with optw) non-NULL:
 * also each mbuf's matched PCB index (CNDP_PCB_NONE: none, or the mbuf was not
 * taken) and, for a header offset above 20, the PCB_TCP_OPT_WORDS little-endian
 * words at mtod + l3_len + 20 of the mbuf as submitted, bytes past the readable
 * ones as zero -- what cndp_tcp_segment_node_host (tcb.c) goes on from.  Inlined
 * into its two callers with hits a constant, so that cndp_tcp_input_node_host's
 * loop carries nothing of the other's. */
static inline __attribute__((always_inline)) int tcp_node_walk(struct cndp_pcb_tbl *t, void *const *mbufs, uint32_t n,
                                                               uint16_t *edges, struct cndp_tcp_seg *segs,
                                                               uint32_t *const hits, uint32_t *const optw,
                                                               const void *readable_end, uint32_t stage_max,
                                                               void *(*metadata)(const void *m))
{
    const int r = pcb_tcp_image(t);
    if (r)
        return r;
    const uint32_t *img = t->timg;
    const uint32_t flags = img[2];
    const uintptr_t end = (uintptr_t)readable_end;
    for (uint32_t i = 0; i < n; i++) {
        uint8_t *m = (uint8_t *)mbufs[i];
        edges[i] = (uint16_t)CNDP_MQ_EDGE_NONE;
        if (segs)
            memset(&segs[i], 0, sizeof(segs[i]));
        if (hits)
            hits[i] = CNDP_PCB_NONE;
        if (!m || (end && (uintptr_t)m + 64u > end))
            continue;
        uint64_t buf, txo;
        uint16_t doff, blen, dlen;
        memcpy(&buf, m + PCB_MB_BUF_ADDR, 8);
        memcpy(&txo, m + PCB_MB_TX_OFFLOAD, 8);
        memcpy(&doff, m + PCB_MB_DATA_OFF, 2);
        memcpy(&blen, m + PCB_MB_BUF_LEN, 2);
        memcpy(&dlen, m + PCB_MB_DATA_LEN, 2);
        const uintptr_t fa = (uintptr_t)buf + doff;
        if (end && fa >= end)
            continue; /* the frame lies outside the region */
        const uint8_t *f = (const uint8_t *)fa;
        /* the readable bytes: data_len, clipped at the buffer's end, the region's and stage_max */
        uint32_t R = dlen;
        const uint32_t room = blen > doff ? (uint32_t)(blen - doff) : 0u;
        R = R < room ? R : room;
        if (end && end - fa < R)
            R = (uint32_t)(end - fa);
        if (stage_max && stage_max < R)
            R = stage_max;
        const uint32_t l3 = (uint32_t)((txo >> 7) & 0x1ffu);
        uint8_t *md = metadata ? (uint8_t *)metadata(m) : m + 64;
        struct cndp_tcp_seg seg;
        memset(&seg, 0, sizeof(seg));
        uint32_t e = 0, hit = CNDP_PCB_NONE, ports = 0, faddr = 0, laddr = 0, tot = 0;
        if (md) {
            uint32_t th[5], sw[4], L;
            for (uint32_t k = 0; k < 5u; k++)
                th[k] = fr32(f, R, l3 + 4u * k);
            const uint32_t w0 = fr32(f, R, 0);
            faddr = fr32(f, R, 12);
            laddr = fr32(f, R, 16);
            ports = th[0];
            tot = ((w0 >> 8) & 0xff00u) | (w0 >> 24);
            hit = pcb_tcp_lookup(img, laddr, faddr, ports >> 16, ports & 0xffffu);
            e = pcb_tcp_rule(hit, flags, w0, th, l3, sw, &L);
            memcpy(&seg, sw, sizeof(seg));
            if (e == PCB_TCP_E(CNDP_TCP_INPUT_SEGMENT)) {
                const uint32_t d0 = l3 < R ? l3 : R, d1 = l3 + L < R ? l3 + L : R;
                const uint32_t S = tcp_raw_sum(f + d0, d1 - d0);
                if (!pcb_udp_cksum_ok(S, pcb_udp_phdr_sum(faddr, laddr, fr8(f, R, 9), L)))
                    e = PCB_TCP_E(CNDP_TCP_INPUT_PKT_DROP) | CNDP_MQ_EDGE_L4_CKSUM;
            }
        }
        const uint32_t out = pcb_tcp_apply(m, md, e, hit == CNDP_PCB_NONE ? 0u : t->user[hit], ports, faddr, laddr,
                                           tot, &seg);
        edges[i] = (uint16_t)out;
        if (segs)
            segs[i] = seg;
        if (hits) { /* the option words as submitted, for a record that stands */
            hits[i] = hit;
            uint32_t *w = optw + (size_t)i * PCB_TCP_OPT_WORDS;
            memset(w, 0, PCB_TCP_OPT_WORDS * sizeof(uint32_t));
            if (seg.offset > 20u) {
                const uint32_t nw = seg.offset <= 32u ? 4u : PCB_TCP_OPT_WORDS; /* as the kernel reads them */
                for (uint32_t k = 0; k < nw; k++)
                    w[k] = fr32(f, R, l3 + 20u + 4u * k);
            }
        }
    }
    return 0;
}

int pcb_tcp_node_walk(struct cndp_pcb_tbl *t, void *const *mbufs, uint32_t n, uint16_t *edges,
                      struct cndp_tcp_seg *segs, uint32_t *hits, uint32_t *optw, const void *readable_end,
                      uint32_t stage_max, void *(*metadata)(const void *m))
{
    return tcp_node_walk(t, mbufs, n, edges, segs, hits, optw, readable_end, stage_max, metadata);
}

int cndp_tcp_input_node_host(cndp_pcb_tbl_t *t, void *const *mbufs, uint32_t n, uint16_t *edges,
                             struct cndp_tcp_seg *segs, const void *readable_end, uint32_t stage_max,
                             void *(*metadata)(const void *m))
{
    if (!t || n > 256u || (n && (!mbufs || !edges)))
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    const int r = tcp_node_walk(t, mbufs, n, edges, segs, NULL, NULL, readable_end, stage_max, metadata);
    pthread_mutex_unlock(&t->lock);
    return r;
}

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
    if (!t->vec || !t->closed || !t->img || pthread_mutex_init(&t->lock, NULL)) {
        free(t->vec);
        free(t->closed);
        free(t->img);
        free(t);
        return -ENOMEM;
    }
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

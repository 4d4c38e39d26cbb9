/*
 * acl.c -- the rule table of include/cndp_acl.h (acl_rules and fwd_acl_build of
 * examples/cndpfwd/acl-func.c), the builder of the image lookups read, and
 * acl_fwd_test's per-frame rule on the host (cndp_acl_classify_host).  Plain C,
 * no HIP: it also builds into a stand-alone program (tests/acl_host).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "acl_internal.h"

int cndp_acl_tbl_create(cndp_acl_tbl_t **out)
{
    if (!out)
        return -EINVAL;
    struct cndp_acl_tbl *t = calloc(1, sizeof(*t));
    if (!t)
        return -ENOMEM;
    if (pthread_mutex_init(&t->lock, NULL)) {
        free(t);
        return -ENOMEM;
    }
    *out = t;
    return 0;
}

void cndp_acl_tbl_destroy(cndp_acl_tbl_t *t)
{
    if (!t)
        return;
    if (t->dev && t->dev_release)
        t->dev_release(t->dev);
    pthread_mutex_destroy(&t->lock);
    free(t->img);
    free(t->rules);
    free(t);
}

/* call with the lock held: room for `want` rules in all.  acl_tbl_ensure_capacity */
static int reserve(struct cndp_acl_tbl *t, uint32_t want)
{
    if (want > CNDP_ACL_MAX_RULES)
        return -ENOSPC;
    if (want <= t->cap)
        return 0;
    uint32_t cap = t->cap ? t->cap : 64u;
    while (cap < want)
        cap *= 2u;
    if (cap > CNDP_ACL_MAX_RULES)
        cap = CNDP_ACL_MAX_RULES;
    struct cndp_acl_rule *r = realloc(t->rules, (size_t)cap * sizeof(*r));
    if (!r)
        return -ENOMEM;
    t->rules = r;
    t->cap = cap;
    return 0;
}

/* call with the lock held and room reserved */
static void push(struct cndp_acl_tbl *t, uint32_t src, uint32_t sm, uint32_t dst, uint32_t dm, int deny)
{
    struct cndp_acl_rule *r = &t->rules[t->n++];
    r->src_addr = src;
    r->dst_addr = dst;
    r->src_msk = (uint8_t)sm;
    r->dst_msk = (uint8_t)dm;
    r->deny = deny ? 1 : 0;
    r->rsvd = 0;
}

int cndp_acl_add(cndp_acl_tbl_t *t, const struct cndp_acl_rule *r)
{
    if (!t || !r || r->src_msk > 32 || r->dst_msk > 32)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int rc = reserve(t, t->n + 1u);
    if (!rc)
        push(t, r->src_addr, r->src_msk, r->dst_addr, r->dst_msk, r->deny);
    pthread_mutex_unlock(&t->lock);
    return rc;
}

int cndp_acl_clear(cndp_acl_tbl_t *t)
{
    if (!t)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    t->n = 0; /* the image stays: acl_tbl_clear does not touch the context */
    pthread_mutex_unlock(&t->lock);
    return 0;
}

int cndp_acl_count(cndp_acl_tbl_t *t)
{
    if (!t)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    const int n = (int)t->n;
    pthread_mutex_unlock(&t->lock);
    return n;
}

int cndp_acl_get(cndp_acl_tbl_t *t, uint32_t idx, struct cndp_acl_rule *out)
{
    if (!t || !out)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    const int rc = idx < t->n ? 0 : -EINVAL;
    if (!rc)
        *out = t->rules[idx];
    pthread_mutex_unlock(&t->lock);
    return rc;
}

#define IPV4(a, b, c, d) ((uint32_t)(a) << 24 | (uint32_t)(b) << 16 | (uint32_t)(c) << 8 | (uint32_t)(d))

int cndp_acl_add_init_rules(cndp_acl_tbl_t *t)
{
    if (!t)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int rc = reserve(t, t->n + CNDP_ACL_INIT_RULES);
    if (!rc) {
        for (uint32_t i = 0; i < 100u; i++) /* acl-func.c:424-432 */
            push(t, 0, 0, IPV4(100, i, 0, 0), 24, 1);
        for (uint32_t i = 0; i < 15u; i++) /* :437-445 */
            push(t, IPV4(10u + i, 0, 0, 0), 8, 0, 0, 1);
        for (uint32_t i = 0; i < 15u; i++) /* :450-458 */
            push(t, IPV4(101, 0, i, 0), 24, 0, 0, 1);
        for (uint32_t i = 0; i < 4096u; i++) /* :463-475 */
            push(t, IPV4(210, 0, i >> 8, i & 0xffu), 32, IPV4(110, 0, i >> 8, i & 0xffu), 32, 0);
    }
    pthread_mutex_unlock(&t->lock);
    return rc;
}

struct grp {
    uint32_t keys, first, off, slots;
    uint8_t sm, dm;
};

int cndp_acl_build(cndp_acl_tbl_t *t)
{
    if (!t)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    /* fwd_acl_build frees the old context first; a build that fails leaves none */
    free(t->img);
    t->img = NULL;
    t->img_words = 0;
    t->gen++;
    int rc = t->n ? 0 : -EINVAL; /* cne_acl_build on an empty context */
    uint16_t *gid = NULL;
    struct grp *g = NULL;
    uint32_t *img = NULL;
    if (rc)
        goto out;
    gid = malloc(ACL_GROUPS_MAX * sizeof(*gid));
    g = calloc(ACL_GROUPS_MAX, sizeof(*g));
    rc = gid && g ? 0 : -ENOMEM;
    if (rc)
        goto out;
    memset(gid, 0xff, ACL_GROUPS_MAX * sizeof(*gid));
    /* the groups in the order of their first rule, which is ascending by lowest index */
    uint32_t ng = 0;
    for (uint32_t i = 0; i < t->n; i++) {
        const struct cndp_acl_rule *r = &t->rules[i];
        const uint32_t k = r->src_msk * 33u + r->dst_msk;
        if (gid[k] == 0xffffu) {
            gid[k] = (uint16_t)ng;
            g[ng].first = i;
            g[ng].sm = r->src_msk;
            g[ng].dm = r->dst_msk;
            ng++;
        }
        g[gid[k]].keys++; /* an upper bound until duplicates are met below */
    }
    size_t words = ACL_HDR_WORDS + (size_t)ng * ACL_DESC_WORDS;
    for (uint32_t j = 0; j < ng; j++) {
        uint32_t slots = 2u;
        while (slots < 2u * g[j].keys)
            slots *= 2u;
        if (2u * slots <= ACL_SPARSE_SLOTS)
            slots *= 2u; /* a small table at load 1/4: a miss then ends after 1.4 probes on average, not 2.5 */
        g[j].slots = slots;
        g[j].off = (uint32_t)words; /* at most 4 * 100000 + 4 * 1089 slots: far below 2^32 words */
        g[j].keys = 0;
        words += (size_t)slots * ACL_SLOT_WORDS;
    }
    img = calloc(words, sizeof(*img));
    rc = img ? 0 : -ENOMEM;
    if (rc)
        goto out;
    for (uint32_t i = 0; i < t->n; i++) {
        const struct cndp_acl_rule *r = &t->rules[i];
        struct grp *q = &g[gid[r->src_msk * 33u + r->dst_msk]];
        const uint32_t ks = r->src_addr & acl_mask(r->src_msk), kd = r->dst_addr & acl_mask(r->dst_msk);
        const uint32_t m = q->slots - 1u;
        uint32_t h = acl_hash(ks, kd);
        for (;; h++) { /* ends: fewer than half the slots are ever taken */
            uint32_t *s = img + q->off + (size_t)(h & m) * ACL_SLOT_WORDS;
            if (!s[2]) {
                s[0] = ks;
                s[1] = kd;
                s[2] = (i + 1u) | (r->deny ? ACL_VAL_DENY : 0u);
                q->keys++;
                break;
            }
            if (s[0] == ks && s[1] == kd)
                break; /* an earlier rule holds this key and always wins */
        }
    }
    img[0] = ACL_MAGIC;
    img[1] = ng;
    img[2] = t->n;
    img[3] = (uint32_t)words;
    for (uint32_t j = 0; j < ng; j++) {
        uint32_t *d = img + ACL_HDR_WORDS + (size_t)j * ACL_DESC_WORDS;
        d[0] = acl_mask(g[j].sm);
        d[1] = acl_mask(g[j].dm);
        d[2] = g[j].off;
        d[3] = g[j].slots - 1u;
        d[4] = g[j].first;
        d[5] = g[j].sm | (uint32_t)g[j].dm << 8;
        d[6] = g[j].keys;
    }
    t->img = img;
    t->img_words = words;
    img = NULL;
out:
    free(img);
    free(g);
    free(gid);
    pthread_mutex_unlock(&t->lock);
    return rc;
}

int acl_io_check(const struct cndp_batch *b, uint32_t mode, uint32_t flags, const struct cndp_acl_io *io)
{
    if (!b || !io || mode > CNDP_ACL_PERMISSIVE || (flags & ~CNDP_ACL_F_MAC_SWAP) || io->in_lport > 255u)
        return -EINVAL;
    if (b->n && (!b->slab || !io->verdict || (b->slab_len >> 63)))
        return -EINVAL;
    if (io->bin_of) {
        uint32_t top = io->in_lport;
        for (uint32_t p = 0; p < 256u; p++)
            if ((io->lport_mask[p >> 6] >> (p & 63u)) & 1u && p > top)
                top = p;
        if (io->n_bins <= top || io->n_bins > CNDP_PART_BINS_MAX)
            return -EINVAL;
    }
    return 0;
}

/* frame byte k (relative to the frame's first byte at slab offset at), zero at or past len */
static uint32_t rd_byte(const uint8_t *s, uint64_t len, uint64_t at, uint32_t k)
{
    const uint64_t x = at + k;
    return x >= at && x < len ? s[x] : 0u; /* x >= at: no wrap for an offset near 2^64 */
}

static uint32_t rd_le32(const uint8_t *s, uint64_t len, uint64_t at, uint32_t k)
{
    return rd_byte(s, len, at, k) | rd_byte(s, len, at, k + 1u) << 8 | rd_byte(s, len, at, k + 2u) << 16 |
           rd_byte(s, len, at, k + 3u) << 24;
}

int cndp_acl_classify_host(cndp_acl_tbl_t *t, const struct cndp_batch *b, uint32_t mode, uint32_t flags,
                           const struct cndp_acl_io *io)
{
    if (!t)
        return -EINVAL;
    int rc = acl_io_check(b, mode, flags, io);
    if (rc)
        return rc;
    pthread_mutex_lock(&t->lock);
    const uint32_t *img = t->img;
    if (!img) {
        pthread_mutex_unlock(&t->lock);
        return -ENOENT;
    }
    uint8_t *slab = (uint8_t *)(uintptr_t)b->slab; /* written only with the swap flag */
    const uint64_t len = b->slab_len;
    uint64_t st[CNDP_ACL_NSTATS] = {0, 0, 0};
    for (uint32_t i = 0; i < b->n; i++) {
        uint32_t res = 0, v = CNDP_ACL_NONE, tx = CNDP_ACL_LPORT_NONE;
        if (!io->sel || io->sel[i]) {
            const uint64_t at = (b->offsets ? b->offsets[i] : (uint64_t)i * b->stride) + b->data_off;
            v = CNDP_ACL_PREFILTER;
            if (!acl_prefilter(rd_le32(slab, len, at, 14), !io->len || io->len[i] >= 20u)) {
                res = acl_lookup(img, __builtin_bswap32(rd_le32(slab, len, at, 26)),
                                 __builtin_bswap32(rd_le32(slab, len, at, 30)));
                v = acl_decide(res, mode);
            }
            if (v == CNDP_ACL_FORWARD) {
                tx = acl_tx_lport(rd_byte(slab, len, at, 5), io->lport_mask[0], io->lport_mask[1], io->lport_mask[2],
                                  io->lport_mask[3], io->in_lport);
                if (flags & CNDP_ACL_F_MAC_SWAP) { /* byte 14 lies inside the slab, so do bytes 0-11 */
                    uint8_t *p = slab + at, tmp[6];
                    memcpy(tmp, p, 6);
                    memcpy(p, p + 6, 6);
                    memcpy(p + 6, tmp, 6);
                }
            }
            st[v - 1u]++;
        }
        if (io->result)
            io->result[i] = res;
        io->verdict[i] = (uint8_t)v;
        if (io->tx_lport)
            io->tx_lport[i] = (uint8_t)tx;
        if (io->bin_of)
            io->bin_of[i] = (uint16_t)(v == CNDP_ACL_FORWARD ? tx : v == CNDP_ACL_DENY ? io->n_bins : io->n_bins + 1u);
    }
    if (io->stats)
        for (uint32_t k = 0; k < CNDP_ACL_NSTATS; k++)
            io->stats[k] += st[k];
    pthread_mutex_unlock(&t->lock);
    return 0;
}

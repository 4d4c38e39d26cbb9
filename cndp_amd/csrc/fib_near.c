/*
 * fib_near.c -- host maintenance of the /16 directory in front of tbl24 and of
 * its "near image" (fib_internal.h), for 4-B DIR-24-8 tables.  Plain C, no
 * device call: cndp_gpu.hip calls in here under dev_lock -- the directory at
 * sync time, the image before a launch that reads it -- and uploads what the
 * dirty ranges name; the tests drive it without a device.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "fib_internal.h"

/* all 256 entries of a block equal: the block against itself one entry on
 * (the C library's vector compare, which stops at the first difference) */
static inline int uniform256(const uint32_t *e)
{
    return memcmp(e, e + 1, 255 * 4) == 0;
}

static int dir16_page_alloc(struct cndp_tbl *t)
{
    if (t->n_free)
        return (int)t->page_free[--t->n_free];
    if (t->page_hwm == t->cap_pages) {
        const uint32_t ncap = t->cap_pages ? t->cap_pages * 2 : 64;
        uint32_t *np = (uint32_t *)realloc(t->pages, (size_t)ncap * 256 * 4);
        if (np)
            t->pages = np;
        uint32_t *nf = (uint32_t *)realloc(t->page_free, (size_t)ncap * 4);
        if (nf)
            t->page_free = nf;
        if (!np || !nf)
            return -ENOMEM;
        t->cap_pages = ncap;
    }
    return (int)t->page_hwm++;
}

static inline void near_dirty(struct cndp_tbl *t, uint64_t lo, uint64_t hi)
{
    if (lo < t->dn_lo)
        t->dn_lo = lo;
    if (hi > t->dn_hi)
        t->dn_hi = hi;
}

/* refresh the near image of /8 blocks [a0, a1] from dir16 */
static int near_update(struct cndp_tbl *t, uint32_t a0, uint32_t a1)
{
    if (!t->near_img) {
        t->near_img = (uint32_t *)calloc(CNDP_NEAR_ENT, 4);
        if (!t->near_img)
            return -ENOMEM;
        for (uint32_t a = 0; a < 256; a++)
            t->mid_of[a] = -1;
        t->n_mid_free = t->n_mid_used = t->mid_hwm = 0;
        a0 = 0;
        a1 = 255;
        t->dn_lo = 0;
        t->dn_hi = 256;
    }
    for (uint32_t a = a0; a <= a1; a++) {
        const uint32_t *d = t->dir16 + (size_t)a * 256;
        const uint32_t v = d[0];
        const int uni = !(v & 1u) && uniform256(d);
        uint32_t nt;
        if (uni) {
            if (t->mid_of[a] >= 0) {
                t->mid_free[t->n_mid_free++] = (uint8_t)t->mid_of[a];
                t->mid_of[a] = -1;
                t->n_mid_used--;
            }
            nt = v;
        } else {
            if (t->mid_of[a] < 0) { /* at most one slot per /8, so never more than 256 */
                t->mid_of[a] = t->n_mid_free ? (int16_t)t->mid_free[--t->n_mid_free] : (int16_t)t->mid_hwm++;
                t->n_mid_used++;
            }
            const uint32_t slot = (uint32_t)t->mid_of[a];
            const uint64_t base = 256u + (uint64_t)slot * 256u;
            uint32_t *m = t->near_img + base;
            uint32_t lo = 256, hi = 0;
            for (uint32_t b = 0; b < 256; b++)
                if (m[b] != d[b]) {
                    m[b] = d[b];
                    if (b < lo)
                        lo = b;
                    hi = b + 1;
                }
            if (hi > lo)
                near_dirty(t, base + lo, base + hi);
            nt = (slot << 1) | 1u;
        }
        if (t->near_img[a] != nt) {
            t->near_img[a] = nt;
            near_dirty(t, a, a + 1u);
        }
    }
    return 0;
}

/* bring the near image up to the directory: the /8 blocks marked stale, 256
 * compares each (all of them the first time) */
int cndp_tbl_near_refresh(struct cndp_tbl *t)
{
    if (!t->dir16)
        return 0;
    if (!t->near_img) {
        const int r = near_update(t, 0, 255);
        if (r)
            return r;
    } else {
        for (uint32_t w = 0; w < 4; w++)
            for (uint64_t m = t->near_stale[w]; m; m &= m - 1) {
                const uint32_t a = w * 64u + (uint32_t)__builtin_ctzll(m);
                const int r = near_update(t, a, a);
                if (r)
                    return r;
            }
    }
    memset(t->near_stale, 0, sizeof(t->near_stale));
    return 0;
}

/* refresh the directory entries of /16 blocks [k0, k1] and mark the /8 blocks
 * they lie in for the near image (a sync pays a few bit sets, not the image) */
int cndp_tbl_dir16_update(struct cndp_tbl *t, uint32_t k0, uint32_t k1)
{
    if (!t->dir16) {
        t->dir16 = (uint32_t *)calloc(65536, 4);
        t->page_of = (int32_t *)malloc(65536 * 4);
        if (!t->dir16 || !t->page_of)
            return -ENOMEM;
        for (uint32_t k = 0; k < 65536; k++)
            t->page_of[k] = -1;
        k0 = 0;
        k1 = 65535;
        t->dd_lo = t->dp_lo = ~0ULL;
        t->dd_hi = t->dp_hi = 0;
    }
    const uint32_t *t24 = (const uint32_t *)(const void *)t->tbl24;
    for (uint32_t k = k0; k <= k1; k++) {
        const uint32_t *e = t24 + (size_t)k * 256;
        const uint32_t v = e[0];
        const int uni = !(v & 1u) && uniform256(e);
        uint32_t nd;
        if (uni) {
            if (t->page_of[k] >= 0) {
                t->page_free[t->n_free++] = (uint32_t)t->page_of[k];
                t->page_of[k] = -1;
                t->n_pages_used--;
            }
            nd = v;
        } else {
            if (t->page_of[k] < 0) {
                const int pg = dir16_page_alloc(t);
                if (pg < 0)
                    return pg;
                t->page_of[k] = pg;
                t->n_pages_used++;
            }
            const uint64_t pe = (uint64_t)t->page_of[k] * 256;
            memcpy(t->pages + pe, e, 256 * 4);
            if (pe < t->dp_lo)
                t->dp_lo = pe;
            if (pe + 256 > t->dp_hi)
                t->dp_hi = pe + 256;
            nd = ((uint32_t)t->page_of[k] << 1) | 1u;
        }
        if (t->dir16[k] != nd || t->dd_hi == 0) {
            t->dir16[k] = nd;
            if (k < t->dd_lo)
                t->dd_lo = k;
            if ((uint64_t)k + 1 > t->dd_hi)
                t->dd_hi = (uint64_t)k + 1;
        }
    }
    for (uint32_t a = k0 >> 8; a <= k1 >> 8; a++)
        t->near_stale[a >> 6] |= 1ULL << (a & 63u);
    return 0;
}

/* bring the directory and the near image up to the host tbl24 without a
 * device: walks the pending tbl24 changes and leaves them pending, so a later
 * device sync still uploads them (the walk is idempotent) */
int cndp_tbl_dir16_refresh(struct cndp_tbl *t)
{
    if (!t || !t->tbl24 || t->is_trie || t->nh_sz != 2)
        return -ENOTSUP;
    int r = 0;
    if (!t->dir16)
        r = cndp_tbl_dir16_update(t, 0, 65535);
    else if (t->d24_hi <= t->d24_lo)
        r = 0;
    else if (t->n_log24 <= CNDP_TBL_LOG)
        for (uint32_t k = 0; !r && k < t->n_log24; k++)
            r = cndp_tbl_dir16_update(t, (uint32_t)(t->log24[k].lo >> 8), (uint32_t)((t->log24[k].hi - 1) >> 8));
    else
        r = cndp_tbl_dir16_update(t, (uint32_t)(t->d24_lo >> 8), (uint32_t)((t->d24_hi - 1) >> 8));
    return r ? r : cndp_tbl_near_refresh(t);
}

/* top -> mid -> page -> tbl8: the rule the LDS-image classify kernel applies */
uint32_t cndp_tbl_near_lookup(const struct cndp_tbl *t, uint32_t ip)
{
    uint32_t e = t->near_img[ip >> 24];
    if (e & 1u)
        e = t->near_img[256u + (e >> 1) * 256u + ((ip >> 16) & 0xffu)];
    if (e & 1u)
        e = t->pages[(size_t)(e >> 1) * 256u + ((ip >> 8) & 0xffu)];
    if (e & 1u)
        e = ((const uint32_t *)(const void *)t->tbl8)[(size_t)(e >> 1) * 256u + (ip & 0xffu)];
    return e >> 1;
}

int cndp_fib_near_refresh(struct cne_fib *fib)
{
    if (!fib)
        return -EINVAL;
    pthread_mutex_lock(&fib->t.dev_lock);
    const int r = cndp_tbl_dir16_refresh(&fib->t);
    pthread_mutex_unlock(&fib->t.dev_lock);
    return r;
}

int cndp_fib_near_info(struct cne_fib *fib, struct cndp_fib_near_info *out)
{
    if (!fib || !out)
        return -EINVAL;
    struct cndp_tbl *t = &fib->t;
    pthread_mutex_lock(&t->dev_lock);
    const int have = t->near_img != NULL;
    out->kib = have ? cndp_tbl_near_kib(t) : 0;
    out->cap_kib = CNDP_NEAR_CAP_KIB;
    out->mid_used = t->n_mid_used;
    out->mid_hwm = t->mid_hwm;
    out->pages_used = t->n_pages_used;
    out->page_hwm = t->page_hwm;
    out->fits = (uint32_t)cndp_tbl_near_fits(t);
    pthread_mutex_unlock(&t->dev_lock);
    return have ? 0 : -ENOENT;
}

int cndp_fib_near_lookup(struct cne_fib *fib, const uint32_t *ips, uint64_t *next_hops, uint32_t n)
{
    if (!fib || (n && (!ips || !next_hops)))
        return -EINVAL;
    struct cndp_tbl *t = &fib->t;
    pthread_mutex_lock(&t->dev_lock);
    int r = cndp_tbl_dir16_refresh(t);
    for (uint32_t i = 0; !r && i < n; i++)
        next_hops[i] = cndp_tbl_near_lookup(t, ips[i]);
    pthread_mutex_unlock(&t->dev_lock);
    return r;
}

/*
 * cfwd.c -- the host side of include/cndp_cfwd.h: l3fwd_fib_init and the next
 * hop packing of examples/cndpfwd/l3-fwd.c, the argument checks, and the rule
 * of _fwd_test / _l3fwd_test on the calling thread (cndp_cfwd_host).  Plain C,
 * no HIP: it also builds into a stand-alone program (tests/cfwd_host).
 */
#include <errno.h>
#include <string.h>

#include "cfwd_internal.h"
#include "fib_internal.h"

struct cne_fib *cndp_cfwd_fib_create(const char *name)
{
    struct cne_fib_conf c; /* l3-fwd.c:98-103 */
    memset(&c, 0, sizeof(c));
    c.type = CNE_FIB_DUMMY;
    c.max_routes = CNDP_CFWD_MAX_ROUTES;
    c.default_nh = CNDP_CFWD_DEFAULT_NH;
    return cne_fib_create(name, &c);
}

uint64_t cndp_cfwd_nexthop(const uint8_t mac[6], uint16_t tx_port)
{
    if (!mac)
        return 0;
    uint64_t v = 0; /* inet_mtoh64 */
    for (int k = 0; k < 6; k++)
        v = v << 8 | mac[k];
    return (uint64_t)tx_port << 48 | v; /* l3-fwd.c:67 */
}

int cndp_cfwd_route_add(struct cne_fib *fib, uint32_t ip, uint8_t depth, const uint8_t mac[6], uint16_t tx_port)
{
    if (!fib || !mac || tx_port > CNDP_CFWD_PORT_MAX)
        return -EINVAL;
    return cne_fib_add(fib, ip, depth, cndp_cfwd_nexthop(mac, tx_port));
}

int cfwd_io_check(struct cne_fib *fib, const struct cndp_batch *b, uint32_t mode, const struct cndp_cfwd_io *io)
{
    if (!b || !io || mode > CNDP_CFWD_L3FWD || io->in_lport > 255u)
        return -EINVAL;
    if (mode == CNDP_CFWD_L3FWD && (!fib || fib->t.nh_sz != 3u || fib->t.is_trie))
        return -EINVAL;
    if (b->n && (!b->slab || !io->tx_lport || (b->slab_len >> 63)))
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

/* the low `cnt` bytes of v to frame bytes k ..., those inside the slab */
static void st_bytes(uint8_t *s, uint64_t len, uint64_t at, uint32_t k, uint32_t v, uint32_t cnt)
{
    for (uint32_t j = 0; j < cnt; j++) {
        const uint64_t x = at + k + j;
        if (x >= at && x < len)
            s[x] = (uint8_t)(v >> (8u * j));
    }
}

int cndp_cfwd_host(struct cne_fib *fib, const struct cndp_batch *b, uint32_t mode, const struct cndp_cfwd_io *io)
{
    int rc = cfwd_io_check(fib, b, mode, io);
    if (rc)
        return rc;
    const int l3 = mode == CNDP_CFWD_L3FWD;
    uint8_t *slab = (uint8_t *)(uintptr_t)b->slab;
    const uint64_t len = b->slab_len;
    uint64_t st[CNDP_CFWD_NSTATS] = {0, 0};
    /* a DUMMY FIB's group pool moves when a route is added: read under the table's lock */
    if (l3)
        pthread_mutex_lock(&fib->t.dev_lock);
    const uint64_t *t24 = l3 ? (const uint64_t *)(const void *)fib->t.tbl24 : NULL;
    const uint64_t *t8 = l3 ? (const uint64_t *)(const void *)fib->t.tbl8 : NULL;
    for (uint32_t i = 0; i < b->n; i++) {
        uint64_t nh = 0;
        uint32_t tx = CNDP_CFWD_LPORT_NONE, echo = 0;
        const int taken = !io->sel || io->sel[i];
        if (taken) {
            const uint64_t at = (b->offsets ? b->offsets[i] : (uint64_t)i * b->stride) + b->data_off;
            struct cfwd_frame f;
            struct cfwd_edit e;
            f.d0 = rd_le32(slab, len, at, 0);
            f.d1 = rd_le32(slab, len, at, 4);
            f.d2 = rd_le32(slab, len, at, 8);
            f.ttl = rd_byte(slab, len, at, 22);
            f.ck = rd_byte(slab, len, at, 24) | rd_byte(slab, len, at, 25) << 8;
            f.dst = rd_le32(slab, len, at, 30);
            cfwd_rule(mode, &f, t24, t8, io->lport_mask[0], io->lport_mask[1], io->lport_mask[2], io->lport_mask[3],
                      io->in_lport, &e);
            if (l3) {
                st_bytes(slab, len, at, 22, e.ttl, 1);
                st_bytes(slab, len, at, 24, e.ck, 2);
            }
            st_bytes(slab, len, at, 0, e.d0, 4);
            if (l3 && !e.echo) {
                st_bytes(slab, len, at, 4, e.d1, 2);
            } else {
                st_bytes(slab, len, at, 4, e.d1, 4);
                st_bytes(slab, len, at, 8, e.d2, 4);
            }
            nh = e.nh;
            tx = e.tx;
            echo = e.echo;
            st[echo ? CNDP_CFWD_STAT_ECHO : CNDP_CFWD_STAT_FORWARD]++;
        }
        if (io->nh)
            io->nh[i] = nh;
        io->tx_lport[i] = (uint16_t)tx;
        if (io->echoed)
            io->echoed[i] = (uint8_t)echo;
        if (io->bin_of)
            io->bin_of[i] = (uint16_t)(taken ? tx : io->n_bins);
    }
    if (l3)
        pthread_mutex_unlock(&fib->t.dev_lock);
    if (io->stats)
        for (uint32_t k = 0; k < CNDP_CFWD_NSTATS; k++)
            io->stats[k] += st[k];
    return 0;
}

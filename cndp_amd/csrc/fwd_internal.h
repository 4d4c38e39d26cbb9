/* The forwarding table behind include/cndp_fwd.h, shared by fwd.c (host, plain
 * C) and cndp_fwd.hip (the device mirror). */
#ifndef CNDP_FWD_INTERNAL_H
#define CNDP_FWD_INTERNAL_H

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cndp_fwd.h"
#include "fib_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Object image (u32 words), kept up to date in place by every change and
 * mirrored to the device as it is:
 *   [0] arp_cap  [1] rt_cap  [2] total words  [3] 0
 *   arp[arp_cap]  two words each:  FWD_SET | netif_idx << 16 | ha[0] | ha[1] << 8,
 *                                  ha[2] | ha[3] << 8 | ha[4] << 16 | ha[5] << 24
 *   rt[rt_cap]    two words each:  gateway,  FWD_SET | netif_idx
 *   netif[256]    two words each:  mac[0..3],  mac[4] | mac[5] << 8
 * A slot that is not set is all zero. */
#define FWD_IMG_HDR 4u
#define FWD_SET 0x80000000u
#define FWD_IMG_WORDS(arp, rt) (FWD_IMG_HDR + 2u * (size_t)(arp) + 2u * (size_t)(rt) + 2u * CNDP_FWD_NETIFS)

struct cndp_fwd_tbl {
    pthread_mutex_t lock; /* serialises changes, host lookups and GPU calls */
    struct cne_fib *arp_fib, *rt4_fib;
    uint32_t arp_cap, rt_cap;
    uint32_t *img;
    size_t img_words;
    uint64_t gen;                       /* bumped by every change */
    size_t d_lo, d_hi;                  /* image words changed since the mirror's last copy */
    uint32_t nif_refs[CNDP_FWD_NETIFS]; /* objects set per netif_idx */
    void *dev;                          /* the device mirror's state, owned by cndp_fwd.hip */
    void (*dev_release)(void *dev);
    /* transmit side (include/cndp_tx.h), kept by tx.c */
    uint16_t ident[CNDP_FWD_NETIFS];    /* the netifs' ip_ident, host copy */
    int ident_host_new;                 /* set on the host since the device copy was written */
    int ident_dev_new;                  /* a GPU call advanced the device copy since the last read-back */
    void *xdev;                         /* the transmit stage's device state, owned by cndp_tx.hip */
    void (*xdev_release)(void *xdev);
    int (*xdev_ident_pull)(struct cndp_fwd_tbl *t); /* lock held: wait, read the counters back */
};

static inline uint32_t *fwd_arp(const struct cndp_fwd_tbl *t) { return t->img + FWD_IMG_HDR; }
static inline uint32_t *fwd_rt(const struct cndp_fwd_tbl *t) { return fwd_arp(t) + 2u * (size_t)t->arp_cap; }
static inline uint32_t *fwd_netif(const struct cndp_fwd_tbl *t) { return fwd_rt(t) + 2u * (size_t)t->rt_cap; }

/* Call with tbl->lock held: the largest netif_idx an object names, or -1. */
int fwd_max_netif(const struct cndp_fwd_tbl *t);

/* ---- the node's rule, one text for fwd.c (cndp_fwd_node_host) and the mbuf
 * queue's kernel (k_mq_ip4_forward, cndp_gpu.hip) ------------------------- */
#if defined(__HIPCC__)
#define FWD_HD __host__ __device__
#else
#define FWD_HD
#endif

/* One FIB as the rule reads it, DIR-24-8 with 4-byte entries: the host image
 * (d16 / pages NULL) or a device mirror, with the /16 directory in front of
 * tbl24 when the mirror has one. */
struct fwd_fibv {
    const uint32_t *t24, *t8, *d16, *pages;
};

/* cne_fib_lookup_bulk for one key (dir24_8.h:131-135) */
static inline FWD_HD uint32_t fwd_fib_lookup(const struct fwd_fibv *f, uint32_t ip)
{
    uint32_t e;
    if (f->d16) {
        e = f->d16[ip >> 16];
        if (e & 1u)
            e = f->pages[(e >> 1) * 256u + ((ip >> 8) & 0xffu)];
    } else
        e = f->t24[ip >> 8];
    if (e & 1u)
        e = f->t8[(size_t)(e >> 1) * 256u + (ip & 0xffu)];
    return e >> 1;
}

/* What a member of a group carries between the rule's three steps. */
struct fwd_member {
    uint32_t key;   /* be32toh(hdr->dst_addr) */
    uint32_t a_idx; /* the ARP object of the destination, when a_hit */
    uint32_t g_idx; /* the ARP object of the route's gateway, when g_hit */
    uint32_t r_nif; /* the route's netif, when g_hit */
    uint32_t a_hit, g_hit;
};

/* What the rule leaves for a member: the node's edge (CNDP_FWD_EDGE_ARP_REQUEST
 * or netif + 2, FWD_EDGE_GATEWAY OR-ed in for the gateway case), and for a
 * transmitted member the 12 bytes d_addr | s_addr as three little-endian
 * dwords; ha is the ARP object whose address was taken, else CNDP_FWD_NONE. */
#define FWD_EDGE_GATEWAY 0x0400u /* CNDP_MQ_EDGE_FWD_GATEWAY (cndp_mqcnet.h) */
struct fwd_answer {
    uint32_t edge, ha;
    uint32_t d0, d1, d2;
};

/* fib_info_lookup's object test: index below the capacity and the slot set */
static inline FWD_HD uint32_t fwd_arp_set_at(const uint32_t *img, uint32_t idx)
{
    return idx < img[0] && (img[FWD_IMG_HDR + 2u * (size_t)idx] & FWD_SET) != 0u;
}

/* Step 1, every member: the ARP FIB on the destination (ip4_forward.c:134,285).
 * `taken` 0 stands for a member the caller could not read: it keeps its place
 * in the group and hits nothing. */
static inline FWD_HD void fwd_rule_direct(const uint32_t *img, const struct fwd_fibv *arp, uint32_t dst_be,
                                          uint32_t taken, struct fwd_member *m)
{
    m->key = __builtin_bswap32(dst_be);
    m->a_idx = m->g_idx = CNDP_FWD_NONE;
    m->r_nif = 0;
    m->a_hit = m->g_hit = 0;
    if (taken) {
        m->a_idx = fwd_fib_lookup(arp, m->key) & 0xffffffu;
        m->a_hit = fwd_arp_set_at(img, m->a_idx);
    }
}

/* Step 2, every member once its group's hits are known: group_hit is the
 * member's own a_hit in the 1-wide loop and the OR over the four members in
 * the 4-wide loop, where one direct hit keeps the whole group away from the
 * route FIB (:134-160).  Otherwise the route FIB, and the ARP FIB on the route
 * object's gateway as it is stored (:164-178, :291-296); a member without a
 * route object has no gateway and stays a miss. */
static inline FWD_HD void fwd_rule_route(const uint32_t *img, const struct fwd_fibv *arp, const struct fwd_fibv *rt,
                                         uint32_t taken, uint32_t group_hit, struct fwd_member *m)
{
    if (!taken || group_hit)
        return;
    const uint32_t *rto = img + FWD_IMG_HDR + 2u * (size_t)img[0];
    const uint32_t r_idx = fwd_fib_lookup(rt, m->key) & 0xffffffu;
    if (r_idx >= img[1])
        return;
    const uint32_t gw = rto[2u * (size_t)r_idx], rw = rto[2u * (size_t)r_idx + 1u];
    if (!(rw & FWD_SET))
        return;
    m->r_nif = rw & 0xffu;
    m->g_idx = fwd_fib_lookup(arp, gw) & 0xffffffu;
    m->g_hit = fwd_arp_set_at(img, m->g_idx);
}

/* Step 3, every member: the edge and the MACs.  `follower` is set for lanes
 * 1-3 of a 4-wide group, which take the ha of lane 0's gateway entry gw0
 * (:190,196,202) -- their own when lane 0 has none (gw0 == CNDP_FWD_NONE). */
static inline FWD_HD void fwd_rule_finish(const uint32_t *img, const struct fwd_member *m, uint32_t follower,
                                          uint32_t gw0, struct fwd_answer *o)
{
    const uint32_t *arpo = img + FWD_IMG_HDR;
    const uint32_t *nif = arpo + 2u * (size_t)img[0] + 2u * (size_t)img[1];
    uint32_t out_nif = 0, gwbit = 0;
    o->edge = CNDP_FWD_EDGE_ARP_REQUEST;
    o->ha = CNDP_FWD_NONE;
    o->d0 = o->d1 = o->d2 = 0;
    if (m->a_hit) {
        o->ha = m->a_idx;
        out_nif = (arpo[2u * (size_t)m->a_idx] >> 16) & 0xffu;
    } else if (m->g_hit) {
        o->ha = follower && gw0 != CNDP_FWD_NONE ? gw0 : m->g_idx;
        out_nif = m->r_nif;
        gwbit = FWD_EDGE_GATEWAY;
    } else
        return;
    const uint32_t h0 = arpo[2u * (size_t)o->ha], h1 = arpo[2u * (size_t)o->ha + 1u];
    const uint32_t m0 = nif[2u * out_nif], m1 = nif[2u * out_nif + 1u];
    o->edge = (out_nif + CNDP_FWD_EDGE_OUTPUT) | gwbit;
    o->d0 = (h0 & 0xffffu) | h1 << 16; /* d_addr at +0, s_addr at +6 */
    o->d1 = h1 >> 16 | m0 << 16;
    o->d2 = m0 >> 16 | m1 << 16;
}

/* ipv4_adjust_cksum (cnet_ipv4.h:159-170) on header bytes 8-11 as one
 * little-endian dword (ttl | proto << 8 | checksum << 16): the new TTL and the
 * new checksum as a little-endian halfword. */
static inline FWD_HD void fwd_adjust_cksum(uint32_t w, uint32_t *ttl, uint32_t *ck)
{
    const int32_t c = (int32_t)((w >> 16) ^ 0xffffu) + (int32_t)0xfffe; /* htobe16(0xFEFF) */
    *ttl = (w - 1u) & 0xffu;
    *ck = ~(uint32_t)(c + (c >> 16)) & 0xffffu;
}

/* The device mirror's reader protocol (cndp_fwd.hip), for a launch that reads
 * the object image and both FIB mirrors on `stream` of device `dev`:
 * fwd_dev_begin takes t->lock, binds the table to the device (-EINVAL when it
 * is bound to another), makes `stream` wait for the last reader when that was
 * another stream, copies a changed image to the mirror, syncs both FIB mirrors
 * and takes a view of each.  It returns 0 with t->lock and both views HELD, or
 * a negative errno with nothing held.  fwd_dev_end, called after the launch is
 * enqueued (launched != 0) or given up (0), drops the views, records the
 * reader's end on `stream` for the next call and releases the lock. */
int fwd_dev_begin(struct cndp_fwd_tbl *t, int dev, void *stream, const uint32_t **img, struct fwd_fibv *arp,
                  struct fwd_fibv *rt);
int fwd_dev_end(struct cndp_fwd_tbl *t, void *stream, int launched);
/* 0, or -EINVAL when the table is bound to another device than `dev` */
int fwd_dev_check(struct cndp_fwd_tbl *t, int dev);

#ifdef __cplusplus
}
#endif
#endif

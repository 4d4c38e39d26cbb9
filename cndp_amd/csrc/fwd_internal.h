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

#ifdef __cplusplus
}
#endif
#endif

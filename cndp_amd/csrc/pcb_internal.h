/* The PCB table behind include/cndp_l4.h and include/cndp_tcp.h, shared by pcb.c
 * (host, plain C) and cndp_l4.hip / cndp_tcp.hip (the device mirrors). */
#ifndef CNDP_PCB_INTERNAL_H
#define CNDP_PCB_INTERNAL_H

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cndp_tcp.h" /* includes cndp_l4.h */

#ifdef __cplusplus
extern "C" {
#endif

#define PCB_F_PUNT 1u
#define PCB_F_TCP 2u

/* Device image (u32 words), rebuilt by pcb_image() when the table changed:
 *   [0] n  [1] H  [2] flags  [3] total words
 *   laddr[n]  faddr[n]  ports[n] (fport | lport << 16)  slots[H]  idxf[(n + 1) / 2]
 * Entries are sorted by (lport, index), so all entries of one local port form a
 * run.  slots is an open-addressed (linear probing, load <= 1/2) map from a
 * local port to the start of its run: PCB_SLOT_VALID | lport << 12 | start;
 * the run ends where ports[j] >> 16 changes.  idxf holds u16 values:
 * the entry's index in vector order | PCB_IDXF_CKSUM when it has
 * CNDP_UDP_CHKSUM_FLAG. */
#define PCB_IMG_HDR 4u
#define PCB_SLOT_VALID 0x80000000u
#define PCB_IDXF_CKSUM 0x8000u
#define PCB_IDXF_IDX 0x0fffu

#if defined(__HIPCC__)
#define PCB_HD __host__ __device__
#else
#define PCB_HD
#endif
static inline PCB_HD uint32_t pcb_port_hash(uint32_t lport, uint32_t H)
{
    return ((lport * 0x9E3779B1u) >> 15) & (H - 1u);
}

struct cndp_pcb_tbl {
    pthread_mutex_t lock;   /* serialises changes, lookups and GPU calls */
    uint32_t max;
    uint32_t count;         /* vector length, deleted entries included */
    uint32_t flags;         /* PCB_F_* */
    struct cndp_pcb_entry *vec;
    uint8_t *closed;        /* 1 = deleted (zeroed, still in the vector) */
    uint64_t gen;           /* bumped by every change */
    uint32_t *img;          /* device image, host copy */
    uint32_t img_words;
    uint64_t img_gen;       /* gen the image was built from (0 = never) */
    void *dev;              /* the device mirror's state, owned by cndp_l4.hip */
    void (*dev_release)(void *dev);
    uint32_t *timg;         /* TCP index image (below), host copy, allocated on first use */
    uint32_t timg_words;
    uint64_t timg_gen;      /* gen the TCP image was built from (0 = never) */
    void *tdev;             /* the TCP stage's device mirror, owned by cndp_tcp.hip */
    void (*tdev_release)(void *tdev);
    /* transmit side (include/cndp_tx.h), kept by tx.c */
    uint8_t *txa;           /* per entry: tos, ttl, ip_proto; allocated on first use */
    uint32_t txa_n;         /* entries of the vector given their defaults so far */
    uint32_t *ximg;         /* transmit image (tx_internal.h), host copy */
    uint64_t ximg_gen;      /* gen the transmit image was built from (0 = never) */
    void *xdev;             /* the transmit stage's device mirror, owned by cndp_tx.hip */
    void (*xdev_release)(void *xdev);
};

/* Call with tbl->lock held: bring tbl->img up to date.  0 or -ENOMEM. */
int pcb_image(struct cndp_pcb_tbl *tbl);

/* TCP index image (u32 words), rebuilt by pcb_tcp_image() when the table changed.
 * A TCP vector is thousands of connections on a few listening ports, so a key is
 * answered from an exact 4-tuple hash and only falls back to a walk of its
 * port's wildcard entries:
 *   [0] n  [1] HE  [2] flags  [3] total words  [4] HP  [5] fully specified entries
 *   [6] [7] 0
 *   laddr[n]  faddr[n]  ports[n] (fport | lport << 16)  eslots[HE]  pslots[HP]
 *   idx[(n + 1) / 2]  (u16: the entry's index in vector order)
 * Entries are sorted by (lport, fully specified, index): a port's entries form
 * a run, its wildcard entries (a zero address; deleted entries are any/any on
 * port 0) first and in vector order, its fully specified entries after them.
 *   eslots  open-addressed (linear probing, load <= 1/2) over the fully
 *           specified entries' (laddr, faddr, ports): PCB_SLOT_VALID |
 *           tag << 12 | position, tag = the hash's top 19 bits, so a probe that
 *           does not own the slot almost never reads the three entry words.
 *           Equal tuples are inserted once, for their lowest vector index.
 *   pslots  the UDP image's port directory: PCB_SLOT_VALID | lport << 12 | run start.
 * At 4096 entries: 8 + 3 * 4096 + 8192 + 8192 + 2048 = 30728 words = 122912
 * bytes at most (every entry fully specified and on a port of its own),
 * inside the 160 KiB of LDS a block can have; 4096 connections on one port
 * take 8 + 3 * 4096 + 8192 + 2 + 2048 words = 90152 bytes.
 * A slot is one dword because lanes of a wave probe scattered slots: each
 * probe is one 4-byte LDS read whose bank is random, and a wider slot would
 * put more bytes behind the same conflicts. */
#define TCB_IMG_HDR 8u
#define TCB_IMG_WORDS(max, he, hp) (TCB_IMG_HDR + 3u * (max) + (he) + (hp) + ((max) + 1u) / 2u)

static inline PCB_HD uint32_t pcb_tcp_hash(uint32_t laddr, uint32_t faddr, uint32_t ports)
{
    /* every input bit reaches the slot bits and the tag: tuples that differ in
     * one address byte or in a port's byte order must not share a chain */
    uint32_t x = laddr * 0x9E3779B1u;
    x ^= x >> 15;
    x += faddr * 0x85EBCA77u;
    x ^= x >> 13;
    x += ports * 0xC2B2AE3Du;
    x ^= x >> 16;
    x *= 0x27D4EB2Fu;
    x ^= x >> 15;
    return x;
}

/* pcb_v4_lookup, BEST_MATCH, answered from the TCP image `img` (host memory or
 * the kernel's LDS copy): the entry's vector index or CNDP_PCB_NONE.
 *  - key with both addresses non-zero: a fully specified entry matches it only
 *    when all four fields are equal, with 0 wildcards, and every wildcard entry
 *    scores >= 1, so an exact-hash hit (lowest index of equal tuples) is the
 *    linear walk's answer.  Without one, only wildcard entries can match: the
 *    first of the port's wildcard run with the fewest wildcards.
 *  - key with a zero address: fully specified entries match with wildcards too;
 *    the whole run is walked and the least (wildcards, index) wins. */
static inline PCB_HD uint32_t pcb_tcp_lookup(const uint32_t *img, uint32_t laddr, uint32_t faddr,
                                             uint32_t lport, uint32_t fport)
{
    const uint32_t n = img[0], HE = img[1], HP = img[4];
    const uint32_t *t_laddr = img + TCB_IMG_HDR, *t_faddr = t_laddr + n, *t_ports = t_faddr + n;
    const uint32_t *es = t_ports + n, *ps = es + HE;
    const uint16_t *idx = (const uint16_t *)(ps + HP);
    const uint32_t ports = fport | lport << 16;
    const int full_key = laddr != 0 && faddr != 0;
    if (full_key) {
        const uint32_t x = pcb_tcp_hash(laddr, faddr, ports), tag = x >> 13;
        for (uint32_t h = x & (HE - 1u);; h = (h + 1u) & (HE - 1u)) {
            const uint32_t s = es[h];
            if (!(s & PCB_SLOT_VALID))
                break;
            if (((s >> 12) & 0x7ffffu) == tag) {
                const uint32_t j = s & 0xfffu;
                if (t_laddr[j] == laddr && t_faddr[j] == faddr && t_ports[j] == ports)
                    return idx[j];
            }
        }
    }
    uint32_t s;
    for (uint32_t h = pcb_port_hash(lport, HP);; h = (h + 1u) & (HP - 1u)) {
        s = ps[h];
        if (!(s & PCB_SLOT_VALID))
            return CNDP_PCB_NONE;
        if (((s >> 12) & 0xffffu) == lport)
            break;
    }
    uint32_t bestw = 3, besti = CNDP_PCB_NONE;
    for (uint32_t j = s & 0xfffu; j < n; j++) {
        const uint32_t pp = t_ports[j];
        if ((pp >> 16) != lport)
            break;
        const uint32_t el = t_laddr[j], ef = t_faddr[j];
        if (full_key && el != 0 && ef != 0)
            break; /* the run's fully specified part: the exact probe answered for it */
        uint32_t w = 0;
        if (el != 0) {
            if (laddr == 0)
                w++;
            else if (el != laddr)
                continue;
        } else if (laddr != 0)
            w++;
        if (ef != 0) {
            if (faddr == 0)
                w++;
            else if (ef != faddr || (pp & 0xffffu) != fport)
                continue;
        } else if (faddr != 0)
            w++;
        const uint32_t i = idx[j];
        if (w < bestw || (w == bestw && i < besti)) {
            bestw = w;
            besti = i;
            if (full_key && w == 1)
                break; /* wildcard entries are in vector order and none scores 0 */
        }
    }
    return besti;
}

/* Call with tbl->lock held: bring tbl->timg up to date.  0 or -ENOMEM. */
int pcb_tcp_image(struct cndp_pcb_tbl *tbl);

#ifdef __cplusplus
}
#endif
#endif

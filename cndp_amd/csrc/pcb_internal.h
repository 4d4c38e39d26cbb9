/* The PCB table behind include/cndp_l4.h, shared by pcb.c (host, plain C) and
 * cndp_l4.hip (the device mirror). */
#ifndef CNDP_PCB_INTERNAL_H
#define CNDP_PCB_INTERNAL_H

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cndp_l4.h"

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
};

/* Call with tbl->lock held: bring tbl->img up to date.  0 or -ENOMEM. */
int pcb_image(struct cndp_pcb_tbl *tbl);

#ifdef __cplusplus
}
#endif
#endif

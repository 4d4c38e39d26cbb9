/* The TCB table behind include/cndp_tcb.h, shared by tcb.c (host, plain C) and
 * cndp_tcb.hip (the device mirror), and the per-segment rule both apply. */
#ifndef CNDP_TCB_INTERNAL_H
#define CNDP_TCB_INTERNAL_H

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cndp_tcb.h"
#include "pcb_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Image: TCB_WORDS u32 words per PCB index, kept up to date in place by every
 * change and mirrored to the device as it is -- struct cndp_tcb's own layout,
 * with rsvd[0] = 1 for an index that has a TCB.  A slot without one is all zero.
 *   [0] rcv_nxt  [1] snd_una  [2] snd_nxt  [3] snd_max
 *   [4] snd_wnd  [5] snd_cwnd  [6] ts_recent  [7] last_ack_sent
 *   [8] rcv_space  [9] max_mss | state << 16 | snd_scale << 24
 *   [10] flags | present << 8
 *   [11] the transmit attributes of include/cndp_tcpout.h, which the segment rule
 *        below does not read: tflags | req_recv_scale << 8 | rcv_scale << 16 */
#define TCB_WORDS 12u
#define TCB_PRESENT 0x100u /* in word 10 */

struct cndp_tcb_tbl {
    pthread_mutex_t lock; /* serialises changes, the host twin and GPU calls; taken before pcb->lock */
    struct cndp_pcb_tbl *pcb;
    uint32_t cap;         /* pcb->max */
    uint32_t *img;        /* cap * TCB_WORDS */
    uint64_t gen;         /* bumped by every change */
    uint32_t d_lo, d_hi;  /* entries changed since the mirror's last copy */
    uint64_t pcb_gen;     /* pcb->gen the deleted entries were last looked at (0 = never) */
    void *dev;            /* the device mirror's state, owned by cndp_tcb.hip */
    void (*dev_release)(void *dev);
    /* transmit side (include/cndp_tcpout.h) */
    uint32_t *kimg;       /* PCB key image (tcpout_internal.h), allocated on first use */
    uint64_t kimg_gen;    /* pcb->gen the key image was built from (0 = never) */
    /* the queue mode's host twin (include/cndp_mqtcb.h) */
    uint32_t *seen;       /* cap stamps: the twin call that last judged a segment of the PCB */
    uint32_t seen_call;   /* the current call's stamp, never 0 */
};

/* Call with t->lock held: take the TCBs of PCBs deleted since the last look
 * away, and return the PCB vector's length. */
uint32_t tcb_reconcile(struct cndp_tcb_tbl *t);

/* Readers of the image's device mirror (cndp_tcb.hip): cndp_gpu_tcp_segment and
 * the mbuf queue's CNDP_MQ_TCP_SEGMENT kernels in cndp_gpu.hip.  The protocol is
 * pcb_tdev_begin / _end / _check's (pcb_internal.h).  tcb_dev_begin takes
 * t->lock, orders `stream` after a reader on another stream, brings the mirror
 * up to date on `stream` and answers the mirror's address; the lock is held
 * until tcb_dev_end, which records the reader's end where it launched.  A
 * reader that takes both tables begins this one first and ends it last: t->lock
 * is taken before pcb->lock.
 * staging = NULL: changed entries are copied from the host image and the copy is
 * waited for, as the host image may change once the lock is gone.  staging =
 * pinned memory of t->cap * TCB_WORDS * 4 bytes that the caller leaves alone until
 * the work it enqueues next on `stream` has completed: the changed entries are
 * snapshot there and copied from there, and nothing is waited for -- stream order
 * keeps the copy behind the stream's earlier readers.  The mirror's allocation,
 * at a table's first use, waits either way. */
int tcb_dev_begin(struct cndp_tcb_tbl *t, int dev, void *stream, void *staging, const uint32_t **img);
int tcb_dev_end(struct cndp_tcb_tbl *t, void *stream, int launched);
int tcb_dev_check(struct cndp_tcb_tbl *t, int dev);

#define TCB_TCP_FIN 0x01u
#define TCB_TCP_SYN 0x02u
#define TCB_TCP_ACK 0x10u
#define TCB_HDR_PREDIC 0x37u /* SYN | FIN | RST | URG | ACK, cnet_tcp.h:160 */
#define TCB_HDR_LEN 20u
/* the option bytes a segment can carry, and the byte at opt_end itself */
#define TCB_OPT_WORDS 11u

/* Word k of the option bytes; a k past them reads as zero.  The kernel keeps
 * the words in registers, so the index has to become a chain of selects there. */
static inline PCB_HD uint32_t tcb_opt_word(const uint32_t *w, uint32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r = 0;
#pragma unroll
    for (uint32_t j = 0; j < TCB_OPT_WORDS; j++)
        r = k == j ? w[j] : r;
    return r;
#else
    return k < TCB_OPT_WORDS ? w[k] : 0u;
#endif
}

/* The four option bytes at position pos, opts[pos] in the low byte. */
static inline PCB_HD uint32_t tcb_opt_win(const uint32_t *w, uint32_t pos)
{
    const uint32_t k = pos >> 2, sh = (pos & 3u) * 8u;
    const uint32_t lo = tcb_opt_word(w, k), hi = tcb_opt_word(w, k + 1u);
    return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
}

static inline PCB_HD uint32_t tcb_be32(uint32_t x) { return __builtin_bswap32(x); }

/* cnet_tcp_input from :3425 to the end of the header-prediction tests for one
 * segment: e = the PCB's image entry, (seq, ack, wnd, len, flags, offset) the
 * segment record, w = the TCB_OPT_WORDS little-endian words that start at the
 * first option byte (read only when offset > 20).  o = struct cndp_tcp_opt as
 * four words.  Returns the verdict, CNDP_TCPSEG_TS_UPDATE included. */
static inline PCB_HD uint32_t tcb_segment(const uint32_t *e, uint32_t seq, uint32_t ack, uint32_t wnd, uint32_t len,
                                          uint32_t flags, uint32_t offset, const uint32_t *w, uint32_t now,
                                          uint32_t *o)
{
    o[0] = o[1] = o[2] = o[3] = 0;
    if (!(e[10] & TCB_PRESENT))
        return CNDP_TCPSEG_RESET;
    const uint32_t state = (e[9] >> 16) & 0xffu;
    if (state == CNDP_TCPS_CLOSED)
        return CNDP_TCPSEG_CLOSED;
    if (!(flags & TCB_TCP_SYN))
        wnd <<= (e[9] >> 24) & 31u;
    uint32_t ts_val = 0, ts_ecr = 0, mss = 0, sflags = 0;
    if (offset > TCB_HDR_LEN) { /* tcp_do_options */
        const uint32_t opt_end = offset - TCB_HDR_LEN;
        uint32_t pos = 0;
        while (pos < opt_end) {
            const uint32_t v = tcb_opt_win(w, pos);
            const uint32_t kind = v & 0xffu, olen = (v >> 8) & 0xffu; /* olen may be the byte at opt_end */
            if (kind == 0u)
                break;
            if (kind == 1u) {
                pos++;
                continue;
            }
            if (kind == 2u || kind == 3u || kind == 4u || kind == 8u) {
                if (pos + olen > opt_end)
                    return CNDP_TCPSEG_BADOPT;
                if (kind == 2u) {
                    if (olen == 4u && (flags & TCB_TCP_SYN)) {
                        const uint32_t m = ((v >> 8) & 0xff00u) | (v >> 24), mm = e[9] & 0xffffu;
                        mss = m > mm ? mm : m;
                        sflags |= CNDP_SEG_MSS_PRESENT;
                    }
                } else if (kind == 3u) {
                    if (olen == 3u && (flags & TCB_TCP_SYN)) {
                        const uint32_t sc = (v >> 16) & 0xffu;
                        sflags = (sflags & ~CNDP_SEG_REQ_SCALE) | (sc > 14u ? 14u : sc) | CNDP_SEG_WS_PRESENT;
                    }
                } else if (kind == 4u) {
                    if (olen == 2u)
                        sflags |= CNDP_SEG_SACK_PERMIT;
                } else if (olen == 10u) {
                    ts_val = tcb_be32(tcb_opt_win(w, pos + 2u));
                    ts_ecr = (flags & TCB_TCP_ACK) ? tcb_be32(tcb_opt_win(w, pos + 6u)) : 0u;
                    sflags |= CNDP_SEG_TS_PRESENT;
                    if (ts_ecr != 0u && (int32_t)(now - ts_ecr) < 0)
                        ts_ecr = 0u;
                }
            }
            if (olen == 0u)
                return CNDP_TCPSEG_BADOPT;
            pos += olen;
        }
    }
    o[0] = ts_val;
    o[1] = ts_ecr;
    o[2] = wnd;
    o[3] = mss | sflags << 16;
    const uint32_t ts = sflags & CNDP_SEG_TS_PRESENT;
    if (!(state == CNDP_TCPS_ESTABLISHED && (flags & TCB_HDR_PREDIC) == TCB_TCP_ACK &&
          (!ts || (int32_t)(ts_val - e[6]) >= 0) && seq == e[0] && wnd != 0u && wnd == e[4] && e[2] == e[3]))
        return CNDP_TCPSEG_SLOW;
    uint32_t v = CNDP_TCPSEG_PRED_NONE;
    if (ts && (int32_t)(ts_val - e[6]) <= 0 && (int32_t)(e[7] - seq) < 0)
        v |= CNDP_TCPSEG_TS_UPDATE;
    if (len == 0u) {
        if ((int32_t)(ack - e[1]) > 0 && (int32_t)(ack - e[3]) <= 0 && e[5] >= e[4])
            v ^= CNDP_TCPSEG_PRED_NONE ^ CNDP_TCPSEG_PRED_ACK;
    } else if (ack == e[1] && (e[10] & CNDP_TCB_REASS_EMPTY) && len <= e[8])
        v ^= CNDP_TCPSEG_PRED_NONE ^ CNDP_TCPSEG_PRED_DATA;
    return v;
}

/* ---- cndp_mqtcb.h: which mbufs of the queue's CNDP_MQ_TCP_SEGMENT mode are judged */

/* Step 11 from the mbuf's final edge and record, as pcb_tcp_apply left them:
 * poll (cndp_gpu.hip) and the twin (tcb.c).  A record that stands has a header
 * offset of 20 or more; the zeroed one of an IPOPT mbuf has none. */
static inline int tcb_mq_judged(uint32_t edge, const struct cndp_tcp_seg *seg)
{
    return (edge & CNDP_MQ_EDGE_TCP_MASK) == PCB_TCP_E(CNDP_TCP_INPUT_SEGMENT) && seg->offset != 0u;
}

/* What the lcore knows at submit and the device does not (pcb_tcp_apply's tests on
 * the metadata hook and the mbuf's lengths): the mode's fill sets these in the
 * frame word, bits 40-42. */
#define TCB_MQ_NOMD 1u   /* step 1: metadata(m) == NULL */
#define TCB_MQ_ADJUST 2u /* step 7: l3_len == 20 and pktmbuf_adjust fails */
#define TCB_MQ_SHORT 4u  /* step 8: l3_len == 20 and rx_short */

static inline uint32_t tcb_mq_host_bits(int nomd, uint32_t l3, uint32_t doff, uint32_t blen, uint32_t dlen)
{
    uint32_t b = nomd ? TCB_MQ_NOMD : 0u;
    if (l3 == 20u) {
        if (l3 > dlen || l3 + doff > blen)
            b |= TCB_MQ_ADJUST;
        else if (dlen - l3 < 20u)
            b |= TCB_MQ_SHORT;
    }
    return b;
}

/* The same decision on the device, before poll has run: edge = pcb_tcp_rule's with
 * the verify's verdict in, bits = the lcore's, offset / tot the header's.  rx_badoff
 * drops an l3_len == 20 mbuf and zeroes the record of every other. */
static inline PCB_HD int tcb_mq_judged_dev(uint32_t edge, uint32_t bits, uint32_t offset, uint32_t tot)
{
    return edge == PCB_TCP_E(CNDP_TCP_INPUT_SEGMENT) && !bits && offset >= 20u && offset <= tot;
}

#ifdef __cplusplus
}
#endif
#endif

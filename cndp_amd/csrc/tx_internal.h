/* The transmit stage behind include/cndp_tx.h and include/cndp_mqtx.h, shared by
 * tx.c (host, plain C), cndp_tx.hip (the device mirrors) and the mbuf queue's
 * CNDP_MQ_IP4_OUTPUT mode in cndp_gpu.hip. */
#ifndef CNDP_TX_INTERNAL_H
#define CNDP_TX_INTERNAL_H

#include <string.h>

#include "../../include/cndp_tx.h"
#include "../../include/cndp_mqtx.h"
#include "fwd_internal.h"
#include "pcb_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Transmit image of a PCB table (u32 words), rebuilt by tx_pcb_image() when the
 * table changed:
 *   [0] n (the vector's length)  [1] [2] [3] 0
 *   word[n]: TXW_LIVE | TXW_CKSUM (CNDP_UDP_CHKSUM_FLAG) | tos << 16 | ttl << 8 | ip_proto
 * A deleted entry's word is 0.  4 + 4096 words = 16400 bytes at most. */
#define TXI_HDR 4u
#define TXW_LIVE 0x80000000u
#define TXW_CKSUM 0x01000000u
#define TXI_WORDS(n) (TXI_HDR + (size_t)(n))

#define TX_TTL_DEFAULT 64u /* cnet_ipv4.h:32-33 */
#define TX_TOS_DEFAULT 0u

/* Call with tbl->lock held: bring tbl->ximg up to date.  0 or -ENOMEM. */
int tx_pcb_image(struct cndp_pcb_tbl *tbl);

/* Call with ft->lock held: the host counters as the last GPU call left them. */
int tx_ident_current(struct cndp_fwd_tbl *ft);

/* how far a frame gets (the batch stage keeps it as the high byte of a frame's state) */
#define TXS_NONE 0u         /* not taken */
#define TXS_DROP_NOUDP 1u   /* udp_output's adjust failed: nothing written */
#define TXS_DROP_UDP 2u     /* the IPv4 prepend failed: the UDP header is written */
#define TXS_DROP_NOROUTE 3u /* no route to the source: the IPv4 header is written too */
#define TXS_DROP_IP 4u      /* the Ethernet prepend failed: the same bytes */
#define TXS_OUT 5u          /* ip4_output.c:93-100 ran: s_addr, type, packet_id, hdr_checksum */
#define TXS_NOMD 6u         /* over mbufs only (cndp_mqtx.h): the metadata hook answered NULL */

/* ---- udp_output + ip4_output per mbuf (cndp_mqtx.h): the text the queue's
 * kernels (k_mq_tx_resolve / k_mq_tx_write, cndp_gpu.hip), cndp_gpu_mq_poll and
 * the host twin cndp_ip4_output_node_host all compile ----------------------- */
#if defined(__HIPCC__)
#define TX_HD __host__ __device__
#else
#define TX_HD
#endif

#define TX_IMG_END(mode) ((mode) == CNDP_TX_UDP ? 42u : 34u) /* header bytes in front of mtod at submit */
#define TX_ROUTE 0xFFu /* tx_reach_front: the headroom holds the IPv4 header; the route decides */

/* How far the mbuf gets before the route is looked up: w its PCB's transmit word
 * (0: none), H its data_off at submit. */
static inline TX_HD uint32_t tx_reach_front(uint32_t w, uint32_t nomd, uint32_t mode, uint32_t H)
{
    if (!(w & TXW_LIVE))
        return TXS_NONE;
    if (nomd)
        return TXS_NOMD;
    if (mode == CNDP_TX_UDP) {
        if (H < 8u)
            return TXS_DROP_NOUDP;
        H -= 8u;
    }
    return H < 20u ? TXS_DROP_UDP : TX_ROUTE;
}

/* ... and once it is: rw the route object's second word (0: no object) */
static inline TX_HD uint32_t tx_reach_route(uint32_t rw, uint32_t mode, uint32_t H)
{
    if (!(rw & FWD_SET))
        return TXS_DROP_NOROUTE;
    return H < TX_IMG_END(mode) ? TXS_DROP_IP : TXS_OUT;
}

/* total_length of the frame (uint16_t arithmetic) and what it adds to its netif's
 * ip_ident: the field as a little-endian host loads it */
static inline TX_HD uint32_t tx_total(uint32_t mode, uint32_t dlen) { return (dlen + (mode == CNDP_TX_UDP ? 28u : 20u)) & 0xffffu; }
static inline TX_HD uint32_t tx_step(uint32_t total) { return ((total & 0xffu) << 8) | (total >> 8); }

/* The bytes the rule has written when the frame stops at `st` with ip4_output's
 * edge `edge`, as indices into the header image whose byte 0 is where the
 * Ethernet header starts (or would) and whose end, TX_IMG_END, is mtod at submit:
 * [*s, *e) except [*hs, *he) (packet_id, not written before the route is known). */
static inline TX_HD void tx_written(uint32_t mode, uint32_t st, uint32_t edge, int *s, int *e, int *hs, int *he)
{
    *s = *e = *hs = *he = 0;
    if (st == TXS_DROP_UDP) {
        *s = 34;
        *e = (int)TX_IMG_END(mode);
    } else if (st == TXS_DROP_NOROUTE || st == TXS_DROP_IP) {
        *s = 14;
        *e = (int)TX_IMG_END(mode);
        *hs = 18;
        *he = 20;
    } else if (st == TXS_OUT) {
        *s = edge >= CNDP_TX_EDGE_OUTPUT ? 0 : 6;
        *e = (int)TX_IMG_END(mode);
    }
}

/* the queue's edge: ip4_output's own, a drop's cause, the checksum flag */
static inline TX_HD uint32_t tx_mq_edge(uint32_t st, uint32_t edge, uint32_t proto_drop, uint32_t cksum)
{
    uint32_t cause = 0;
    if (st == TXS_NONE)
        return CNDP_TX_EDGE_NONE;
    if (st == TXS_NOMD)
        cause = CNDP_MQ_TX_CAUSE_NOMD;
    else if (st == TXS_DROP_NOROUTE)
        cause = CNDP_MQ_TX_CAUSE_NOROUTE;
    else if (st != TXS_OUT)
        cause = CNDP_MQ_TX_CAUSE_HEADROOM;
    else if (proto_drop)
        cause = CNDP_MQ_TX_CAUSE_PROTO;
    return edge | cause << 9 | (cksum ? CNDP_MQ_EDGE_TX_CKSUM : 0u);
}

/* the CNDP_MQ_STAT_TX_* key of an edge that is not CNDP_MQ_EDGE_NONE */
static inline int tx_mq_stat_key(uint32_t e)
{
    const uint32_t own = e & CNDP_MQ_EDGE_TX_MASK;
    if (own >= CNDP_TX_EDGE_OUTPUT)
        return CNDP_MQ_STAT_TX_SENT;
    if (own == CNDP_TX_EDGE_ARP_REQUEST)
        return CNDP_MQ_STAT_TX_ARP_REQUEST;
    return CNDP_MQ_STAT_TX_DROP_NOMD + (int)CNDP_MQ_EDGE_TX_CAUSE(e) - 1;
}

/* The sum of the UDP header udp_output wrote, as far as l4_len bytes reach into
 * it: its little-endian 16-bit words (a last odd byte as a low byte).  U0 / U1
 * are the header's two dwords as loaded. */
static inline TX_HD uint32_t tx_udp_hdr_sum(uint32_t U0, uint32_t U1, uint32_t l4_len)
{
    uint64_t v = (uint64_t)U0 | (uint64_t)U1 << 32;
    if (l4_len < 8u)
        v &= l4_len ? ~0ull >> (8u * (8u - l4_len)) : 0ull;
    return (uint32_t)(v & 0xffffu) + (uint32_t)((v >> 16) & 0xffffu) + (uint32_t)((v >> 32) & 0xffffu) +
           (uint32_t)(v >> 48);
}

static inline TX_HD uint32_t tx_reduce16(uint32_t s) /* __cne_raw_cksum_reduce */
{
    s = (s >> 16) + (s & 0xffffu);
    s = (s >> 16) + (s & 0xffffu);
    return s & 0xffffu;
}

/* cne_ipv4_udptcp_cksum's folds (net/cne_ip.h:275-325) once the L4 bytes are
 * summed: S their little-endian 16-bit words' sum, src / dst as loaded */
static inline TX_HD uint32_t tx_l4_cksum(uint32_t S, uint32_t total, uint32_t proto, uint32_t src, uint32_t dst)
{
    uint32_t c = 0;
    if (total >= 20u) {
        const uint32_t l4_len = total - 20u;
        const uint32_t ph = (src & 0xffffu) + (src >> 16) + (dst & 0xffffu) + (dst >> 16) + (proto << 8) +
                            tx_step(l4_len);
        c = tx_reduce16(S) + tx_reduce16(ph);
        c = ((c >> 16) + (c & 0xffffu)) & 0xffffu;
    }
    c = ~c & 0xffffu;
    if (c == 0 && proto == 17u)
        c = 0xffffu;
    return c;
}

#define TX_MB_DATA_OFF 24
#define TX_MB_DATA_LEN 30
#define TX_MB_TX_OFFLOAD 40

/* The mbuf header edits of a frame that stopped at `st` (not TXS_NONE): the twin
 * makes them as it goes, cndp_gpu_mq_poll from the device's record. */
static inline void tx_mbuf_apply(uint8_t *m, uint32_t mode, uint32_t st)
{
    if (st == TXS_NOMD)
        return;
    uint64_t txo;
    uint16_t doff, dlen;
    memcpy(&txo, m + TX_MB_TX_OFFLOAD, 8);
    memcpy(&doff, m + TX_MB_DATA_OFF, 2);
    memcpy(&dlen, m + TX_MB_DATA_LEN, 2);
    uint32_t pre = 0;
    if (mode == CNDP_TX_UDP) {
        txo = 0; /* udp_output.c:46-47 */
        if (st != TXS_DROP_NOUDP)
            pre = 8;
    }
    if (st != TXS_DROP_NOUDP) {
        txo = (txo & ~(0x1ffull << 7)) | 20ull << 7; /* l3_len, before the prepend */
        if (st != TXS_DROP_UDP) {
            pre += 20;
            if (st != TXS_DROP_NOROUTE) {
                txo = (txo & ~0x7full) | 14ull; /* l2_len, before the prepend */
                if (st != TXS_DROP_IP)
                    pre += 14;
            }
        }
    }
    doff = (uint16_t)(doff - pre);
    dlen = (uint16_t)(dlen + pre);
    memcpy(m + TX_MB_TX_OFFLOAD, &txo, 8);
    memcpy(m + TX_MB_DATA_OFF, &doff, 2);
    memcpy(m + TX_MB_DATA_LEN, &dlen, 2);
}

/* Readers of the transmit stage's device state (cndp_tx.hip): cndp_gpu_ip4_output
 * and the mbuf queue's CNDP_MQ_IP4_OUTPUT kernels in cndp_gpu.hip.  tx_dev_begin
 * takes ft->lock and pt->lock, binds both tables to device `dev` (-EINVAL when
 * one is bound to another), orders `stream` after the last reader when that was
 * on another stream, brings both images and the counters' device copy up to date
 * (a copy is waited for, so the tables may change once the locks are dropped),
 * syncs both FIB mirrors and takes a view of each.  On 0 the locks and views are
 * held until tx_dev_end; on an error nothing is.  The counters are 256 uint16_t
 * at ident_in; a launch may advance them there (TX_DEV_INPLACE) or leave the new
 * ones at ident_out (TX_DEV_MOVED), where no launch enqueued before reads.
 * tx_dev_end drops the views, and when launched records the reader's end on
 * `stream`, makes the device counters the authoritative ones, and drops the
 * locks. */
struct tx_dev_view {
    const uint32_t *ximg; /* the PCB table's transmit image */
    const uint32_t *img;  /* the forwarding table's object image (fwd_internal.h) */
    struct fwd_fibv arp, rt;
    uint16_t *ident_in, *ident_out;
    int cus;
};
#define TX_DEV_NONE 0    /* the launch was given up */
#define TX_DEV_INPLACE 1
#define TX_DEV_MOVED 2
int tx_dev_begin(struct cndp_fwd_tbl *ft, struct cndp_pcb_tbl *pt, int dev, void *stream, struct tx_dev_view *v);
int tx_dev_end(struct cndp_fwd_tbl *ft, struct cndp_pcb_tbl *pt, void *stream, int launched);
/* -EINVAL when a table's transmit mirror lives on another device than `dev`, else 0 */
int tx_dev_check(struct cndp_fwd_tbl *ft, struct cndp_pcb_tbl *pt, int dev);

#ifdef __cplusplus
}
#endif
#endif

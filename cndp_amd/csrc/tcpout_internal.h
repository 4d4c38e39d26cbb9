/* TCP transmit behind include/cndp_tcpout.h: the PCB key image and the per-frame
 * rule of tcpout.c (host, plain C), kept apart from it and callable from device
 * code (PCB_HD) as tcb_internal.h's rule is, so that a device stage applies the
 * same statement of it. */
#ifndef CNDP_TCPOUT_INTERNAL_H
#define CNDP_TCPOUT_INTERNAL_H

#include "../../include/cndp_tcpout.h"
#include "tcb_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Key image: TOK_WORDS u32 words per PCB index, rebuilt by tcpout_key_image()
 * when the PCB table changed:
 *   [0] laddr  [1] faddr  [2] fport | lport << 16  [3] TOK_LIVE
 * A deleted entry and an index past the vector are all zero.  The transmit
 * attributes ride in word 11 of the TCB image (tcb_internal.h). */
#define TOK_WORDS 4u
#define TOK_LIVE 1u

/* Call with t->lock held: bring t->kimg up to date.  0 or -ENOMEM. */
int tcpout_key_image(struct cndp_tcb_tbl *t);

#define TOUT_FIN 0x01u
#define TOUT_SYN 0x02u
#define TOUT_RST 0x04u
#define TOUT_ACK 0x10u
#define TOUT_MAXWIN 65535u /* TCP_MAXWIN = ETHER_MAX_MTU, cnet_tcp.h:220-222 */
#define TOUT_HDR 26u       /* the TCP header's offset from H */
#define TOUT_PAY 46u       /* the payload's offset from H, before optlen */
#define TOUT_WORDS 10u     /* 20 header bytes and up to 20 option bytes */

static inline PCB_HD uint32_t tout_be32(uint32_t x) { return __builtin_bswap32(x); }
static inline PCB_HD uint32_t tout_be16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

#define TOUT_O_MSS 1u
#define TOUT_O_WS 2u
#define TOUT_O_TS 4u
/* Which options tcp_send_options writes (:3742-3798): tf = CNDP_TCBF_*, fl = the TCP flags. */
static inline PCB_HD uint32_t tout_opt_mask(uint32_t tf, uint32_t fl)
{
    uint32_t m = 0;
    if (fl & TOUT_SYN) {
        m = TOUT_O_MSS;
        if ((tf & CNDP_TCBF_REQ_SCALE) && (!(fl & TOUT_ACK) || (tf & CNDP_TCBF_RCVD_SCALE)))
            m |= TOUT_O_WS;
    }
    if ((tf & CNDP_TCBF_REQ_TSTAMP) && !(fl & TOUT_RST) &&
        ((fl & (TOUT_SYN | TOUT_ACK)) == TOUT_SYN || (tf & CNDP_TCBF_RCVD_TSTAMP)))
        m |= TOUT_O_TS;
    return m;
}
static inline PCB_HD uint32_t tout_optlen(uint32_t tf, uint32_t fl)
{
    const uint32_t m = tout_opt_mask(tf, fl);
    return ((m & TOUT_O_MSS) ? 4u : 0u) + ((m & TOUT_O_WS) ? 4u : 0u) + ((m & TOUT_O_TS) ? 12u : 0u);
}

/* tcp_send_options: the option bytes as little-endian words o[0..4] (unused ones
 * zero) for TCB image entry e (no TCB: no options).  Returns optlen.  The
 * timestamp's three words land at word 0, 1 or 2; written as selects over
 * constant indices, so that device code can keep o in registers. */
static inline PCB_HD uint32_t tout_options(const uint32_t *e, uint32_t fl, uint32_t now, uint32_t *o)
{
    o[0] = o[1] = o[2] = o[3] = o[4] = 0;
    if (!(e[10] & TCB_PRESENT))
        return 0;
    const uint32_t m = tout_opt_mask(e[11] & 0xffu, fl);
    uint32_t k = 0;
    if (m & TOUT_O_MSS) {
        const uint32_t mss = e[9] & 0xffffu;
        o[0] = 0x0402u | (mss >> 8) << 16 | (mss & 0xffu) << 24; /* MSS, 4, high byte, low byte */
        k = 1;
    }
    if (m & TOUT_O_WS) {
        o[1] = 0x0303u | ((e[11] >> 8) & 0xffu) << 16 | 0x01u << 24; /* WS, 3, req_recv_scale, NOP */
        k = 2;
    }
    if (m & TOUT_O_TS) {
        const uint32_t t0 = 0x0a080101u, t1 = tout_be32(now), t2 = tout_be32(e[6]); /* NOP NOP TS 10 */
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < 5u; j++)
            o[j] = j == k ? t0 : j == k + 1u ? t1 : j == k + 2u ? t2 : o[j];
        k += 3u;
    }
    return 4u * k;
}

/* The 20-byte header of :397-485 / :1061-1079 as little-endian words w[0..4]:
 * k = the PCB's key image entry, wnd and urp host order, checksum 0. */
static inline PCB_HD void tout_header(const uint32_t *k, uint32_t seq, uint32_t ack, uint32_t fl, uint32_t wnd,
                                      uint32_t urp, uint32_t optlen, uint32_t *w)
{
    w[0] = k[2] >> 16 | k[2] << 16; /* src_port = lport, dst_port = fport */
    w[1] = tout_be32(seq);
    w[2] = tout_be32(ack);
    w[3] = (((20u + optlen) >> 2) << 4) | (fl & 0xffu) << 8 | tout_be16(wnd & 0xffffu) << 16;
    w[4] = tout_be16(urp & 0xffffu) << 16;
}

/* What happens to one candidate frame.  k = key image entry, e = TCB image entry
 * (both all zero for an index outside the table), r = the frame's 16-byte record
 * as four words: struct cndp_tcp_txseg (SEGMENT, or RESPOND with `desc`) or struct
 * cndp_tcp_seg.  mc = a multicast test held (RESPOND from a segment).  On
 * CNDP_TCPOUT_STAT_SENT: w[0..4] the header, w[5..9] the options, *optlen, *plen
 * (payload bytes; 0 in RESPOND).  Any other return: the frame is not taken. */
static inline PCB_HD uint32_t tout_frame(uint32_t mode, int desc, const uint32_t *k, const uint32_t *e,
                                         const uint32_t *r, int mc, uint32_t now, uint32_t *w, uint32_t *optlen,
                                         uint32_t *plen)
{
    *optlen = *plen = 0;
    if (!(k[3] & TOK_LIVE))
        return CNDP_TCPOUT_STAT_NOPCB;
    const uint32_t fl_in = (r[3] >> 16) & 0xffu;
    if (mode == CNDP_TCPOUT_SEGMENT) {
        if (!(e[10] & TCB_PRESENT))
            return CNDP_TCPOUT_STAT_NOPCB;
        if (k[0] == 0u)
            return CNDP_TCPOUT_STAT_NOLADDR;
        const uint32_t ol = tout_options(e, fl_in, now, w + 5), len = r[3] & 0xffffu;
        if ((int32_t)len > (int32_t)(e[9] & 0xffffu) - (int32_t)ol)
            return CNDP_TCPOUT_STAT_TOOBIG;
        tout_header(k, r[0], r[1], fl_in, r[2] & 0xffffu, r[2] >> 16, ol, w);
        *optlen = ol;
        *plen = len;
        return CNDP_TCPOUT_STAT_SENT;
    }
    uint32_t seq = r[0], ack = r[1], fl = fl_in;
    if (!desc) { /* tcp_drop_with_reset */
        if (fl_in & TOUT_RST)
            return CNDP_TCPOUT_STAT_RST_IN;
        if (mc)
            return CNDP_TCPOUT_STAT_MCAST;
        if (fl_in & TOUT_ACK) {
            seq = r[1];
            ack = 0;
            fl = TOUT_RST;
        } else {
            uint32_t len = r[3] & 0xffffu;
            if (fl_in & TOUT_SYN)
                len = (len + 1u) & 0xffffu; /* seg->len++, a uint16_t */
            seq = 0;
            ack = len; /* seg->seq + seg->len after seg->seq = 0 */
            fl = TOUT_RST | TOUT_ACK;
        }
    }
    const uint32_t ol = tout_options(e, fl, now, w + 5);
    uint32_t wnd = 0;
    if ((e[10] & TCB_PRESENT) && !(fl & TOUT_RST)) {
        const uint32_t sc = (e[11] >> 16) & 31u, lim = TOUT_MAXWIN << sc;
        wnd = ((e[8] > lim ? lim : e[8]) >> sc) & 0xffffu;
    }
    tout_header(k, seq, ack, fl, wnd, 0, ol, w);
    *optlen = ol;
    return CNDP_TCPOUT_STAT_SENT;
}

/* is_multicast() (:231-245) on ip->dst_addr as a little-endian host loads it */
static inline PCB_HD int tout_ip_mcast(uint32_t dst_loaded) { return dst_loaded >= 0xE0000000u && dst_loaded <= 0xEFFFFFFFu; }

#ifdef __cplusplus
}
#endif
#endif

/*
 * cndp_tcpout.h -- TCP transmit: the part of the cnet TCP output path that builds
 * the L4 header of an outgoing frame (CNDP v25.08.0, lib/cnet/tcp/cnet_tcp.c):
 *
 *   tcp_send_options     :3742-3798   MSS only with SYN; WS + NOP with SYN when
 *                        TCBF_REQ_SCALE is set and (ACK is clear or TCBF_RCVD_SCALE
 *                        is set); NOP NOP TS(now, ts_recent) when TCBF_REQ_TSTAMP is
 *                        set, RST is clear and ((flags & SYN_ACK) == SYN or
 *                        TCBF_RCVD_TSTAMP is set).  0, 4, 8, 12, 16 or 20 bytes.
 *   tcp_output's mbuf build, :836-870: the TOOBIG clamp test, the data_off move,
 *                        the memset, tcp_mbuf_copydata.
 *   tcp_send_segment     :371-517     the options and the 20-byte header in front
 *                        of the payload, md->faddr / md->laddr from the PCB key.
 *   tcp_drop_with_reset  :1120-1149   and
 *   tcp_do_response      :1020-1108   the reply to a segment, in the mbuf it came in.
 *
 * The stage sits between the host's tcp_output decisions (which segment, which
 * seq / ack / window / flags: struct cndp_tcp_txseg) and
 * cndp_gpu_ip4_output(..., CNDP_TX_IP4, ...) of cndp_tx.h, which writes IPv4 and
 * Ethernet in front of the header built here and generates the TCP checksum.
 * This build runs the rule on the calling thread only (cndp_tcp_output_host); it
 * has no device stage, so a device-resident batch takes a host round trip here.
 *
 * Where the header starts.  H = data_off is a fresh mbuf's data_off.
 * tcp_output moves data_off forward by sizeof(struct cne_tcp_hdr) + optlen +
 * iphdr_len + sizeof(struct ether_addr) (:858-859; tcp_do_response the same,
 * :1046-1050).  The last term is the 6-byte address, not the 14-byte Ethernet
 * header, so for IPv4 the move is 46 + optlen and the payload starts at
 * P = H + 46 + optlen.  tcp_send_segment then prepends optlen (:387) and 20
 * (:390): the options start at H + 46 and the TCP header at H + 26 for EVERY
 * frame, whatever its options.  The follow-on cndp_gpu_ip4_output call therefore
 * takes one data_off for the whole batch, H + 26, and `len` as returned here.
 * (ip4_output's own prepends need 34 bytes: a caller keeps H >= 8.)
 *
 * CNDP_TCPOUT_SEGMENT, per taken frame, in the reference's order of effects:
 *   optlen = tcp_send_options; the memset of :862-863 -- made AFTER data_off has
 *   moved, so it clears 46 + optlen bytes starting at P: the payload area, not the
 *   header area; the payload copy to P; the options at H + 46; the header of
 *   :397-485 at H + 26: ports from the PCB key, data_off = ((20 + optlen) >> 2)
 *   << 4, checksum 0, the rest from the descriptor.  So the bytes [P + len,
 *   P + 46 + optlen) of a short segment end up zero and [H, H + 26) is not
 *   written.
 * CNDP_TCPOUT_RESPOND, per taken frame:
 *   tcp_drop_with_reset: nothing for a segment with RST, a multicast
 *   destination or a multicast / broadcast frame (below); with ACK, <SEQ=SEG.ACK>
 *   <CTL=RST>; without, seg->len++ when SYN is set -- although seg->len already
 *   counts the SYN (cnet_tcp.c:3414), in uint16_t -- then seg->seq = 0 and
 *   <SEQ=0><ACK=seg->seq + seg->len><CTL=RST,ACK>: seg->seq is zeroed BEFORE the
 *   sum, so the ACK number is SEG.LEN (+ 1), not SEG.SEQ + SEG.LEN.
 *   tcp_do_response: pktmbuf_reset puts data_off back to H; options from
 *   tcp_send_options; header and options zeroed (:1061), then written; addresses
 *   AND ports from the PCB key, not from the frame, so the reply for a wildcard
 *   PCB goes where its key says (address 0, port 0); rx_win of :1087-1094 only
 *   with a TCB and without RST: min(rcv_space, TCP_MAXWIN << rcv_scale) >>
 *   rcv_scale, TCP_MAXWIN = 65535.  len out is 20 + optlen; nothing but
 *   [H + 26, H + 46 + optlen) is written, so the slab may be the receive slab.
 *   With io->txseg given instead of io->seg the stage is tcp_do_response alone, as
 *   tcp_send_ack and its kin call it: seq, ack and flags from the descriptor (its
 *   wnd, urp and len are not read), and `sel` is required.
 *   The multicast tests: is_multicast() compares ip->dst_addr AS LOADED (network
 *   order on a little-endian host) with the host-order range 224.0.0.0 -
 *   239.255.255.255, so it looks at the address's LAST byte; CNE_MBUF_IS_MCAST is
 *   what eth_rx.c:50-53 left in ol_flags, the group bit of the destination MAC.
 *   Both are answered from the frame when io->rxmeta is given (the frame at
 *   H, its IPv4 header at H + l2_len); without it the slab is taken not to hold the
 *   received frame and neither test is made.
 *
 * Not modelled:
 *  - every side effect on the TCB: tflags (ACK_NOW, DELAYED_ACK, FORCE_TX),
 *    last_ack_sent, snd_nxt = snd_iss on SYN.  The stage writes no TCB, as
 *    cndp_gpu_tcp_segment does not; the host applies them.
 *  - tcp_output's decision logic, the sendalot loop, timers, and the IPv6 branches;
 *  - the mbuf's bookkeeping (data_off, data_len, l4_len, userptr) and a chained
 *    send buffer: tcp_mbuf_copydata is one contiguous source region here;
 *  - pcb->ch == NULL and netif == NULL in tcp_do_response.
 * Where the reference faults or lacks the input this build defines:
 *  - RESPOND for a PCB without a TCB (the reference passes a NULL tcb into
 *    tcp_send_options): no options, window 0;
 *  - SEGMENT with laddr == 0 in the PCB key (the cnet_netif_match_subnet branch,
 *    :438-469, rewrites the PCB): the frame is not taken and counted under
 *    NOLADDR; the host resolves the address first.  RESPOND has no such branch and
 *    replies from address 0;
 *  - a descriptor with len > max_mss - optlen (int arithmetic, :838): not taken,
 *    counted under TOOBIG.  The host's loop clamps and sets sendalot;
 *    cndp_tcp_send_optlen gives it optlen;
 *  - a pcb[i] that is CNDP_PCB_NONE, at or past the vector's length, deleted or, in
 *    SEGMENT mode, without a TCB: not taken, counted under NOPCB;
 *  - rcv_scale above TCP_MAX_WINSHIFT (14) shifts an int past its width in the
 *    reference: the shift count is rcv_scale & 31 in 32-bit unsigned arithmetic;
 *  - bytes at or past slab + slab_len are never written (and read as zero); snd
 *    bytes at or past snd_len read as zero;
 *  - a frame that is not taken gets len = 0, taken = 0, faddr = laddr = 0, and its
 *    slot is untouched.
 * Errors are negative errno values.
 */
#ifndef CNDP_TCPOUT_H
#define CNDP_TCPOUT_H

#include <stdint.h>

#include "cndp_tcb.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tcb_entry.tflags bits tcp_send_options reads (cnet_tcp.h:420-428) */
#define CNDP_TCBF_REQ_SCALE 0x01u   /* TCBF_REQ_SCALE   */
#define CNDP_TCBF_RCVD_SCALE 0x02u  /* TCBF_RCVD_SCALE  */
#define CNDP_TCBF_REQ_TSTAMP 0x04u  /* TCBF_REQ_TSTAMP  */
#define CNDP_TCBF_RCVD_TSTAMP 0x08u /* TCBF_RCVD_TSTAMP */

/* What the transmit side reads of a struct tcb_entry beyond struct cndp_tcb
 * (max_mss, ts_recent and rcv_space come from that snapshot).  A freshly set TCB
 * has all-zero attributes; cndp_tcb_set on an index that already has a TCB keeps
 * them; cndp_tcb_clear and a PCB delete take them away. */
struct cndp_tcb_tx {
    uint8_t tflags;         /* CNDP_TCBF_*; other bits are not kept */
    uint8_t req_recv_scale; /* cnet_tcp.h:365 */
    uint8_t rcv_scale;      /* cnet_tcp.h:364 */
    uint8_t rsvd;           /* not kept */
};
/* -EINVAL / -ENOENT as cndp_tcb_set / cndp_tcb_get; -ENOENT also for an index
 * that has no TCB. */
int cndp_tcb_tx_set(cndp_tcb_tbl_t *t, uint32_t idx, const struct cndp_tcb_tx *a);
int cndp_tcb_tx_get(cndp_tcb_tbl_t *t, uint32_t idx, struct cndp_tcb_tx *a);

#define CNDP_TCPOUT_SEGMENT 0u /* tcp_output's mbuf build + tcp_send_segment, from descriptors */
#define CNDP_TCPOUT_RESPOND 1u /* tcp_drop_with_reset + tcp_do_response, from received segments */

/* What the host's tcp_output decided for one segment, host byte order. */
struct cndp_tcp_txseg {
    uint32_t seq, ack;
    uint16_t wnd, urp; /* wnd already scaled (seg->wnd) */
    uint16_t len;      /* payload bytes */
    uint8_t flags, rsvd;
};

#define CNDP_TCPOUT_STAT_SENT 0    /* taken: a header was written */
#define CNDP_TCPOUT_STAT_NOTSEL 1  /* sel[i] == 0, or (RESPOND, sel == NULL) a verdict other than RESET */
#define CNDP_TCPOUT_STAT_NOPCB 2   /* no such PCB, or (SEGMENT) no TCB */
#define CNDP_TCPOUT_STAT_NOLADDR 3 /* SEGMENT: laddr == 0 in the PCB key */
#define CNDP_TCPOUT_STAT_TOOBIG 4  /* SEGMENT: len > max_mss - optlen */
#define CNDP_TCPOUT_STAT_RST_IN 5  /* RESPOND: the segment has RST set: no reply */
#define CNDP_TCPOUT_STAT_MCAST 6   /* RESPOND: a multicast test held: no reply */
#define CNDP_TCPOUT_STAT_OPTS 7    /* taken frames that carry options (also counted under SENT) */
#define CNDP_TCPOUT_NSTATS 8

/* Arrays of n elements (stats: CNDP_TCPOUT_NSTATS) in host memory.  The inputs
 * are read only.  faddr, laddr, taken and len plug straight into struct cndp_tx_io
 * (faddr, laddr, sel, len). */
struct cndp_tcpout_io {
    const uint8_t *sel;  /* in: frame i is a candidate when sel[i] != 0.  NULL = all (SEGMENT), the
                          * frames whose verdict[i] & CNDP_TCPSEG_VERDICT is CNDP_TCPSEG_RESET (RESPOND) */
    const uint32_t *pcb; /* in, required: the PCB index */
    const struct cndp_tcp_txseg *txseg; /* in, 16-byte aligned: required in SEGMENT; in RESPOND the
                                         * tcp_do_response-alone form (above) */
    const struct cndp_tcp_seg *seg;     /* in, 16-byte aligned, RESPOND without txseg: cndp_gpu_tcp_input's */
    const uint8_t *verdict;             /* in, RESPOND with sel == NULL: cndp_gpu_tcp_segment's */
    const uint32_t *rxmeta;             /* in, optional, RESPOND: the receive batch's rxmeta (multicast tests) */
    const void *snd;         /* in, optional, SEGMENT: the send buffer the payload is gathered from.  NULL =
                              * the application has already put the payload at P */
    uint64_t snd_len;        /* bytes of snd */
    const uint64_t *src_off; /* in, required with snd: frame i's payload starts at snd + src_off[i] */
    uint16_t *len;           /* out, required: data_len for ip4_output: 20 + optlen + payload */
    uint32_t *faddr;         /* out, required: md->faddr / md->laddr from the PCB key, in the form */
    uint32_t *laddr;         /*      cndp_tx_io takes                                              */
    uint8_t *taken;          /* out, required: 1 = a header was written */
    uint64_t *stats;         /* out, optional: [CNDP_TCPOUT_NSTATS], accumulated (+=) */
};

/* The rule on the calling thread over host memory, written IN PLACE into `slab`;
 * io holds host pointers.  The layout is given as for cndp_tx_output_host: slab,
 * slab_len, stride / offsets and data_off = H.  `now` stands for
 * stk_get_timer_ticks().  len, faddr, laddr and taken are written for all n
 * frames.  -EINVAL: a NULL argument, an unknown mode, a missing slab or required
 * array, a txseg or seg that is not 16-byte aligned, a slab_len of 2^63 or more;
 * -ENOMEM. */
int cndp_tcp_output_host(cndp_tcb_tbl_t *t, uint32_t mode, uint32_t now, void *slab, uint64_t slab_len,
                         uint64_t stride, const uint64_t *offsets, uint32_t data_off, uint32_t n,
                         const struct cndp_tcpout_io *io_host);

/* tcp_send_options' length for a TCB with these CNDP_TCBF_* bits and a segment
 * with these TCP flags: 0, 4, 8, 12, 16 or 20.  Pure. */
uint32_t cndp_tcp_send_optlen(uint8_t tcb_tflags, uint8_t seg_flags);

#ifdef __cplusplus
}
#endif
#endif

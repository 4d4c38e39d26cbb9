/*
 * cndp_mqtcp.h -- cnet's tcp_input node (CNDP v25.08.0 built with enable_tcp,
 * lib/cnet/tcp/tcp_input.c:41-119) and the opening of cnet_tcp_input
 * (lib/cnet/tcp/cnet_tcp.c:3329-3414), up to the point where the TCP state
 * machine starts, as a mode of the asynchronous mbuf queue (cndp_gpu_mq_*,
 * cndp_gpu.h), and the same node on the calling thread
 * (cndp_tcp_input_node_host).  Both take pktmbuf_t bursts as ip4_proto hands
 * them to its tcp_input edge (CNDP_MQ_UDP_INPUT's CNDP_IP4_PROTO_TCP edge,
 * cndp_mql4.h) and look them up in a TCP PCB table, a cndp_pcb_tbl_t as
 * cndp_tcp.h uses it.
 *
 * A queue made here is driven by cndp_gpu_mq_submit / _flush / _poll / _wait /
 * _pending / _stat / _free as every other one, and by cndp_gpu_mq_poll_tcp.
 *
 * The mbuf at submit: pktmbuf_mtod is the IPv4 header; tx_offload holds l2_len
 * (bits 0-6), l3_len (bits 7-15) and l4_len (bits 16-23); data_len is whatever
 * it is.  Every submitted mbuf is taken.  Frames are independent: burst
 * boundaries decide nothing.  Per mbuf, in this order:
 *   1. md = metadata(m).  NULL: pkt_drop with nothing written, counted
 *      CNDP_MQ_STAT_TCP_NOMD (tcp_input.c:55-57).
 *   2. The key: faddr / laddr from header bytes 12-19, fport / lport from bytes
 *      0-3 at mtod + l3_len.  md->faddr.cin_port and md->laddr.cin_port are
 *      written now, for every frame that reaches this step (:91-92).
 *   3. The BEST_MATCH lookup in the table's TCP index, exactly
 *      cndp_pcb_lookup_indexed's.  No match: pkt_punt or pkt_drop by the
 *      table's punt flag; m->userptr is not written.
 *   4. cne_ipv4_udptcp_cksum_verify, always, a zero checksum field included,
 *      over total_length - IHL * 4 bytes from mtod + l3_len; total_length below
 *      the IHL fails.  A failure is pkt_drop with CNDP_MQ_EDGE_L4_CKSUM set;
 *      userptr and the mbuf header stay, the ports of step 2 stay written.
 *   5. m->userptr = the PCB's user value (cndp_pcb_user_set, cndp_mql4.h); both
 *      20-byte in_caddr of the metadata become the key's (family AF_INET, len 4,
 *      port, address, then twelve zero bytes).
 *   6. l3_len != 20: see "Defined by this build".
 *   7. pktmbuf_adjust(m, l3_len): it fails when l3_len > data_len or l3_len +
 *      data_off > buf_len; then no header field changes and the edge is
 *      pkt_drop, counted CNDP_MQ_STAT_TCP_ADJUST.  Else data_off += l3_len,
 *      data_len -= l3_len.
 *   8. data_len < 20 now: pkt_drop (rx_short), CNDP_MQ_STAT_TCP_SHORT.  The edit
 *      of step 7 stays.
 *   9. offset = (data_off byte & 0xF0) >> 2; pktmbuf_adj_offset(m, offset),
 *      which changes nothing when offset > data_len or offset + data_off >
 *      buf_len; then rx_badoff: offset < 20 or offset > total_length is
 *      pkt_drop, CNDP_MQ_STAT_TCP_BADOFF -- after the adj_offset has happened.
 *  10. CNDP_TCP_INPUT_SEGMENT, with the frame's struct cndp_tcp_seg (cndp_tcp.h;
 *      len keeps the reference's uint16_t wrap).
 *
 * Edge of each mbuf: CNDP_MQ_EDGE(CNDP_MQ_NODE_TCP_INPUT, e) with e the node's
 * own edge index (tcp_input_priv.h): pkt_drop 0, SEGMENT 1 (the slot of
 * chnl_recv, named as cndp_tcp.h names it and for its reason), pkt_punt 2.
 * (edge & CNDP_MQ_EDGE_TCP_MASK) is the node's own edge.
 *
 * Defined by this build:
 *  - m->userptr at submit is not read; the family is always AF_INET.
 *  - l3_len != 20 (IPv4 options).  The reference's tcp_strip_ip_options is an
 *    overlapping memcpy from odd addresses, so there is nothing well defined to
 *    be exact against.  Here the mbuf comes back as it stood at the call of
 *    cnet_tcp_input: steps 1-5 done and nothing further.  The edge is SEGMENT
 *    with CNDP_MQ_EDGE_TCP_IPOPT set, counted CNDP_MQ_STAT_TCP_IPOPT, and the
 *    record is what cndp_gpu_tcp_input computes for such a frame (all zero when
 *    that stage would call it rx_badoff).  The host's continuation runs its own
 *    cnet_tcp_input on the mbuf.
 *  - The readable bytes of a frame, clipping, bytes that read as zero and
 *    CNDP_MQ_EDGE_NONE for zero-copy mbufs outside every registered region are
 *    cndp_mql4.h's, word for word: readable are [mtod, mtod + data_len),
 *    clipped at buf_addr + buf_len always; at the end of the frame's registered
 *    region for zero-copy; at stage_max bytes from mtod for staged
 *    (conf.stage_max, 0 = 2048).  Bytes past them read as zero.  No frame byte
 *    is ever written.  Zero-copy, an mbuf or a frame's first byte outside every
 *    registered region: the edge is CNDP_MQ_EDGE_NONE, nothing is read or
 *    written, and the mbuf counts nowhere.
 *
 * The device writes neither mbuf headers, nor metadata, nor frames: per mbuf it
 * returns one 32-byte record into pinned memory, and cndp_gpu_mq_poll makes
 * every edit above on the calling lcore, zero-copy and staged alike.  poll also
 * counts the eight keys below; they are exact once cndp_gpu_mq_pending is 0.
 * On a queue of another mode cndp_gpu_mq_stat answers -EINVAL for them.
 */
#ifndef CNDP_MQTCP_H
#define CNDP_MQTCP_H

#include <stdint.h>

#include "cndp_mql4.h"
#include "cndp_tcp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_MQ_TCP_INPUT 9u /* tcp_input_node_process + cnet_tcp_input's opening */
#define CNDP_MQ_NODE_TCP_INPUT 5u
#define CNDP_MQ_EDGE_TCP_IPOPT 0x0040u /* OR-ed into SEGMENT: l3_len != 20, the mbuf as at cnet_tcp_input's call */
#define CNDP_MQ_EDGE_TCP_MASK 0xFF3Fu  /* the node's own edge (CNDP_MQ_EDGE_L4_CKSUM and _TCP_IPOPT removed) */

#define CNDP_MQ_STAT_TCP_SEGMENT 17 /* SEGMENT, l3_len == 20 */
#define CNDP_MQ_STAT_TCP_NOMATCH 18 /* drop or punt: no PCB matched */
#define CNDP_MQ_STAT_TCP_CKSUM 19   /* drop: the checksum verify failed */
#define CNDP_MQ_STAT_TCP_NOMD 20    /* drop: the metadata hook answered NULL */
#define CNDP_MQ_STAT_TCP_ADJUST 21  /* drop: pktmbuf_adjust(m, l3_len) failed */
#define CNDP_MQ_STAT_TCP_SHORT 22   /* drop: rx_short */
#define CNDP_MQ_STAT_TCP_BADOFF 23  /* drop: rx_badoff */
#define CNDP_MQ_STAT_TCP_IPOPT 24   /* SEGMENT | CNDP_MQ_EDGE_TCP_IPOPT */

/* A queue in mode CNDP_MQ_TCP_INPUT over `tbl`, which must outlive it.
 * conf->metadata is pktmbuf_metadata (NULL: m + 64); poll calls it.  Entries,
 * flags and user values changed between batches reach the batches launched
 * after the change.  The queue reads the table's TCP device mirror by the
 * protocol cndp_gpu_tcp_input uses, so both may run on one table.
 * -EINVAL: a NULL argument, another mode, any conf->flags bit, what
 * cndp_gpu_mq_create answers for batch, depth, stage_max and umem, and a table
 * already bound to another device.  cndp_gpu_mq_create, cndp_gpu_mq_create_fwd,
 * cndp_gpu_mq_create_ip4_forward and cndp_gpu_mq_create_udp_input answer
 * -EINVAL for this mode. */
int cndp_gpu_mq_create_tcp_input(cndp_gpu_ctx_t *ctx, const struct cndp_mq_conf *conf,
                                 cndp_pcb_tbl_t *tbl, cndp_gpu_mq_t **out);

/* cndp_gpu_mq_poll, and segs[k] = the record of mbufs[k]: all zero unless
 * edges[k] is SEGMENT (with or without CNDP_MQ_EDGE_TCP_IPOPT).  segs may be
 * NULL.  -EINVAL as cndp_gpu_mq_poll, and on a queue of another mode.  Plain
 * cndp_gpu_mq_poll works on this mode and drops the records; the two may be
 * interleaved. */
int cndp_gpu_mq_poll_tcp(cndp_gpu_mq_t *q, void **mbufs, uint16_t *edges, struct cndp_tcp_seg *segs,
                         uint32_t max);

/* The same node on the calling thread over the table's host image: one burst
 * of n <= 256 mbufs, the same mbuf header and metadata edits, the same edges
 * and records as the queue's.  segs may be NULL.  readable_end, stage_max and
 * metadata as cndp_udp_input_node_host has them (cndp_mql4.h).  -EINVAL: tbl
 * NULL, n above 256, or n != 0 with mbufs or edges NULL; -ENOMEM. */
int cndp_tcp_input_node_host(cndp_pcb_tbl_t *tbl, void *const *mbufs, uint32_t n, uint16_t *edges,
                             struct cndp_tcp_seg *segs, const void *readable_end, uint32_t stage_max,
                             void *(*metadata)(const void *m));

#ifdef __cplusplus
}
#endif
#endif

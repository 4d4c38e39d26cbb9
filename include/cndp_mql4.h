/*
 * cndp_mql4.h -- cnet's UDP socket demux, ip4_proto + udp_input (CNDP v25.08.0,
 * lib/cnet/ipv4/ip4_proto.c:30-195, lib/cnet/udp/udp_input.c:43-123), as a mode
 * of the asynchronous mbuf queue (cndp_gpu_mq_*, cndp_gpu.h), and the same two
 * nodes on the calling thread (cndp_udp_input_node_host).  Both take pktmbuf_t
 * bursts as ip4_input hands them to its proto edge and look them up in a PCB
 * table (cndp_pcb_*, cndp_l4.h).
 *
 * A queue made here is driven by cndp_gpu_mq_submit / _flush / _poll / _wait /
 * _pending / _stat / _free as every other one.
 *
 * The mbuf at submit: pktmbuf_mtod is the IPv4 header; tx_offload holds l2_len
 * (bits 0-6), l3_len (bits 7-15) and l4_len (bits 16-23); data_len is whatever
 * it is (ip4_input left the total length there).  Every submitted mbuf is
 * taken.  Frames are independent: there are no group rules, and burst
 * boundaries decide nothing.  Per mbuf, in this order:
 *   1. ip4_proto on header byte 9: 17 goes on to udp_input; 6 leaves on the
 *      tcp_input edge when the table's TCP flag is set (cndp_pcb_set_flags);
 *      everything else leaves on drop.  Nothing is written for a frame that
 *      stops here.
 *   2. md = metadata(m).  NULL: udp_input's pkt_drop with nothing written,
 *      counted CNDP_MQ_STAT_L4_NOMD (udp_input.c:57-59).
 *   3. The key: faddr / laddr from header bytes 12-19, fport / lport from bytes
 *      0-3 at mtod + l3_len.  md->faddr.cin_port and md->laddr.cin_port are
 *      written now, for every frame that reaches this step (:95-96).
 *   4. The BEST_MATCH lookup, exactly cndp_gpu_udp_input's.  No match:
 *      m->userptr = NULL and the edge is punt or drop by the table's punt flag.
 *   5. The PCB has CNDP_UDP_CHKSUM_FLAG and the UDP checksum field is nonzero:
 *      cne_ipv4_udptcp_cksum_verify over total_length - IHL * 4 bytes from
 *      mtod + l3_len; total_length below the IHL fails.  A failure is pkt_drop
 *      with CNDP_MQ_EDGE_L4_CKSUM set; userptr and the mbuf header stay, the
 *      ports of step 3 stay written.
 *   6. chnl_recv: m->userptr = the PCB's user value (cndp_pcb_user_set); both
 *      20-byte in_caddr of the metadata become the key's (family AF_INET, len 4,
 *      port, address, then twelve zero bytes); pktmbuf_adj_offset(m, l3_len +
 *      l4_len): data_off += len, data_len -= len, both as uint16_t.  If
 *      len > data_len or len + data_off > buf_len no header field changes
 *      (pktmbuf.h:961-971); the edge is still chnl_recv.
 *
 * Edge of each mbuf: CNDP_MQ_EDGE(node, e) with e the node's own edge index --
 * ip4_proto: drop 0, tcp_input 2; udp_input: pkt_drop 0, chnl_recv 1, pkt_punt 2.
 * CNDP_MQ_EDGE_L4_CKSUM is OR-ed into a udp_input drop edge that the checksum
 * verify caused; (edge & CNDP_MQ_EDGE_L4_MASK) is the node's own edge.
 *
 * Defined by this build:
 *  - m->userptr at submit is not read.  The reference derives the address
 *    family from it; the family is always AF_INET here.
 *  - The readable bytes of a frame are [mtod, mtod + data_len), clipped at
 *    buf_addr + buf_len always; at the end of the frame's registered region
 *    for zero-copy; at stage_max bytes from mtod for staged (conf.stage_max,
 *    0 = 2048).  Bytes past the readable bytes read as zero.  No frame byte is
 *    ever written.
 *  - Zero-copy, an mbuf or a frame's first byte outside every registered
 *    region: the edge is CNDP_MQ_EDGE_NONE, nothing is read or written, and the
 *    mbuf counts nowhere.
 *
 * The device writes neither mbuf headers, nor metadata, nor frames: per mbuf it
 * returns one 16-byte record into pinned memory (edge, PCB index, ports, the
 * two addresses), and cndp_gpu_mq_poll makes every edit above on the calling
 * lcore, zero-copy and staged alike -- the shape CNDP_MQ_F_HOST_WRITEBACK gave
 * cnet.  poll also counts the six keys below, from the edges it returns; they
 * are exact once cndp_gpu_mq_pending is 0.  CNDP_MQ_EDGE_NONE mbufs count
 * nowhere and every other family's key reads 0 here.  On a queue of another
 * mode cndp_gpu_mq_stat answers -EINVAL for these six keys, as it did before
 * they existed: keys above 10 were unknown there.
 */
#ifndef CNDP_MQL4_H
#define CNDP_MQL4_H

#include <stdint.h>

#include "cndp_l4.h"
#include "cndp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_MQ_UDP_INPUT 8u /* ip4_proto_node_process + udp_input_node_process */
#define CNDP_MQ_NODE_IP4_PROTO 3u
#define CNDP_MQ_NODE_UDP_INPUT 4u
#define CNDP_MQ_EDGE_L4_CKSUM 0x0080u /* OR-ed into a udp_input drop edge the checksum verify caused */
#define CNDP_MQ_EDGE_L4_MASK 0xFF7Fu  /* the node's own edge */

#define CNDP_MQ_STAT_L4_RECV 11       /* chnl_recv */
#define CNDP_MQ_STAT_L4_NOMATCH 12    /* udp_input drop or punt: no PCB matched */
#define CNDP_MQ_STAT_L4_CKSUM 13      /* udp_input drop: the checksum verify failed */
#define CNDP_MQ_STAT_L4_PROTO_DROP 14 /* ip4_proto drop */
#define CNDP_MQ_STAT_L4_TCP 15        /* ip4_proto's tcp_input edge */
#define CNDP_MQ_STAT_L4_NOMD 16       /* udp_input drop: the metadata hook answered NULL */

/* A queue in mode CNDP_MQ_UDP_INPUT over `tbl`, which must outlive it.
 * conf->metadata is pktmbuf_metadata (NULL: m + 64); poll calls it.  Entries,
 * flags and user values changed between batches reach the batches launched
 * after the change.  The queue reads the table's device mirror by the protocol
 * cndp_gpu_udp_input uses, so both may run on one table.
 * -EINVAL: a NULL argument, another mode, any conf->flags bit, what
 * cndp_gpu_mq_create answers for batch, depth, stage_max and umem, and a table
 * already bound to another device.  cndp_gpu_mq_create, cndp_gpu_mq_create_fwd
 * and cndp_gpu_mq_create_ip4_forward answer -EINVAL for this mode. */
int cndp_gpu_mq_create_udp_input(cndp_gpu_ctx_t *ctx, const struct cndp_mq_conf *conf,
                                 cndp_pcb_tbl_t *tbl, cndp_gpu_mq_t **out);

/* The same two nodes on the calling thread over the table's host image: one
 * burst of n <= 256 mbufs, the same mbuf header and metadata edits and the same
 * edges as the queue's.  readable_end NULL: no region; otherwise the end of the
 * region the mbufs lie in, as the zero-copy queue has it: frames are clipped
 * there, and a NULL entry of mbufs[], an mbuf whose header ends past it or a
 * frame whose first byte lies at or past it is not taken (CNDP_MQ_EDGE_NONE,
 * nothing read or written).  stage_max 0: no clip; otherwise frames are
 * clipped at stage_max bytes from mtod, as the staged queue has it.  metadata
 * NULL means m + 64.  -EINVAL: tbl NULL, n above 256, or n != 0 with mbufs or
 * edges NULL; -ENOMEM. */
int cndp_udp_input_node_host(cndp_pcb_tbl_t *tbl, void *const *mbufs, uint32_t n, uint16_t *edges,
                             const void *readable_end, uint32_t stage_max,
                             void *(*metadata)(const void *m));

/* A host-only 64-bit value per PCB: what the node stores in m->userptr on
 * chnl_recv (a binding stores its struct pcb_entry * there).  The default is
 * the entry's index; cndp_pcb_del resets it to that.  It is not part of the
 * device image and does not bump the table's generation; a value set while a
 * batch is in flight may or may not reach that batch.  -EINVAL: a NULL table
 * (or `user`), an index outside the vector. */
int cndp_pcb_user_set(cndp_pcb_tbl_t *tbl, uint32_t idx, uint64_t user);
int cndp_pcb_user_get(cndp_pcb_tbl_t *tbl, uint32_t idx, uint64_t *user);

#ifdef __cplusplus
}
#endif
#endif

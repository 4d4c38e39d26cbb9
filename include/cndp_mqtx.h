/*
 * cndp_mqtx.h -- cnet's UDP transmit, udp_output + ip4_output (CNDP v25.08.0,
 * lib/cnet/udp/udp_output.c:33-65, lib/cnet/ipv4/ip4_output.c:48-126, with
 * pktmbuf_prepend / pktmbuf_adj_offset of pktmbuf.h:924-983), as a mode of the
 * asynchronous mbuf queue (cndp_gpu_mq_*, cndp_gpu.h), and the same two nodes on
 * the calling thread (cndp_ip4_output_node_host).  Both take pktmbuf_t bursts as
 * the application hands them to udp_output (CNDP_TX_UDP) or as the TCP
 * continuation hands them to ip4_output (CNDP_TX_IP4, what cndp_tcp_output_host
 * built), and resolve them in a PCB table (cndp_pcb_*, cndp_l4.h, with the
 * transmit attributes of cndp_tx.h) and a forwarding table (cndp_fwd_*,
 * cndp_fwd.h, with the netifs' identification counters of cndp_tx.h).  It is
 * cndp_gpu_ip4_output's rule (cndp_tx.h) over mbufs instead of a slab, with the
 * mbuf bookkeeping that stage leaves out.
 *
 * A queue made here is driven by cndp_gpu_mq_submit / _flush / _poll / _wait /
 * _pending / _stat / _free as every other one.
 *
 * The mbuf at submit: pktmbuf_mtod is the payload (CNDP_TX_UDP) or the L4 header
 * (CNDP_TX_IP4) and data_len its length.  The low 32 bits of m->userptr are the
 * PCB's index in the table: the default user value CNDP_MQ_UDP_INPUT leaves
 * there on chnl_recv (cndp_pcb_user_set, cndp_mql4.h); a binding that keeps its
 * own pointer there puts the index back before it submits.  The metadata
 * (conf->metadata, NULL = m + 64) holds faddr at +0 and laddr at +20, two
 * 20-byte struct in_caddr with the port at +2 and the address at +4, as
 * udp_input left them: faddr is the sender, so an untouched mbuf is an echo.
 *
 * H is data_off at submit.  Lengths are uint16_t arithmetic as in cndp_tx.h.
 * Per mbuf, in submission order:
 *   1. Not taken (CNDP_MQ_EDGE_NONE, nothing read or written, counted nowhere):
 *      m->userptr above 32 bits, at or past the vector's length, or naming a
 *      deleted PCB (the reference dereferences it); zero-copy only: the mbuf
 *      header, or the bytes from max(buf_addr, mtod - 42) (34 in CNDP_TX_IP4) up
 *      to mtod, not inside one registered region.
 *   2. md == NULL: pkt_drop, cause NOMD, nothing written (udp_output.c:40-42,
 *      ip4_output.c:64-66).
 *   3. CNDP_TX_UDP only, udp_output: the whole tx_offload word becomes 0
 *      (:46-47; the l4_len = 8 just stored is overwritten).  H < 8: pkt_drop,
 *      cause HEADROOM, nothing else changes.  Otherwise data_off -= 8,
 *      data_len += 8 and the UDP header is written at the new mtod: src_port from
 *      md->laddr, dst_port from md->faddr, dgram_len = htobe16(data_len),
 *      dgram_cksum = 0.
 *   4. ip4_output: l3_len = 20 (bits 7-15 of tx_offload; in CNDP_TX_IP4 the
 *      other bits stay).  Headroom below 20: pkt_drop, HEADROOM.  Otherwise 20
 *      bytes are prepended and the IPv4 header is written but for packet_id:
 *      0x45, the PCB's tos, total_length = htobe16(data_len), fragment_offset 0,
 *      the PCB's ttl and ip_proto, hdr_checksum 0, dst from md->faddr, src from
 *      md->laddr.  The route FIB on be32toh(src); a miss: pkt_drop, NOROUTE, and
 *      packet_id's two bytes stay as the headroom had them.  l2_len = 14
 *      (bits 0-6); headroom below 14: pkt_drop, HEADROOM.  Otherwise 14 bytes are
 *      prepended; s_addr is the route's netif's MAC, ether_type 0x0800,
 *      packet_id = htobe16(the netif's ip_ident), and the counter advances by
 *      total_length AS LOADED (the big-endian field on a little-endian host, a
 *      uint16_t that wraps); hdr_checksum.  The PCB's ip_proto neither 17 nor 6:
 *      pkt_drop, PROTO, with the counter advanced and the header checksum
 *      written.  The UDP checksum when the PCB has CNDP_UDP_CHKSUM_FLAG (a
 *      computed 0 goes out as 0xFFFF), the TCP checksum always; the field is
 *      where the PCB's ip_proto puts it (+6 or +16 from the L4 start), in either
 *      mode; a total_length below 20 after the wrap sums to 0.  The ARP FIB on
 *      be32toh(dst): a hit writes d_addr and gives edge netif_idx + 2 (the
 *      route's netif), a miss gives arp_request with d_addr untouched.
 *   5. Which bytes exist after each stopping point are exactly the ones
 *      cndp_gpu_ip4_output writes for it.  m->userptr is never written.
 *
 * Order: frame i's packet_id is its netif's counter plus the step of every
 * earlier submitted mbuf that reached the same netif, across bursts and across
 * batches; burst boundaries decide nothing.  Two queues, or a queue and
 * cndp_gpu_ip4_output, on one table are ordered as their launches were.  After a
 * batch the device counters are authoritative, as after cndp_gpu_ip4_output:
 * cndp_fwd_netif_ident_get, cndp_tx_output_host and cndp_ip4_output_node_host
 * first wait for the table's last launch.  A cndp_fwd_netif_ident_set, and
 * table changes made with nothing pending, reach the next batch.
 *
 * Defined by this build:
 *  - The L4 bytes read for a checksum are [mtod, mtod + data_len) as they were at
 *    submit, clipped at buf_addr + buf_len always; at the end of the frame's
 *    registered region for zero-copy; at stage_max bytes from mtod for staged
 *    (conf.stage_max, 0 = 2048).  Bytes past the clip read as zero and are never
 *    written: a checksum field that lies past it is not stored.
 *  - a netif index is below 256 and an unset netif's MAC is six zero bytes, a
 *    new table's counters are 0, as in cndp_tx.h.
 *
 * Edge of each mbuf: (edge & CNDP_MQ_EDGE_TX_MASK) is ip4_output's own edge,
 * CNDP_TX_EDGE_PKT_DROP 0, CNDP_TX_EDGE_ARP_REQUEST 1 or netif_idx + 2;
 * CNDP_MQ_EDGE_TX_CAUSE(edge) names a drop's cause; CNDP_MQ_EDGE_TX_CKSUM is set
 * when an L4 checksum was generated.
 *
 * The device writes neither mbuf headers nor metadata.  Frame bytes are written
 * by the device: zero-copy in place in the registered pool, staged into the
 * slot's staging, from where cndp_gpu_mq_poll copies back exactly the bytes
 * written.  Per mbuf the device returns one record into pinned memory (the edge
 * and how far the frame got) and poll makes the data_off / data_len / tx_offload
 * edits on the calling lcore, zero-copy and staged alike.  poll also counts the
 * seven keys below from the edges it returns; they are exact once
 * cndp_gpu_mq_pending is 0.  CNDP_MQ_EDGE_NONE mbufs count nowhere and every
 * other family's key above 10 answers -EINVAL here, as these seven do on a queue
 * of any other mode.
 */
#ifndef CNDP_MQTX_H
#define CNDP_MQTX_H

#include <stdint.h>

#include "cndp_gpu.h"
#include "cndp_tx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_MQ_IP4_OUTPUT 10u /* udp_output_node_do + ip4_output_node_process */

#define CNDP_MQ_EDGE_TX_MASK 0x01FFu /* ip4_output's own edge */
#define CNDP_MQ_EDGE_TX_CAUSE(e) (((e) >> 9) & 7u)
#define CNDP_MQ_TX_CAUSE_NOMD 1u     /* the metadata hook answered NULL */
#define CNDP_MQ_TX_CAUSE_HEADROOM 2u /* pktmbuf_adjust / pktmbuf_prepend failed */
#define CNDP_MQ_TX_CAUSE_NOROUTE 3u  /* no route to the local address */
#define CNDP_MQ_TX_CAUSE_PROTO 4u    /* pcb->ip_proto is neither UDP nor TCP */
#define CNDP_MQ_EDGE_TX_CKSUM 0x1000u /* an L4 checksum was generated */

#define CNDP_MQ_STAT_TX_SENT 25
#define CNDP_MQ_STAT_TX_ARP_REQUEST 26
#define CNDP_MQ_STAT_TX_DROP_NOMD 27
#define CNDP_MQ_STAT_TX_DROP_HEADROOM 28
#define CNDP_MQ_STAT_TX_DROP_NOROUTE 29
#define CNDP_MQ_STAT_TX_DROP_PROTO 30
#define CNDP_MQ_STAT_TX_CKSUM 31

/* A queue in mode CNDP_MQ_IP4_OUTPUT over the two tables, which must outlive
 * it.  conf->metadata is pktmbuf_metadata (NULL: m + 64); submit calls it.  The
 * queue reads the tables' device mirrors by the protocol cndp_gpu_ip4_output
 * uses, so both may run on one pair of tables.
 * -EINVAL: a NULL argument, another mode, any conf->flags bit, tx_mode above
 * CNDP_TX_IP4, what cndp_gpu_mq_create answers for batch, depth, stage_max and
 * umem, and a table already bound to another device.  The other create calls
 * answer -EINVAL for this mode. */
int cndp_gpu_mq_create_ip4_output(cndp_gpu_ctx_t *ctx, const struct cndp_mq_conf *conf,
                                  cndp_fwd_tbl_t *fwd_tbl, cndp_pcb_tbl_t *pcb_tbl, uint32_t tx_mode,
                                  cndp_gpu_mq_t **out);

/* The same two nodes on the calling thread over the tables' host images: one
 * burst of n <= 256 mbufs, the same frame bytes, mbuf header edits and edges as
 * the queue's; the host counters advance.  Waits for the tables' last GPU call
 * first.  readable_end NULL: no region; otherwise the end of the region the
 * mbufs lie in, as the zero-copy queue has it: the L4 bytes are clipped there,
 * and a NULL entry of mbufs[], an mbuf whose header ends past it or whose mtod
 * lies past it is not taken.  stage_max 0: no clip; otherwise the L4 bytes are
 * clipped at stage_max bytes from mtod, as the staged queue has it.  metadata
 * NULL means m + 64.  -EINVAL: a table NULL, tx_mode above CNDP_TX_IP4, n above
 * 256, or n != 0 with mbufs or edges NULL; -ENOMEM. */
int cndp_ip4_output_node_host(cndp_fwd_tbl_t *fwd_tbl, cndp_pcb_tbl_t *pcb_tbl, uint32_t tx_mode,
                              void *const *mbufs, uint32_t n, uint16_t *edges, const void *readable_end,
                              uint32_t stage_max, void *(*metadata)(const void *m));

#ifdef __cplusplus
}
#endif
#endif

/*
 * cndp_mqcnet.h -- cnet's ip4_forward node (CNDP v25.08.0,
 * lib/cnet/ipv4/ip4_forward.c:50-335) as a mode of the asynchronous mbuf queue
 * (cndp_gpu_mq_*, cndp_gpu.h), and the same node on the calling thread
 * (cndp_fwd_node_host).  Both take pktmbuf_t bursts as ip4_input hands them to
 * its forward edge and resolve them in a forwarding table (cndp_fwd_*,
 * cndp_fwd.h), whose group rules and build-defined cases apply here unchanged.
 *
 * A queue made here is driven by cndp_gpu_mq_submit / _flush / _poll / _wait /
 * _pending / _stat / _free as every other one.
 *
 * The mbuf at submit: pktmbuf_mtod is the IPv4 header, l2_len is
 * tx_offload & 0x7F, data_len is whatever it is.  Per mbuf, in this order
 * (:112-115, :271-318):
 *   1. dst_addr from header bytes 16-19;
 *   2. ipv4_adjust_cksum on header byte 8 and bytes 10-11;
 *   3. pktmbuf_adjust(m, -l2_len): data_off -= l2_len, data_len += l2_len, both
 *      as uint16_t;
 *   4. the ARP FIB on the destination, then the route FIB, then the ARP FIB on
 *      the route's gateway;
 *   5. on a hit d_addr at the new mtod + 0 and s_addr at + 6.
 * Each submitted burst -- a submit call, or each 256-mbuf chunk of a longer one
 * -- is the node's objs[]; the queue never splits one.  The first k & ~3 mbufs
 * of a burst of k go through the 4-wide loop in groups of four consecutive
 * mbufs, the rest through the 1-wide loop.
 *
 * The only frame bytes that may change are header byte 8, header bytes 10-11
 * and the 12 MAC bytes; the only mbuf header fields data_off and data_len,
 * which cndp_gpu_mq_poll writes on the host, zero-copy or staged: the device
 * never writes an mbuf header in this mode.
 *
 * Edge of each mbuf: CNDP_FWD_EDGE_ARP_REQUEST, or netif_idx + 2 with
 * CNDP_MQ_EDGE_FWD_GATEWAY OR-ed in when the frame goes through a route's
 * gateway; (edge & CNDP_MQ_EDGE_FWD_MASK) is the node's own edge.
 *
 * Where the reference writes through NULL or reads out of bounds this build
 * defines the result:
 *  - l2_len > data_off (pktmbuf_adj_offset answers NULL, :115): the mbuf keeps
 *    its place in its group and gets its TTL / checksum edit and its edge; no
 *    MAC byte is written and data_off / data_len stay;
 *  - l2_len < 12: the MAC bytes overlap the IP header; they are written after
 *    the TTL / checksum bytes and win, as in the reference;
 *  - zero-copy, an mbuf or a frame (its IPv4 header's first byte) outside
 *    every registered region: the edge is CNDP_MQ_EDGE_NONE, nothing is read or
 *    written, the mbuf keeps its group position and contributes no hit;
 *  - bytes past what is readable read as zero and are never written:
 *    zero-copy, readable ends at the end of the frame's registered region (and
 *    MAC bytes in front of that region's start are not written either);
 *    staged, at buf_addr + buf_len.
 *
 * Counters: none on the device.  cndp_gpu_mq_poll counts the three keys below
 * from the edges it returns, so they are exact once cndp_gpu_mq_pending is 0;
 * CNDP_MQ_EDGE_NONE mbufs count nowhere, and every other family's key reads 0.
 */
#ifndef CNDP_MQCNET_H
#define CNDP_MQCNET_H

#include <stdint.h>

#include "cndp_fwd.h"
#include "cndp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_MQ_IP4_FORWARD 7u           /* ip4_forward_node_process, lib/cnet/ipv4/ip4_forward.c:50-335 */
#define CNDP_MQ_EDGE_FWD_GATEWAY 0x0400u /* OR-ed into the edge of a frame sent through a route's gateway */
#define CNDP_MQ_EDGE_FWD_MASK 0x01FFu    /* the node's own edge: 1 = arp_request, netif_idx + 2 */

#define CNDP_MQ_STAT_FWD_DIRECT 8       /* transmitted on the destination's own ARP entry */
#define CNDP_MQ_STAT_FWD_GATEWAY 9      /* transmitted through a route's gateway */
#define CNDP_MQ_STAT_FWD_ARP_REQUEST 10 /* sent to arp_request */

/* A queue in mode CNDP_MQ_IP4_FORWARD over `tbl`, which must outlive it.
 * Objects, netif MACs and FIB routes changed between batches reach the batches
 * launched after the change.  The queue reads the table's device mirror by the
 * protocol cndp_gpu_ip4_forward uses, so both may run on one table.
 * -EINVAL: a NULL argument, another mode, any conf->flags bit, what
 * cndp_gpu_mq_create answers for batch, depth, stage_max and umem, and a table
 * already bound to another device.  cndp_gpu_mq_create and
 * cndp_gpu_mq_create_fwd answer -EINVAL for this mode. */
int cndp_gpu_mq_create_ip4_forward(cndp_gpu_ctx_t *ctx, const struct cndp_mq_conf *conf, cndp_fwd_tbl_t *tbl,
                                   cndp_gpu_mq_t **out);

/* The same node on the calling thread over the table's host images: one burst
 * of n <= 256 mbufs, the first n & ~3 through the 4-wide loop, the rest through
 * the 1-wide loop; the same frame and mbuf header edits and the same edges,
 * gateway bit included, as the queue's.  readable_end NULL bounds each frame
 * by its mbuf's buf_addr + buf_len, as the staged queue does; otherwise it is
 * the end of the region the mbufs lie in, as the zero-copy queue has it: an
 * mbuf whose header or whose frame's first byte lies at or past it is not
 * taken (edge CNDP_MQ_EDGE_NONE, as is a NULL entry of mbufs[], which stands
 * for an mbuf outside the region).  There is no lower bound here: MAC bytes go
 * wherever mtod - l2_len points.  -EINVAL: tbl NULL, n above 256, or n != 0
 * with mbufs or edges NULL. */
int cndp_fwd_node_host(cndp_fwd_tbl_t *tbl, void *const *mbufs, uint32_t n, uint16_t *edges,
                       const void *readable_end);

#ifdef __cplusplus
}
#endif
#endif

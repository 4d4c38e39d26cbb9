/*
 * cndp_tx.h -- UDP transmit on MI355X: the two cnet graph nodes that turn a
 * payload in an mbuf into a frame (CNDP v25.08.0):
 *
 *   udp_output  lib/cnet/udp/udp_output.c:33-65     pktmbuf_adjust(m, -8)
 *               (pktmbuf.h:955-983), the UDP header in front of the payload:
 *               ports from md->faddr / md->laddr, dgram_len = htobe16(data_len),
 *               dgram_cksum = 0.
 *   ip4_output  lib/cnet/ipv4/ip4_output.c:48-126   pktmbuf_prepend(m, 20), the
 *               IPv4 header from the PCB (tos, ttl, ip_proto) and the metadata
 *               addresses; the route FIB on be32toh(src_addr) names the netif;
 *               pktmbuf_prepend(m, 14), s_addr and ether_type; packet_id from the
 *               netif's running ip_ident, which then advances by total_length AS
 *               LOADED (the big-endian field on a little-endian host, a uint16_t
 *               that wraps, cnet_netif.h:89); cne_ipv4_cksum; the UDP checksum
 *               when the PCB has UDP_CHKSUM_FLAG, the TCP checksum always
 *               (cne_ipv4_udptcp_cksum, net/cne_ip.h:275-325); the ARP FIB on
 *               be32toh(dst_addr): d_addr and edge = netif_idx + 2, or arp_request.
 *
 * The node calls ip4_output_header for mbuf 0, 1, 2, 3 of its 4-wide loop in
 * turn, so the order of effects is objs[] order and there is no burst parameter.
 * The stage reuses the tables of cndp_l4.h and cndp_fwd.h: the PCB table (with
 * the transmit attributes below) and the forwarding table (with the netifs'
 * identification counters below).  Errors are negative errno values.
 *
 * Not modelled:
 *  - md == NULL (ip4_output.c:64-66) and the IPv6 branch of udp_output;
 *  - the mbuf's data_off / data_len / l2_len / l3_len bookkeeping: a batch
 *    carries frames, not mbufs; a sent frame starts data_off - 42 (UDP mode) or
 *    data_off - 34 (IP4 mode) bytes into its buffer;
 *  - arp_request itself, eth_tx and the channel callback.
 * Over pktmbuf_t bursts, with md == NULL and the bookkeeping, the same rule is a
 * mode of the mbuf queue: cndp_mqtx.h.
 * Where the reference's behaviour is undefined this build defines it:
 *  - a frame whose pcb[i] is CNDP_PCB_NONE, at or past the vector's length or a
 *    deleted entry is not taken (the reference dereferences m->userptr);
 *  - a netif index is below 256 and an unset netif's MAC is six zero bytes, as
 *    in cndp_fwd.h;
 *  - bytes at or past slab + slab_len read as zero and are never written; the
 *    header checksum and the pseudo-header sum are those of the header the stage
 *    builds, whatever part of it lies past slab_len: only L4 bytes are read;
 *  - the reference seeds ip_ident from rdtsc; a new table's counters are 0.
 * Lengths are uint16_t arithmetic as in the reference (a total_length below 20
 * after the wrap makes __ipv4_udptcp_cksum return 0); callers keep len + 28
 * inside the frame.  The L4 checksum field is where the PCB's ip_proto puts it
 * (UDP +6, TCP +16 from the L4 start), in either mode, as ip4_output.c:103-112
 * has it.
 */
#ifndef CNDP_TX_H
#define CNDP_TX_H

#include <stdint.h>

#include "cndp_fwd.h"
#include "cndp_l4.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_TX_UDP 0u /* udp_output then ip4_output: the payload is at the data offset */
#define CNDP_TX_IP4 1u /* ip4_output alone: the L4 header is at the data offset, len counts it */

#define CNDP_TX_EDGE_PKT_DROP 0u    /* IP4_OUTPUT_NEXT_PKT_DROP (also udp_output's drop) */
#define CNDP_TX_EDGE_ARP_REQUEST 1u /* IP4_OUTPUT_NEXT_ARP_REQUEST */
#define CNDP_TX_EDGE_OUTPUT 2u      /* IP4_OUTPUT_NEXT_MAX: edge = netif_idx + 2 */
#define CNDP_TX_EDGE_NONE 0xFFFFu   /* the frame was not taken */

#define CNDP_TX_STAT_SENT 0
#define CNDP_TX_STAT_ARP_REQUEST 1
#define CNDP_TX_STAT_DROP_HEADROOM 2 /* pktmbuf_adjust / pktmbuf_prepend failed */
#define CNDP_TX_STAT_DROP_NOROUTE 3  /* no route to the local address */
#define CNDP_TX_STAT_DROP_PROTO 4    /* pcb->ip_proto is neither UDP nor TCP */
#define CNDP_TX_STAT_CKSUM 5         /* datagrams whose L4 checksum was generated */
#define CNDP_TX_NSTATS 6

/* What ip4_output reads of a struct pcb_entry beyond cndp_pcb_entry.  A new
 * entry has tos 0 (TOS_DEFAULT), ttl 64 (TTL_DEFAULT, cnet_ipv4.h:32-33) and
 * ip_proto 17; deleting the entry clears them. */
struct cndp_pcb_tx {
    uint8_t tos, ttl, ip_proto;
};
/* -EINVAL for an index outside the vector, -ENOENT for a deleted entry. */
int cndp_pcb_tx_set(cndp_pcb_tbl_t *tbl, uint32_t idx, const struct cndp_pcb_tx *a);
int cndp_pcb_tx_get(cndp_pcb_tbl_t *tbl, uint32_t idx, struct cndp_pcb_tx *a);

/* netif idx's ip_ident (idx < 256, else -EINVAL).  After a GPU call the device
 * copy is authoritative: _get (and cndp_tx_output_host) first wait for the
 * table's last cndp_gpu_ip4_output and read the 256 counters back; a _set
 * reaches the device before the next call. */
int cndp_fwd_netif_ident_set(cndp_fwd_tbl_t *tbl, uint32_t idx, uint16_t ident);
int cndp_fwd_netif_ident_get(cndp_fwd_tbl_t *tbl, uint32_t idx, uint16_t *ident);

/* Arrays of n elements (stats: CNDP_TX_NSTATS), optional unless noted: device
 * memory for cndp_gpu_ip4_output, host memory for cndp_tx_output_host. */
struct cndp_tx_io {
    const uint8_t *sel;    /* in: frame i is a candidate when sel[i] != 0; NULL = all */
    const uint32_t *pcb;   /* in, required: m->userptr as an index into the PCB table */
    const uint32_t *faddr; /* in, required: md->faddr / md->laddr addresses, as a   */
    const uint32_t *laddr; /*     little-endian host loads them from a frame        */
    const uint32_t *ports; /* in, required in CNDP_TX_UDP: fport | lport << 16, the
                            * packing cndp_l4_io.ports returns */
    const uint16_t *len;   /* in, required: m->data_len on entry */
    uint16_t *tx_edge;     /* out, required: CNDP_TX_EDGE_* */
    uint16_t *bin_of;      /* out: the netif for transmitted frames, n_bins for arp_request,
                            * n_bins + 1 for the rest: cndp_gpu_bin_partition's input */
    uint32_t n_bins;       /* > cndp_fwd_max_netif(fwd_tbl) and <= 65533 when bin_of is given */
    uint64_t *stats;       /* out: [CNDP_TX_NSTATS], CNDP_TX_STAT_*, accumulated (+=) */
};

/* Enqueue udp_output + ip4_output (CNDP_TX_UDP) or ip4_output (CNDP_TX_IP4)
 * over the frames of `b`, writing the headers IN PLACE into b->slab in front of
 * each frame's data.  b gives the layout only: slab, slab_len, stride / offsets
 * (the mbuf's buffer) and data_off (the mbuf's data_off, the headroom: the same
 * for every frame of a call); the classify outputs of b are not read.  Frame
 * i's packet_id is its netif's counter at call start plus total_length as loaded
 * of every earlier frame of the call, in index order, that reached the same
 * netif.  The call returns without waiting for the kernels; tables changed
 * since the last call are copied to their device mirrors first and those copies
 * are waited for, and both FIB mirrors are synced.  Calls on one table are
 * serialised and ordered across streams.  Both tables are bound to the device
 * of their first call.  -EINVAL for argument errors. */
int cndp_gpu_ip4_output(cndp_gpu_ctx_t *ctx, cndp_fwd_tbl_t *fwd_tbl, cndp_pcb_tbl_t *pcb_tbl,
                        const struct cndp_batch *b, uint32_t mode, const struct cndp_tx_io *io,
                        void *stream);

/* The same rule on the calling thread over host memory and the host images;
 * io holds host pointers.  Waits for the tables' last GPU call first. */
int cndp_tx_output_host(cndp_fwd_tbl_t *fwd_tbl, cndp_pcb_tbl_t *pcb_tbl, uint32_t mode, void *slab,
                        uint64_t slab_len, uint64_t stride, const uint64_t *offsets, uint32_t data_off,
                        uint32_t n, const struct cndp_tx_io *io_host);

#ifdef __cplusplus
}
#endif
#endif

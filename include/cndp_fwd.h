/*
 * cndp_fwd.h -- ip4_forward on MI355X: the cnet graph node behind ip4_input's
 * forward edge (CNDP v25.08.0):
 *
 *   ip4_forward  lib/cnet/ipv4/ip4_forward.c:50-335   TTL - 1 with the incremental
 *                checksum (ipv4_adjust_cksum, cnet_ipv4.h:159-170), then up to
 *                three dependent FIB lookups (fib_info_lookup,
 *                incs/cnet_fib_info.h:52-61,239-251,330-377): the ARP FIB on the
 *                destination, the route FIB, the ARP FIB on the route's gateway;
 *                the source and destination MAC written into the frame; edge =
 *                netif_idx + NODE_IP4_FORWARD_OUTPUT_OFFSET, or arp_request.
 *
 * The forwarding table (cndp_fwd_*) is plain host C and holds what the node
 * reads of this_cnet: the two FIBs, the ARP and route object arrays behind them
 * and the netif MACs.  The host image answers synchronous callers
 * (cndp_fwd_lookup, what ip4_output.c:87,118 needs), a device mirror answers
 * batches (cndp_gpu_ip4_forward), the same split the FIBs and the PCB tables
 * have.  The stage runs after a CNDP_MODE_CNET cndp_gpu_classify of the same
 * batch, on that call's outputs.  Errors are negative errno values.
 *
 * Not modelled:
 *  - the node's cached next_index (ip4_forward.c:69,210-268,306-317): it only
 *    decides how the per-edge streams are filled, never a frame's edge;
 *  - the mbuf's data_off / data_len adjustment (pktmbuf_adjust, :115,279): a
 *    batch carries frames, not mbufs (over mbufs: the queue mode and the host
 *    node of cndp_mqcnet.h, which make it).
 * Where the reference's behaviour is undefined this build defines it:
 *  - a frame of a 4-wide group without a route object has no gateway: no
 *    lookup is made and it counts as a miss (:162-175 read gateway[k]
 *    uninitialised);
 *  - lanes 1-3 of a 4-wide group take the destination MAC of lane 0's gateway
 *    entry (:190,196,202); when lane 0 has none (a NULL dereference there) the
 *    lane takes its own entry's;
 *  - a netif index is below 256 (cnet_netif_from_index takes a uint8_t and
 *    indexes a vector unchecked): the table rejects larger ones, and the MAC of
 *    a netif never set is six zero bytes;
 *  - bytes at or past slab + slab_len read as zero and are never written.
 */
#ifndef CNDP_FWD_H
#define CNDP_FWD_H

#include <stdint.h>

#include "cndp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_FWD_OBJS_MAX (1u << 24) /* an object index is a FIB value's low 24 bits */
#define CNDP_FWD_NETIFS 256u
#define CNDP_FWD_NONE 0xFFFFFFFFu
#define CNDP_FWD_EDGE_PKT_DROP 0u    /* ip4_forward_priv.h: never taken by the node's arithmetic */
#define CNDP_FWD_EDGE_ARP_REQUEST 1u /* NODE_IP4_FORWARD_ARP_REQUEST */
#define CNDP_FWD_EDGE_OUTPUT 2u      /* NODE_IP4_FORWARD_OUTPUT_OFFSET: edge = netif_idx + 2 */
#define CNDP_FWD_EDGE_NONE 0xFFFFu   /* the frame was not taken */

/* What the node reads of a struct arp_entry. */
struct cndp_fwd_arp {
    uint16_t netif_idx; /* < CNDP_FWD_NETIFS */
    uint8_t ha[6];
};

/* What the node reads of a struct rt4_entry.  gateway is gateway.s_addr as the
 * stack stores it; the node hands it to the ARP FIB as it is (:166,178,295),
 * while destinations are looked up as be32toh(dst_addr) (:113,282). */
struct cndp_fwd_rt {
    uint32_t gateway;
    uint16_t netif_idx; /* < CNDP_FWD_NETIFS */
};

/* One answer of cndp_fwd_lookup. */
struct cndp_fwd_result {
    uint16_t edge;     /* netif_idx + 2, or CNDP_FWD_EDGE_ARP_REQUEST (MACs zero) */
    uint8_t s_addr[6]; /* the outgoing netif's MAC */
    uint8_t d_addr[6]; /* the ARP entry's ha */
};

typedef struct cndp_fwd_tbl cndp_fwd_tbl_t;

/* arp_fib / rt4_fib: cnet's "arp-fib" and "rt4-fib", DIR-24-8 with 4-byte
 * entries as cnet_arp.c:186-193 and cnet_route4.c:171-178 create them (anything
 * else is -EINVAL); the caller's, and they must outlive the table.  arp_objs /
 * rt_objs: capacities of the object arrays in [1, CNDP_FWD_OBJS_MAX].  A FIB
 * value v names object v & 0xFFFFFF, a hit only when that index is below the
 * capacity and the slot is set -- so the FIBs' default next hop (num_entries +
 * 1, cnet_arp.c:189-190, cnet_route4.c:174-175) is a miss.  -EINVAL, -ENOMEM. */
int cndp_fwd_create(struct cne_fib *arp_fib, struct cne_fib *rt4_fib, uint32_t arp_objs,
                    uint32_t rt_objs, cndp_fwd_tbl_t **out);
void cndp_fwd_free(cndp_fwd_tbl_t *tbl);
/* Set / replace and clear an object slot (fib_info_alloc / fib_info_free).
 * -EINVAL for an index at or past the capacity or a netif_idx >= 256, -ENOENT
 * for clearing a slot that is not set. */
int cndp_fwd_arp_set(cndp_fwd_tbl_t *tbl, uint32_t idx, const struct cndp_fwd_arp *e);
int cndp_fwd_arp_clear(cndp_fwd_tbl_t *tbl, uint32_t idx);
int cndp_fwd_rt_set(cndp_fwd_tbl_t *tbl, uint32_t idx, const struct cndp_fwd_rt *e);
int cndp_fwd_rt_clear(cndp_fwd_tbl_t *tbl, uint32_t idx);
/* The MAC of netif idx (< 256, else -EINVAL); mac NULL = six zero bytes again. */
int cndp_fwd_netif_set(cndp_fwd_tbl_t *tbl, uint32_t idx, const uint8_t *mac);
/* The largest netif_idx of the objects now set, or -1 without one; -EINVAL. */
int cndp_fwd_max_netif(cndp_fwd_tbl_t *tbl);
/* The node's 1-wide rule (ip4_forward.c:271-318) on the calling thread over the
 * host images: dst_be[k] is a destination address as a little-endian host
 * loads it from the frame. */
int cndp_fwd_lookup(cndp_fwd_tbl_t *tbl, const uint32_t *dst_be, uint32_t n,
                    struct cndp_fwd_result *out);

#define CNDP_FWD_STAT_DIRECT 0      /* transmitted on the destination's own ARP entry */
#define CNDP_FWD_STAT_GATEWAY 1     /* transmitted through a route's gateway */
#define CNDP_FWD_STAT_ARP_REQUEST 2 /* sent to arp_request */

/* Device arrays of n elements (stats: 3), optional unless noted. */
struct cndp_fwd_io {
    const uint8_t *sel; /* in: frame i is taken when sel[i] != 0.  NULL = derived:
                         * nh[i] != CNDP_NH_INVALID, nh[i] >> 24 == 1 (the input node's
                         * forward edge) and ptype[i]'s own p_nxt edge is ip4_input
                         * (b->ptype required) -- exact whenever the ptype node's
                         * speculation did not route the frame to another node than
                         * its own type's */
    uint16_t *fwd_edge; /* required: the node's edge, CNDP_FWD_EDGE_NONE if not taken */
    uint32_t *arp_idx;  /* the ARP object whose ha was written, else CNDP_FWD_NONE; lane
                         * 0's for lanes 1-3 of a 4-wide group's gateway case */
    uint16_t *bin_of;   /* edge - 2 (the netif) for transmitted frames, n_bins for
                         * arp_request, n_bins + 1 for frames not taken:
                         * cndp_gpu_bin_partition's input */
    uint32_t n_bins;    /* > cndp_fwd_max_netif(tbl) and <= 65533 when bin_of is given */
    uint64_t *stats;    /* [3], CNDP_FWD_STAT_*, accumulated (+=) */
};

/* Enqueue ip4_forward over the frames of `b` that ip4_input sent to its
 * forward edge, rewriting b->slab IN PLACE: TTL and header checksum at mtod =
 * frame + l2_len for every taken frame (arp_request ones included), the MACs at
 * the frame start (d_addr +0, s_addr +6, whatever l2_len is) for transmitted
 * ones.  b gives the frame layout and the cnet classify outputs read here: b->nh
 * and b->rxmeta (both required).  The batch is cut into graph bursts of `burst`
 * consecutive frames, in [1, 256] (the last may be short): the taken frames of
 * a burst, in order, are the node's objs[]; with C of them the first C & ~3 go
 * through the 4-wide loop (:88-269) in groups of four, the rest through the
 * 1-wide loop (:271-318) -- one receive burst per graph walk.  The call returns
 * without waiting for the kernel; a table changed since the last call is
 * copied to its device mirror first and that copy is waited for, and both FIB
 * mirrors are synced.  Calls on one table are serialised and ordered across
 * streams.  A table is bound to the device of its first call. */
int cndp_gpu_ip4_forward(cndp_gpu_ctx_t *ctx, cndp_fwd_tbl_t *tbl, const struct cndp_batch *b,
                         uint32_t burst, const struct cndp_fwd_io *io, void *stream);

#ifdef __cplusplus
}
#endif
#endif

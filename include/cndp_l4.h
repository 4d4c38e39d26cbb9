/*
 * cndp_l4.h -- UDP socket demux on MI355X: the two cnet graph nodes behind
 * ip4_input's proto edge (CNDP v25.08.0, default build: enable_ip6 false,
 * enable_tcp false):
 *
 *   ip4_proto   lib/cnet/ipv4/ip4_proto.c:30-195   proto_nxt[next_proto_id]
 *   udp_input   lib/cnet/udp/udp_input.c:43-123    4-tuple key, best-match PCB
 *               lookup (cnet_pcb_lookup, lib/cnet/pcb/cnet_pcb.c:41-92),
 *               optional UDP checksum verify (cne_ipv4_udptcp_cksum_verify,
 *               net/cne_ip.h:275-349), chnl_recv / pkt_punt / pkt_drop
 *
 * The PCB table (cndp_pcb_*) is plain host C: the host image answers
 * synchronous callers (cndp_pcb_lookup), a device mirror answers batches
 * (cndp_gpu_udp_input), the same split the FIBs have.  The stage runs after a
 * CNDP_MODE_CNET cndp_gpu_classify of the same batch, on that call's outputs.
 * Errors are negative errno values.
 */
#ifndef CNDP_L4_H
#define CNDP_L4_H

#include <stdint.h>

#include "cndp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_PCB_MAX_ENTRIES 4096u /* the reference's own cap is CNET_NUM_CHANNELS = 512 */
#define CNDP_PCB_NONE 0xFFFFFFFFu
#define CNDP_UDP_CHKSUM_FLAG 0x0080u /* UDP_CHKSUM_FLAG, lib/cnet/chnl/chnl_priv.h:276 */

/* What udp_input reads of a struct pcb_entry.  Addresses and ports are in
 * network order, as the u32 / u16 a little-endian host loads from the frame. */
struct cndp_pcb_entry {
    uint32_t laddr;
    uint32_t faddr;
    uint16_t lport;
    uint16_t fport;
    uint16_t opt_flag; /* only CNDP_UDP_CHKSUM_FLAG matters here */
};

/* struct pcb_key (cnet_pcb.h:31-34), IPv4 */
struct cndp_pcb_key {
    uint32_t laddr;
    uint32_t faddr;
    uint16_t lport;
    uint16_t fport;
};

typedef struct cndp_pcb_tbl cndp_pcb_tbl_t;

/* max_entries in [1, CNDP_PCB_MAX_ENTRIES], else -EINVAL; -ENOMEM. */
int cndp_pcb_create(uint32_t max_entries, cndp_pcb_tbl_t **out);
void cndp_pcb_free(cndp_pcb_tbl_t *tbl);
/* cnet_pcb_alloc's vec_add: returns the entry's index in vector order,
 * -ENOSPC when the vector is full, -EINVAL. */
int cndp_pcb_add(cndp_pcb_tbl_t *tbl, const struct cndp_pcb_entry *e);
/* cnet_pcb_delete -> cnet_pcb_free (cnet_pcb.h:63-111): the entry is zeroed and
 * STAYS in the vector, where it matches a key with local port 0 as an any/any
 * entry from then on.  -EINVAL for an index outside the vector, -ENOENT for an
 * entry already deleted.  The mempool's reuse of freed objects is not
 * modelled: an index is never handed out twice. */
int cndp_pcb_del(cndp_pcb_tbl_t *tbl, uint32_t idx);
/* cnet->flags & CNET_PUNT_ENABLED (udp_input.c:122), and whether ip4_proto was
 * built with CNET_ENABLE_TCP (ip4_proto.c:190-192).  A new table has punting
 * on and TCP off, the reference's default build. */
int cndp_pcb_set_flags(cndp_pcb_tbl_t *tbl, int punt_enabled, int tcp_enabled);
/* Length of the vector (deleted entries included), or -EINVAL. */
int cndp_pcb_count(cndp_pcb_tbl_t *tbl);
/* pcb_v4_lookup with BEST_MATCH on the calling thread, host image:
 * idx_out[k] = the entry's index or CNDP_PCB_NONE. */
int cndp_pcb_lookup(cndp_pcb_tbl_t *tbl, const struct cndp_pcb_key *keys, uint32_t n,
                    uint32_t *idx_out);

/* Edges of the two nodes as the stage reports them. */
#define CNDP_L4_NODE_IP4_PROTO 0u
#define CNDP_L4_NODE_UDP_INPUT 1u
#define CNDP_L4_EDGE(node, e) ((uint8_t)(((node) << 4) | (e)))
#define CNDP_L4_EDGE_NONE 0xFFu /* the frame was not taken */
#define CNDP_IP4_PROTO_DROP 0u  /* CNE_NODE_IP4_INPUT_PROTO_DROP */
#define CNDP_IP4_PROTO_TCP 2u   /* CNE_NODE_IP4_INPUT_PROTO_TCP: tcp_input stays on the CPU */
#define CNDP_UDP_INPUT_PKT_DROP 0u /* udp_input_priv.h:13-17 */
#define CNDP_UDP_INPUT_CHNL_RECV 1u
#define CNDP_UDP_INPUT_PKT_PUNT 2u

#define CNDP_L4_STAT_RECV 0      /* chnl_recv */
#define CNDP_L4_STAT_NOMATCH 1   /* udp_input drop or punt: no PCB */
#define CNDP_L4_STAT_CKSUM 2     /* udp_input drop: checksum */
#define CNDP_L4_STAT_PROTO_DROP 3 /* ip4_proto drop */

/* Device arrays of n elements (stats: 4), optional unless noted. */
struct cndp_l4_io {
    const uint8_t *sel;    /* in: frame i is taken when sel[i] != 0.  NULL = derived:
                            * nh[i] != CNDP_NH_INVALID, nh[i] >> 24 == 2 (the input
                            * node's proto edge) and ptype[i]'s own p_nxt edge is
                            * ip4_input (b->ptype required) -- exact whenever the ptype
                            * node's speculation did not route the frame to another node
                            * than its own type's */
    uint8_t *l4edge;       /* required: CNDP_L4_EDGE(node, e), CNDP_L4_EDGE_NONE if not taken */
    uint32_t *pcb;         /* m->userptr as a table index on chnl_recv, else CNDP_PCB_NONE */
    uint32_t *ports;       /* fport | lport << 16 as in the frame for every frame that
                            * reaches udp_input (udp_input.c:95-96 stores them before the
                            * lookup), else 0 */
    uint16_t *payload_off; /* l2_len + l3_len + l4_len on chnl_recv (udp_input.c:115), else 0 */
    uint16_t *bin_of;      /* the PCB index on chnl_recv, n_bins for every drop, n_bins + 1
                            * for the rest: cndp_gpu_bin_partition's input */
    uint32_t n_bins;       /* >= cndp_pcb_count(tbl) and <= 65533 when bin_of is given;
                            * cndp_gpu_bin_partition takes n_bins <= CNDP_PART_BINS_MAX
                            * (every table's count fits) and returns -EINVAL above it */
    uint64_t *stats;       /* [4], CNDP_L4_STAT_*, accumulated (+=) */
};

/* Enqueue ip4_proto + udp_input over the frames of `b` that ip4_input sent to
 * its proto edge.  b gives the frame layout (slab, slab_len, stride / offsets,
 * data_off, n) and the cnet classify outputs read here: b->nh and b->rxmeta
 * (both required; mtod = frame + l2_len, the UDP header at mtod + l3_len).
 * Bytes at or past slab + slab_len read as zero, whatever the lengths in the
 * frame say.  The call returns without waiting for the kernels; a table changed
 * since the last call is copied to its device mirror first, and that copy is
 * waited for.  Calls on one table are serialised and ordered across streams. */
int cndp_gpu_udp_input(cndp_gpu_ctx_t *ctx, cndp_pcb_tbl_t *tbl, const struct cndp_batch *b,
                       const struct cndp_l4_io *io, void *stream);

#ifdef __cplusplus
}
#endif
#endif

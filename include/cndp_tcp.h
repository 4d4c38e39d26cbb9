/*
 * cndp_tcp.h -- TCP connection demux on MI355X: the cnet graph node behind
 * ip4_proto's tcp_input edge (CNDP v25.08.0 built with enable_tcp), up to the
 * point where the TCP state machine starts:
 *
 *   tcp_input   lib/cnet/tcp/tcp_input.c:41-119    4-tuple key, best-match PCB
 *               lookup in stk->tcp->tcp_hd (cnet_pcb_lookup, cnet_pcb.c:41-92),
 *               the mandatory checksum verify (cne_ipv4_udptcp_cksum_verify,
 *               net/cne_ip.h:275-349), pkt_punt / pkt_drop
 *   cnet_tcp_input's opening, lib/cnet/tcp/cnet_tcp.c:3386-3414: the header
 *               offset test (rx_badoff) and the segment record (seq, ack,
 *               window, urgent pointer, flags, length)
 *
 * The TCP PCB vector is a second cndp_pcb_tbl_t (the reference keeps
 * stk->tcp->tcp_hd apart from udp_hd), made and changed with cndp_pcb_create /
 * add / del / count / lookup of cndp_l4.h; opt_flag is ignored, a TCP checksum
 * is always verified.  The stage runs after cndp_gpu_udp_input of the same batch
 * (whose table had tcp_enabled), on that call's l4edge.
 *
 * Left to the host, which has the mbuf: the two tests that need its data_len
 * (pktmbuf_adjust failing and rx_short, cnet_tcp.c:3371-3384; the batch carries
 * no per-frame length), tcp_strip_ip_options (it rewrites the frame), and
 * everything from "Segment Arrives" on: TCBs, options, reassembly, timers, RST
 * generation.  Errors are negative errno values.  Over pktmbuf_t bursts the
 * node is a mode of the mbuf queue (cndp_mqtcp.h), which has the mbuf and makes
 * the data_len tests as well.
 */
#ifndef CNDP_TCP_H
#define CNDP_TCP_H

#include <stdint.h>

#include "cndp_l4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cndp_pcb_lookup's results, answered from the table's TCP index (an exact
 * 4-tuple hash and per-port wildcard runs, built when the table changed)
 * instead of a walk of the vector. */
int cndp_pcb_lookup_indexed(cndp_pcb_tbl_t *tbl, const struct cndp_pcb_key *keys, uint32_t n,
                            uint32_t *idx_out);

/* Edges of tcp_input (tcp_input_priv.h:13-18) as CNDP_L4_EDGE(CNDP_L4_NODE_TCP_INPUT, e). */
#define CNDP_L4_NODE_TCP_INPUT 2u
#define CNDP_TCP_INPUT_PKT_DROP 0u
/* The lookup hit, the checksum verified and the header offset is sane: the
 * frame goes on to the host's continuation of cnet_tcp_input with `seg` and
 * `pcb` filled in.  1 is the slot of TCP_INPUT_NEXT_CHNL_RECV, an edge that only
 * the state machine can choose; the stage never claims it has. */
#define CNDP_TCP_INPUT_SEGMENT 1u
#define CNDP_TCP_INPUT_PKT_PUNT 2u

#define CNDP_TCP_STAT_SEGMENT 0 /* handed to the state machine */
#define CNDP_TCP_STAT_NOMATCH 1 /* drop or punt: no PCB */
#define CNDP_TCP_STAT_CKSUM 2   /* drop: checksum (total_length < IHL * 4 included) */
#define CNDP_TCP_STAT_BADOFF 3  /* drop: rx_badoff */
#define CNDP_TCP_STAT_RSVD 4    /* always 0 */
#define CNDP_TCP_NSTATS 5

/* struct seg_entry's fields that come from the frame alone (cnet_tcp.c:3393-3414),
 * host byte order. */
struct cndp_tcp_seg {
    uint32_t seq;   /* be32toh(sent_seq) */
    uint32_t ack;   /* be32toh(recv_ack) */
    uint16_t wnd;   /* be16toh(rx_win), not scaled */
    uint16_t urp;   /* be16toh(tcp_urp) */
    uint16_t len;   /* total_length - (offset + l3_len) + tcp_syn_fin_cnt[flags & SYN_FIN] in the
                     * reference's own uint16_t arithmetic: it wraps when l3_len + offset >
                     * total_length, which the reference does not test */
    uint8_t flags;  /* tcp_flags & TCP_MASK (0x3f) */
    uint8_t offset; /* (data_off & 0xF0) >> 2: header and options in bytes */
};

/* Device arrays of n elements (stats: CNDP_TCP_NSTATS), optional unless noted. */
struct cndp_tcp_io {
    const uint8_t *sel; /* in: frame i is taken when sel[i] != 0.  NULL = the frames whose
                         * l4edge[i] is CNDP_L4_EDGE(CNDP_L4_NODE_IP4_PROTO, CNDP_IP4_PROTO_TCP),
                         * as cndp_gpu_udp_input left it */
    uint8_t *l4edge;    /* required.  in (sel == NULL) / out: only the taken entries are
                         * overwritten, with CNDP_L4_EDGE(CNDP_L4_NODE_TCP_INPUT, e) */
    uint32_t *pcb;      /* m->userptr as a table index once the checksum verified (SEGMENT, and
                         * the rx_badoff drop, which the reference takes after setting it),
                         * else CNDP_PCB_NONE */
    uint32_t *ports;    /* fport | lport << 16 as in the frame for every taken frame
                         * (tcp_input.c:91-92 stores them before the lookup), else 0 */
    struct cndp_tcp_seg *seg; /* 16-byte aligned; all zero unless the edge is SEGMENT */
    uint16_t *bin_of;   /* the PCB index on SEGMENT, n_bins for every drop, n_bins + 1 for the
                         * rest: cndp_gpu_bin_partition then gives per-connection lists in
                         * arrival order */
    uint32_t n_bins;    /* >= cndp_pcb_count(tbl) and <= 65533 when bin_of is given;
                         * cndp_gpu_bin_partition takes n_bins <= CNDP_PART_BINS_MAX (every
                         * table's count fits) and returns -EINVAL above it */
    uint64_t *stats;    /* [CNDP_TCP_NSTATS], CNDP_TCP_STAT_*, accumulated (+=) */
};

/* Enqueue tcp_input over the taken frames of `b`.  b gives the frame layout
 * (slab, slab_len, stride / offsets, data_off, n) and b->rxmeta (required): the
 * IPv4 header is read at mtod = frame + l2_len, the TCP header at mtod +
 * l3_len.  pcb, ports, seg and bin_of are written for all n frames, with the
 * values above for a frame that is not taken.  Bytes at or past slab + slab_len
 * read as zero, whatever the lengths in the frame say.  The table's punt flag
 * (cndp_pcb_set_flags) chooses pkt_punt or pkt_drop for a frame without a PCB.
 * The call returns without waiting for the kernels; a table changed since the
 * last call is copied to its device mirror first, and that copy is waited for.
 * Calls on one table are serialised and ordered across streams.  b->n == 0
 * brings the mirror up to date and launches nothing.  -EINVAL: a NULL argument,
 * a missing slab, rxmeta or l4edge, a seg that is not 16-byte aligned, a slab_len
 * of 2^63 or more, an n_bins outside the range above, or a table already
 * mirrored on another device; -ENOMEM, -ENODEV, -EIO as for cndp_gpu_udp_input. */
int cndp_gpu_tcp_input(cndp_gpu_ctx_t *ctx, cndp_pcb_tbl_t *tbl, const struct cndp_batch *b,
                       const struct cndp_tcp_io *io, void *stream);

#ifdef __cplusplus
}
#endif
#endif

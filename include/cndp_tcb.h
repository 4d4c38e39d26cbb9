/*
 * cndp_tcb.h -- the first two per-frame steps of "Segment Arrives" on MI355X,
 * for the frames cndp_gpu_tcp_input (cndp_tcp.h) left on tcp_input's SEGMENT
 * edge (CNDP v25.08.0, lib/cnet/tcp/cnet_tcp.c):
 *
 *   :3425-3460   the TCB tests in front of the state machine: no TCB (the host
 *                sends the RST), a TCB in TCPS_CLOSED, and the window scaling
 *   tcp_do_options, :1179-1279, for every segment that carries options
 *   the header-prediction entry test, :3479-3482, and the branch tests inside
 *   tcp_header_prediction, :3214-3281: is the segment a pure in-window ACK,
 *   in-order data, or work for do_segment_arrives
 *
 * Both steps are state-free once the connection's variables are visible: the
 * host keeps a snapshot of what they read (struct cndp_tcb) per PCB index, in a
 * table that lives beside the cndp_pcb_tbl_t holding the TCP vector.  The stage
 * reads the snapshot and changes nothing: the TCB updates (snd_una, ts_recent,
 * rcv_nxt, timers), reassembly, RST generation and do_segment_arrives stay with
 * the host, which continues from `opt` and `verdict`.
 *
 * More than one segment of a connection in a batch: the frame with the lowest
 * index among a PCB's taken frames carries CNDP_TCPSEG_FIRST.  For it the
 * snapshot is the TCB the reference would have met, and its verdict is the
 * reference's.  Every later frame of that PCB is judged against the SAME
 * snapshot: the stage does not simulate the TCB updates the earlier frames cause
 * (_process_data advances rcv_nxt by the mbuf's data_len, which the batch does
 * not carry), so its verdict is a hint that the host re-checks after it has
 * applied the earlier frames.  `opt` does not depend on TCB state a segment
 * changes and is exact for every frame, up to max_mss, snd_scale and `now`.
 *
 * Errors are negative errno values.
 */
#ifndef CNDP_TCB_H
#define CNDP_TCB_H

#include <stdint.h>

#include "cndp_tcp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tcb_state_t, cnet_tcp.h:123-136 */
#define CNDP_TCPS_FREE 0u
#define CNDP_TCPS_CLOSED 1u
#define CNDP_TCPS_LISTEN 2u
#define CNDP_TCPS_SYN_SENT 3u
#define CNDP_TCPS_SYN_RCVD 4u
#define CNDP_TCPS_ESTABLISHED 5u
#define CNDP_TCPS_CLOSE_WAIT 6u
#define CNDP_TCPS_FIN_WAIT_1 7u
#define CNDP_TCPS_CLOSING 8u
#define CNDP_TCPS_LAST_ACK 9u
#define CNDP_TCPS_FIN_WAIT_2 10u
#define CNDP_TCPS_TIME_WAIT 11u

#define CNDP_TCB_REASS_EMPTY 1u /* vec_len(tcb->reassemble) == 0 */

/* What the two steps read of a struct tcb_entry and its channel, host byte order. */
struct cndp_tcb {
    uint32_t rcv_nxt, snd_una, snd_nxt, snd_max;
    uint32_t snd_wnd, snd_cwnd, ts_recent, last_ack_sent;
    uint32_t rcv_space; /* cb_space(&ch->ch_rcv) */
    uint16_t max_mss;
    uint8_t state;      /* CNDP_TCPS_* */
    uint8_t snd_scale;  /* the shift count is snd_scale & 31 */
    uint8_t flags;      /* CNDP_TCB_REASS_EMPTY; other bits are not kept */
    uint8_t rsvd[7];    /* not kept */
};

typedef struct cndp_tcb_tbl cndp_tcb_tbl_t;

/* A TCB table beside `pcb_tbl` (which must outlive it), one slot per PCB index
 * the PCB table can hold.  A PCB index that was never set has no TCB
 * (pcb->tcb == NULL).  -EINVAL, -ENOMEM. */
int cndp_tcb_tbl_create(cndp_pcb_tbl_t *pcb_tbl, cndp_tcb_tbl_t **out);
void cndp_tcb_tbl_destroy(cndp_tcb_tbl_t *t);
/* -EINVAL for NULL, idx >= cndp_pcb_count(pcb_tbl) or state > 11; -ENOENT for a
 * PCB that was deleted: cnet_pcb_free zeroes the entry, its tcb pointer
 * included, so cndp_pcb_del also takes the index's TCB away, and an index is
 * never handed out twice (cndp_l4.h). */
int cndp_tcb_set(cndp_tcb_tbl_t *t, uint32_t idx, const struct cndp_tcb *tcb);
/* pcb->tcb = NULL.  -EINVAL as above, -ENOENT when the index has no TCB. */
int cndp_tcb_clear(cndp_tcb_tbl_t *t, uint32_t idx);
/* The snapshot as it was set (flags masked, rsvd zero).  -EINVAL, -ENOENT. */
int cndp_tcb_get(cndp_tcb_tbl_t *t, uint32_t idx, struct cndp_tcb *out);

/* seg_entry.sflags, cnet_tcp.h:320-325 */
#define CNDP_SEG_TS_PRESENT 0x8000u
#define CNDP_SEG_MSS_PRESENT 0x4000u
#define CNDP_SEG_WS_PRESENT 0x2000u
#define CNDP_SEG_SACK_PERMIT 0x1000u
#define CNDP_SEG_REQ_SCALE 0x000fu

/* What tcp_do_options and :3459-3460 leave in the seg_entry.  All zero unless
 * the verdict is SLOW or one of PRED_*. */
struct cndp_tcp_opt {
    uint32_t ts_val, ts_ecr;
    uint32_t wnd;    /* seg.wnd << snd_scale unless SYN is set */
    uint16_t mss;
    uint16_t sflags; /* CNDP_SEG_* | req_scale in bits 0-3 */
};

/* verdict[i] & CNDP_TCPSEG_VERDICT, in the reference's order of tests */
#define CNDP_TCPSEG_NONE 0u      /* frame not taken */
#define CNDP_TCPSEG_RESET 1u     /* the PCB has no TCB (:3425): the host sends the RST */
#define CNDP_TCPSEG_CLOSED 2u    /* state == TCPS_CLOSED: drop */
#define CNDP_TCPSEG_BADOPT 3u    /* tcp_do_options returned non-zero: drop */
#define CNDP_TCPSEG_SLOW 4u      /* the entry test of :3479-3482 fails: do_segment_arrives */
#define CNDP_TCPSEG_PRED_ACK 5u  /* entry test holds, seg.len == 0, the ACK conditions of :3227-3228 hold */
#define CNDP_TCPSEG_PRED_DATA 6u /* entry test holds, seg.len != 0, ack == snd_una, reassembly empty,
                                  * seg.len <= rcv_space (:3264-3265) */
#define CNDP_TCPSEG_PRED_NONE 7u /* entry test holds, neither branch taken */
#define CNDP_TCPSEG_NSTATS 8
#define CNDP_TCPSEG_VERDICT 0x0fu
#define CNDP_TCPSEG_TS_UPDATE 0x40u /* the timestamp update of :3214-3218 would fire; only with PRED_* */
#define CNDP_TCPSEG_FIRST 0x80u     /* the first taken frame, in batch order, of its PCB (see above) */

/* Arrays of n elements (stats: CNDP_TCPSEG_NSTATS); device memory for
 * cndp_gpu_tcp_segment, host memory for cndp_tcp_segment_host.  The inputs are
 * read only. */
struct cndp_tcpseg_io {
    const uint8_t *sel;    /* in: frame i is taken when sel[i] != 0.  NULL = the frames whose l4edge[i]
                            * is CNDP_L4_EDGE(CNDP_L4_NODE_TCP_INPUT, CNDP_TCP_INPUT_SEGMENT).  Either
                            * way a frame whose pcb[i] is not an index of the table is not taken. */
    const uint8_t *l4edge; /* in: cndp_gpu_tcp_input's; required when sel == NULL */
    const uint32_t *pcb;   /* in, required: cndp_gpu_tcp_input's */
    const struct cndp_tcp_seg *seg; /* in, required, 16-byte aligned: cndp_gpu_tcp_input's */
    struct cndp_tcp_opt *opt;       /* out, required, 16-byte aligned */
    uint8_t *verdict;               /* out, required: CNDP_TCPSEG_* | TS_UPDATE | FIRST */
    uint64_t *stats;                /* optional: one counter per verdict value (NONE counts the frames
                                     * not taken), accumulated (+=) */
};

/* Enqueue the stage over the taken frames of `b`, after cndp_gpu_tcp_input of the
 * same batch on the same stream.  b gives the frame layout and b->rxmeta
 * (required) as for cndp_gpu_tcp_input: the options are read at mtod + l3_len +
 * 20.  `now` stands for stk_get_timer_ticks().  opt and verdict are written for
 * all n frames.  Bytes at or past slab + slab_len read as zero; the parser's one
 * read outside the header (the length byte of a known option kind that is the
 * header's last byte) is bounded by that rule.  The call returns without waiting
 * for the kernels; TCBs changed since the last call (PCB deletes included) are
 * copied to the device mirror first, and that copy is waited for.  Calls on one
 * table are serialised and ordered across streams.  b->n == 0 brings the mirror
 * up to date and launches nothing.  -EINVAL: a NULL argument, a missing slab,
 * rxmeta, pcb, seg, opt, verdict or (sel == NULL) l4edge, a seg or opt that is
 * not 16-byte aligned, a slab_len of 2^63 or more, or a table already mirrored
 * on another device; -ENOMEM, -ENODEV, -EIO as for cndp_gpu_tcp_input. */
int cndp_gpu_tcp_segment(cndp_gpu_ctx_t *ctx, cndp_tcb_tbl_t *t, const struct cndp_batch *b,
                         const struct cndp_tcpseg_io *io, uint32_t now, void *stream);

/* The same rule on the calling thread over host memory (b->slab, b->offsets,
 * b->rxmeta and io's arrays are host pointers): the CPU baseline, and the rule's
 * test on a machine without a GPU.  -EINVAL as above. */
int cndp_tcp_segment_host(cndp_tcb_tbl_t *t, uint32_t now, const struct cndp_batch *b,
                          const struct cndp_tcpseg_io *io);

#ifdef __cplusplus
}
#endif
#endif

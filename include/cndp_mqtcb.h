/*
 * cndp_mqtcb.h -- cnet's tcp_input node, the opening of cnet_tcp_input and what
 * follows it up to the TCP state machine (CNDP v25.08.0 built with enable_tcp,
 * lib/cnet/tcp/cnet_tcp.c): the TCB tests of :3425-3460, tcp_do_options
 * (:1179-1279) and the header-prediction tests (:3479-3482, :3214-3281), as one
 * mode of the asynchronous mbuf queue (cndp_gpu_mq_*, cndp_gpu.h), and the same
 * on the calling thread (cndp_tcp_segment_node_host).  It is CNDP_MQ_TCP_INPUT
 * (cndp_mqtcp.h) with cndp_gpu_tcp_segment's rule (cndp_tcb.h) behind it: the
 * queue looks each mbuf up in a TCP PCB table, and judges every segment that
 * survives against the TCB snapshot the cndp_tcb_tbl_t beside that table holds.
 *
 * A queue made here is driven by cndp_gpu_mq_submit / _flush / _poll / _wait /
 * _pending / _stat / _free as every other one, by cndp_gpu_mq_poll_tcp, and by
 * cndp_gpu_mq_poll_tcpseg and cndp_gpu_mq_tcp_now.
 *
 * Steps 1-10 of cndp_mqtcp.h hold here word for word, per mbuf: the mbuf at
 * submit, the edges (node CNDP_MQ_NODE_TCP_INPUT, CNDP_MQ_EDGE_L4_CKSUM,
 * CNDP_MQ_EDGE_TCP_IPOPT), the mbuf header and metadata edits poll makes, the
 * readable bytes, CNDP_MQ_EDGE_NONE, the segment record and the counters
 * CNDP_MQ_STAT_TCP_SEGMENT ... _TCP_IPOPT.  Then:
 *  11. An mbuf is judged when its final edge, masked with CNDP_MQ_EDGE_TCP_MASK,
 *      is SEGMENT and its record is not the zeroed one.  That includes an mbuf
 *      with CNDP_MQ_EDGE_TCP_IPOPT set -- the batch chain cndp_gpu_tcp_input ->
 *      cndp_gpu_tcp_segment judges it too -- and leaves out the IPOPT mbuf whose
 *      header offset is below 20 or past total_length, whose record is all zero.
 *  12. A judged mbuf gets `opt` and `verdict` as cndp_tcb.h defines them
 *      (cnet_tcp.c:3425-3460, tcp_do_options, :3479-3482, :3214-3281), from the
 *      matched PCB's TCB snapshot, its segment record, `now`
 *      (cndp_gpu_mq_tcp_now) and, when the header offset is above 20, the option
 *      bytes at mtod + l3_len + 20 of the mbuf as submitted.  Bytes past the
 *      readable ones read as zero, the parser's one read at opt_end (the length
 *      byte of a known option kind that is the header's last byte) included.
 *      Every other mbuf gets CNDP_TCPSEG_NONE and an all-zero opt.
 *  13. CNDP_TCPSEG_FIRST is set on the judged mbuf with the lowest index among
 *      its PCB's judged mbufs of one launched batch.
 *
 * Defined by this build:
 *  - The batch takes the place of cndp_gpu_tcp_segment's "one call": a batch is
 *    what CNDP_MQ_STAT_BATCHES counts -- conf.batch mbufs, or fewer where
 *    cndp_gpu_mq_flush or the queue's delay rule launched it -- and for
 *    cndp_tcp_segment_node_host the call's n mbufs.  Burst boundaries decide
 *    nothing; batch boundaries decide FIRST and nothing else.
 *  - A batch is judged against the TCB table as it stood when the batch was
 *    launched; cndp_tcb_set / _clear and cndp_pcb_del reach the batches launched
 *    after them.  A FIRST verdict is the reference's only if the snapshot was
 *    current at that moment.  With more than one batch in flight the host has
 *    not yet applied the earlier batches when a later one is launched: a
 *    connection that had segments in an earlier batch not yet applied is
 *    re-checked by the host, FIRST or not, as every non-FIRST segment is
 *    (cndp_tcb.h).
 *  - Which mbufs survive steps 1 and 7-8 is known on the lcore only (the
 *    metadata hook, the mbuf's lengths): submit calls conf->metadata once per
 *    mbuf and hands the device three bits, so that FIRST lands on the first
 *    surviving mbuf.  poll makes every edit and decides every edge as
 *    CNDP_MQ_TCP_INPUT does; an mbuf that poll drops although the device judged
 *    it (the hook answering differently at poll, a header changed while the mbuf
 *    was in flight) has its opt and verdict cleared.  The opposite disagreement is
 *    the caller's to avoid and is not repaired: an mbuf the device left out
 *    (the hook answered NULL at submit) that poll then sends on SEGMENT comes back
 *    with a standing record, CNDP_TCPSEG_NONE and a zero opt, counts under no
 *    CNDP_MQ_STAT_TSEG_* key -- the sum rule below is short by it -- and FIRST may
 *    sit on a later mbuf of its PCB.  A hook must answer the same for an mbuf at
 *    submit and at poll.
 *  - A changed TCB is copied to the device on the queue's stream from a pinned
 *    snapshot taken at launch; no launch waits for the stream.  The table's first
 *    use on a device allocates the mirror and may wait.
 *  - The device returns one 64-byte record per mbuf into pinned memory: mode 9's
 *    32 bytes, opt, and the verdict in a word of its own.
 *
 * poll counts a judged mbuf under its verdict value, keys CNDP_MQ_STAT_TSEG_RESET
 * ... _TSEG_PRED_NONE; their sum is CNDP_MQ_STAT_TCP_SEGMENT + _TCP_IPOPT less
 * the IPOPT mbufs with a zeroed record.  On a queue of another mode
 * cndp_gpu_mq_stat answers -EINVAL for them, and on this one for the keys of
 * cndp_mqtx.h.
 */
#ifndef CNDP_MQTCB_H
#define CNDP_MQTCB_H

#include <stdint.h>

#include "cndp_mqtcp.h"
#include "cndp_tcb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_MQ_TCP_SEGMENT 11u /* CNDP_MQ_TCP_INPUT's node + :3425-3460, tcp_do_options, the prediction tests */

/* one per verdict value 1-7: key = CNDP_MQ_STAT_TSEG_RESET + (verdict & CNDP_TCPSEG_VERDICT) - 1 */
#define CNDP_MQ_STAT_TSEG_RESET 32
#define CNDP_MQ_STAT_TSEG_CLOSED 33
#define CNDP_MQ_STAT_TSEG_BADOPT 34
#define CNDP_MQ_STAT_TSEG_SLOW 35
#define CNDP_MQ_STAT_TSEG_PRED_ACK 36
#define CNDP_MQ_STAT_TSEG_PRED_DATA 37
#define CNDP_MQ_STAT_TSEG_PRED_NONE 38

/* A queue in mode CNDP_MQ_TCP_SEGMENT over `tbl` and `tcbs`, which must both
 * outlive it; tcbs must have been created over tbl (cndp_tcb_tbl_create), else
 * -EINVAL.  Otherwise the argument rules are cndp_gpu_mq_create_tcp_input's
 * (cndp_mqtcp.h), -EINVAL for a table already bound to another device being one
 * of them, for either table.  The queue reads both device mirrors by the
 * protocols cndp_gpu_tcp_input and cndp_gpu_tcp_segment use, so those may run on
 * the same tables.  Every other create call answers -EINVAL for this mode. */
int cndp_gpu_mq_create_tcp_segment(cndp_gpu_ctx_t *ctx, const struct cndp_mq_conf *conf,
                                   cndp_pcb_tbl_t *tbl, cndp_tcb_tbl_t *tcbs, cndp_gpu_mq_t **out);

/* stk_get_timer_ticks() for the batches launched after the call (0 until set).
 * -EINVAL: NULL, or a queue of another mode. */
int cndp_gpu_mq_tcp_now(cndp_gpu_mq_t *q, uint32_t now);

/* cndp_gpu_mq_poll_tcp, and opts[k], verdicts[k] of mbufs[k].  Any of segs, opts
 * and verdicts may be NULL.  -EINVAL as cndp_gpu_mq_poll, and on a queue of
 * another mode.  cndp_gpu_mq_poll and cndp_gpu_mq_poll_tcp work on this mode and
 * drop what they do not return; the three may be interleaved. */
int cndp_gpu_mq_poll_tcpseg(cndp_gpu_mq_t *q, void **mbufs, uint16_t *edges, struct cndp_tcp_seg *segs,
                            struct cndp_tcp_opt *opts, uint8_t *verdicts, uint32_t max);

/* The same on the calling thread over the tables' host images: one batch of
 * n <= 256 mbufs, the same mbuf header and metadata edits, the same edges,
 * records, opts and verdicts as the queue's for a batch of these n mbufs.  segs,
 * opts and verdicts may be NULL.  readable_end, stage_max and metadata as
 * cndp_tcp_input_node_host has them.  -EINVAL: tbl or tcbs NULL, tcbs not made
 * over tbl, n above 256, or n != 0 with mbufs or edges NULL; -ENOMEM. */
int cndp_tcp_segment_node_host(cndp_pcb_tbl_t *tbl, cndp_tcb_tbl_t *tcbs, uint32_t now, void *const *mbufs,
                               uint32_t n, uint16_t *edges, struct cndp_tcp_seg *segs, struct cndp_tcp_opt *opts,
                               uint8_t *verdicts, const void *readable_end, uint32_t stage_max,
                               void *(*metadata)(const void *m));

#ifdef __cplusplus
}
#endif
#endif

/*
 * cndp_mqfwd.h -- cndpfwd's fwd, l3fwd and ACL forwarding modes as modes of the
 * asynchronous mbuf queue (cndp_gpu_mq_*, cndp_gpu.h): the layer that takes
 * pktmbuf_t bursts the way cndpfwd's thread_func loop hands them out
 * (CNDP v25.08.0, examples/cndpfwd/main.c, acl-func.c).  The per-frame rules are
 * those of cndp_cfwd.h and cndp_acl.h; the queue runs them on each mbuf's frame
 * at pktmbuf_mtod, in place over PCIe (zero-copy, conf.umem) or on a staged copy
 * of the bytes a mode reads, whose changed bytes poll copies back.
 *
 * A queue made here is driven by cndp_gpu_mq_submit / _flush / _poll / _wait /
 * _pending / _stat / _free as every other one.
 *
 * Edge of each mbuf poll returns:
 *   CNDP_MQ_CFWD_FWD, _L3FWD   tx_lport (0..255), with CNDP_MQ_EDGE_ECHO OR-ed in
 *                              when the target port was unknown and the frame
 *                              goes back to conf.lport (the incoming port)
 *   CNDP_MQ_ACL_FWD            a forwarded frame: tx_lport (the reference counts
 *                              no echo here, so the bit is never set); else
 *                              CNDP_MQ_EDGE_ACL_DENY or _ACL_PREFILTER, which
 *                              cndpfwd frees
 *   zero-copy, an mbuf or frame outside every registered region:
 *                              CNDP_MQ_EDGE_NONE, the frame untouched
 *
 * Frame edits are exactly those of cndp_cfwd_host / cndp_acl_classify_host: FWD
 * bytes 0-11; L3FWD bytes 22, 24-25 and 0-5 (0-11 when echoed); ACL bytes 0-11
 * of forwarded frames and only with CNDP_ACL_F_MAC_SWAP.  Every other frame byte
 * and every byte of the mbuf header keeps its value.  ACL's link-length test
 * uses m->data_len as the host reads it at submit.  Bytes past what is readable
 * read as zero and are never written: zero-copy, past the end of the frame's
 * registered region; staged, past buf_len - data_off.
 *
 * Counters: none on the device.  cndp_gpu_mq_poll counts the five keys below
 * from the edges of the mbufs it returns, so they are exact once
 * cndp_gpu_mq_pending is 0; CNDP_MQ_EDGE_NONE mbufs count nowhere, and a key of
 * another mode's family reads 0.
 */
#ifndef CNDP_MQFWD_H
#define CNDP_MQFWD_H

#include <stdint.h>

#include "cndp_acl.h"
#include "cndp_cfwd.h"
#include "cndp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_MQ_CFWD_FWD 4u   /* _fwd_test,   main.c:164-206 */
#define CNDP_MQ_CFWD_L3FWD 5u /* _l3fwd_test, main.c:257-314 */
#define CNDP_MQ_ACL_FWD 6u    /* acl_fwd_test, acl-func.c:310-402 */

#define CNDP_MQ_EDGE_ECHO 0x0100u          /* fwd / l3fwd: OR-ed into the edge of a frame sent back to in_lport */
#define CNDP_MQ_EDGE_ACL_DENY 0xFFFCu      /* acl: freed, acl_deny */
#define CNDP_MQ_EDGE_ACL_PREFILTER 0xFFFBu /* acl: freed, acl_prefilter_drop */

#define CNDP_MQ_STAT_FORWARD 3 /* fwd / l3fwd: frames sent to the port p[5] / the FIB named */
#define CNDP_MQ_STAT_ECHO 4    /* fwd / l3fwd: frames sent back to in_lport */
#define CNDP_MQ_STAT_ACL_PREFILTER 5
#define CNDP_MQ_STAT_ACL_DENY 6
#define CNDP_MQ_STAT_ACL_PERMIT 7

struct cndp_mq_fwd {
    struct cne_fib *fib;    /* L3FWD: 8-byte entries (cndp_cfwd_fib_create / DIR24_8_8B); else NULL */
    cndp_acl_tbl_t *acl;    /* ACL_FWD: a table with an image; else NULL */
    uint32_t acl_mode;      /* CNDP_ACL_STRICT / _PERMISSIVE */
    uint32_t acl_flags;     /* CNDP_ACL_F_MAC_SWAP or 0 */
    uint64_t lport_mask[4]; /* the ports jcfg_lport_by_index knows */
};

/* A queue in one of the three modes above; conf->lport is the incoming port.
 * The FIB and the ACL table must outlive the queue; routes added or deleted and
 * images built between batches reach the batches launched after them.  A batch
 * launched while the table has no image (a failed build) fails like any other
 * launch: poll returns it with every edge CNDP_MQ_EDGE_NONE and the next submit
 * returns -ENOENT.
 * -EINVAL: a NULL argument, a mode outside 4-6, any conf->flags bit, conf->lport
 * above 255, L3FWD without a FIB or with one of another entry width, ACL_FWD
 * without a table or with an unknown acl_mode / acl_flags, and what
 * cndp_gpu_mq_create answers for batch, depth, stage_max and umem.  -ENOENT: an
 * ACL table without an image.  cndp_gpu_mq_create itself answers -EINVAL for
 * these modes: it has no tables to use. */
int cndp_gpu_mq_create_fwd(cndp_gpu_ctx_t *ctx, const struct cndp_mq_conf *conf, const struct cndp_mq_fwd *fwd,
                           cndp_gpu_mq_t **out);

#ifdef __cplusplus
}
#endif
#endif

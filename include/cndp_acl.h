/*
 * cndp_acl.h -- the ACL forwarding mode of examples/cndpfwd on MI355X
 * (CNDP v25.08.0, examples/cndpfwd/acl-func.c): the rule table, the classify
 * and the permit / deny decision of acl_fwd_test, one frame per lane.
 *
 *   :103-109, :165-185   a rule is {src_addr, src_msk, dst_addr, dst_msk, deny}:
 *                        addresses in host order, masks are prefix lengths
 *                        0..32 (:540-547), the proto field is always 0/0,
 *                        priority = CNE_ACL_MAX_PRIORITY - idx and userdata =
 *                        idx + (deny ? 0xf0000000 : 1)
 *   :145-163             at most MAX_ACL_RULE_NUM rules, -ENOSPC beyond
 *   :604-651             fwd_acl_build: rules take effect only here, in a fresh
 *                        context made of the whole table; a failed build leaves
 *                        no usable context
 *   :404-484             add_init_rules, the default set of 4226 rules
 *   :244-282, :284-308   validate_ipv4_pkt over the header at mtod + 14
 *   :310-402             acl_fwd_test: classify at mtod + 14 + 9, then forward
 *                        or free, MAC_SWAP, the three counters
 *
 * cne_acl_classify returns the userdata of the highest-priority rule that
 * matches, or 0.  With the priorities above that is the rule of the LOWEST
 * index k with ((src ^ rule[k].src_addr) & mask(src_msk)) == 0 and the same for
 * dst: the bits of a rule's address beyond its prefix are ignored, /0 matches
 * every address, of two equal rules the earlier wins.  Only this result is
 * reproduced, not the reference's multi-bit trie: the image behind a table is a
 * tuple space (one hash table per (src_msk, dst_msk) pair in use).
 *
 * Reference quirks kept:
 *   - the ethertype is never looked at: a frame of any type whose byte 14 says
 *     version 4, IHL >= 5 is classified
 *   - the link-length test compares the whole frame's data_len with 20, not 34
 *   - the classify fields sit at fixed frame bytes -- proto 23, src 26-29, dst
 *     30-33 -- whatever the IHL says
 *   - a forwarded frame whose destination MAC's last byte names no existing
 *     port goes back out of the port it came in on
 *
 * Not modelled: the rule parser and the uds commands around the table
 * (:497-602, :653-760), the thread stop / start protocol around a build, the
 * txbuff queues and their flush (the stage hands out tx_lport and bin_of; the
 * host or cndp_gpu_bin_partition makes the per-port lists), pktmbuf_free.
 *
 * Where the reference is undefined this build defines:
 *   - classifying with no built context (the reference would dereference an
 *     unbuilt or NULL ctx): -ENOENT, nothing is written
 *   - header bytes at or past the end of the slab: they read as zero, so a frame
 *     whose byte 14 lies there fails the version test and is prefiltered
 *
 * Errors are negative errno values.
 */
#ifndef CNDP_ACL_H
#define CNDP_ACL_H

#include <stdint.h>

#include "cndp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_ACL_MAX_RULES 100000u           /* MAX_ACL_RULE_NUM */
#define CNDP_ACL_DENY_SIGNATURE 0xf0000000u  /* ACL_DENY_SIGNATURE */
#define CNDP_ACL_INIT_RULES 4226u            /* what cndp_acl_add_init_rules adds */

/* struct acl_rule_desc, host byte order */
struct cndp_acl_rule {
    uint32_t src_addr, dst_addr;
    uint8_t src_msk, dst_msk; /* prefix lengths, 0..32 */
    uint8_t deny;             /* non-zero = deny */
    uint8_t rsvd;             /* not kept */
};

typedef struct cndp_acl_tbl cndp_acl_tbl_t;

/* An empty rule table without an image.  -EINVAL, -ENOMEM. */
int cndp_acl_tbl_create(cndp_acl_tbl_t **out);
void cndp_acl_tbl_destroy(cndp_acl_tbl_t *t);
/* Append a rule; its index is the table's length before the call.  0, -EINVAL
 * for NULL or a mask above 32, -ENOSPC for the rule after CNDP_ACL_MAX_RULES,
 * -ENOMEM. */
int cndp_acl_add(cndp_acl_tbl_t *t, const struct cndp_acl_rule *r);
/* acl_tbl_clear: the table's length becomes 0.  -EINVAL for NULL. */
int cndp_acl_clear(cndp_acl_tbl_t *t);
/* The number of rules in the table (not in the image), or -EINVAL. */
int cndp_acl_count(cndp_acl_tbl_t *t);
/* Rule idx as it was added (deny as 0 / 1, rsvd zero).  -EINVAL for NULL or
 * idx >= the count. */
int cndp_acl_get(cndp_acl_tbl_t *t, uint32_t idx, struct cndp_acl_rule *out);
/* add_init_rules: 100 deny on dst 100.i.0.0/24, 15 deny on src (10+i).0.0.0/8,
 * 15 deny on src 101.0.i.0/24, 4096 allow 210.0.hi.lo/32 -> 110.0.hi.lo/32.
 * Returns 0, or -ENOSPC / -ENOMEM with nothing added. */
int cndp_acl_add_init_rules(cndp_acl_tbl_t *t);
/* fwd_acl_build: make the image lookups read from the whole table as it stands.
 * Rules added or cleared since the last build do not affect lookups until this
 * runs.  On zero rules it returns -EINVAL (cne_acl_build's answer) and leaves
 * the table WITHOUT an image, a previous one included.  -ENOMEM leaves the
 * table without one as well. */
int cndp_acl_build(cndp_acl_tbl_t *t);

#define CNDP_ACL_STRICT 0u     /* forward only what a rule permits */
#define CNDP_ACL_PERMISSIVE 1u /* forward what no rule matches too */
#define CNDP_ACL_F_MAC_SWAP 1u /* MAC_SWAP the forwarded frames in place */

/* verdict[i] */
#define CNDP_ACL_NONE 0u      /* frame not taken (sel[i] == 0) */
#define CNDP_ACL_PREFILTER 1u /* validate_ipv4_pkt failed: freed, acl_prefilter_drop */
#define CNDP_ACL_DENY 2u      /* freed, acl_deny */
#define CNDP_ACL_FORWARD 3u   /* sent to tx_lport[i], acl_permit */
#define CNDP_ACL_LPORT_NONE 0xffu /* tx_lport[i] of a frame that is not forwarded */
#define CNDP_ACL_STAT_PREFILTER_DROP 0
#define CNDP_ACL_STAT_DENY 1
#define CNDP_ACL_STAT_PERMIT 2
#define CNDP_ACL_NSTATS 3

/* Arrays of n elements; device memory for cndp_gpu_acl_fwd, host memory for
 * cndp_acl_classify_host.  The inputs are read only. */
struct cndp_acl_io {
    const uint8_t *sel;     /* in, optional: frame i is taken when sel[i] != 0; NULL = all */
    const uint16_t *len;    /* in, optional: m->data_len per frame; NULL = the link-length test passes */
    uint32_t in_lport;      /* the port the burst came in on, < 256 */
    uint64_t lport_mask[4]; /* bit p set = jcfg_lport_by_index knows port p */
    uint32_t *result;       /* out, optional: acl_results as the reference leaves them; 0 for frames
                             * that were not classified */
    uint8_t *verdict;       /* out, required: CNDP_ACL_* */
    uint8_t *tx_lport;      /* out, optional: the destination port of a forwarded frame, else
                             * CNDP_ACL_LPORT_NONE */
    uint16_t *bin_of;       /* out, optional, input for cndp_gpu_bin_partition: tx_lport for forwarded
                             * frames, n_bins for denied ones, n_bins + 1 for the rest */
    uint32_t n_bins;        /* with bin_of: above in_lport and the highest port of lport_mask, and at
                             * most CNDP_PART_BINS_MAX */
    uint64_t *stats;        /* optional, CNDP_ACL_NSTATS counters, accumulated (+=); a frame that is not
                             * taken counts nowhere */
};

/* Enqueue acl_fwd_test's per-frame work over the frames of `b`, which gives the
 * layout only (n, slab, slab_len, stride / offsets, data_off).  With
 * CNDP_ACL_F_MAC_SWAP the forwarded frames have their MAC addresses swapped in
 * place exactly as cndp_gpu_mac_swap does it; every other byte of the slab is
 * untouched, and without the flag the slab is only read.  The outputs are
 * written for all n frames.  Header bytes at or past slab + slab_len read as
 * zero and no byte there is written.  The call returns without waiting for the
 * kernel; an image built since the last call is copied to the device mirror
 * first, and that copy is waited for.  Calls on one table are serialised and
 * ordered across streams, and the table is bound to the device of its first
 * call.  b->n == 0 brings the mirror up to date and launches nothing.
 * -ENOENT: the table has no image (nothing is written).  -EINVAL: a NULL
 * argument, a missing slab or verdict, an unknown mode or flag, in_lport above
 * 255, an n_bins that breaks the rule above, a slab_len of 2^63 or more, or a
 * table already mirrored on another device; -ENOMEM, -ENODEV, -EIO as for
 * cndp_gpu_tcp_segment. */
int cndp_gpu_acl_fwd(cndp_gpu_ctx_t *ctx, cndp_acl_tbl_t *t, const struct cndp_batch *b, uint32_t mode,
                     uint32_t flags, const struct cndp_acl_io *io, void *stream);

/* The same rule on the calling thread over host memory (b->slab, b->offsets and
 * io's arrays are host pointers; the slab is written only with the swap flag):
 * the CPU baseline, and the rule's test on a machine without a GPU.  -ENOENT,
 * -EINVAL as above. */
int cndp_acl_classify_host(cndp_acl_tbl_t *t, const struct cndp_batch *b, uint32_t mode, uint32_t flags,
                           const struct cndp_acl_io *io);

#ifdef __cplusplus
}
#endif
#endif

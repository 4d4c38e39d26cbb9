/* The ACL table behind include/cndp_acl.h, shared by acl.c (host, plain C) and
 * cndp_acl.hip (the device mirror), and the per-frame rule both apply. */
#ifndef CNDP_ACL_INTERNAL_H
#define CNDP_ACL_INTERNAL_H

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cndp_acl.h"

#if defined(__HIPCC__)
#define ACL_HD __host__ __device__
#else
#define ACL_HD
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Image: u32 words, immutable once built, no pointers inside (offsets are word
 * indices into the image), read as it is by the host and by the device.
 *
 *   header, ACL_HDR_WORDS:   [0] ACL_MAGIC  [1] groups  [2] rules  [3] words of the image
 *   descriptors, ACL_DESC_WORDS each, one per (src_msk, dst_msk) pair in use,
 *   ascending by the lowest rule index of the group:
 *       [0] src mask  [1] dst mask  [2] first word of the group's table
 *       [3] slots - 1 (slots is a power of two, at least twice the group's keys,
 *           four times while that keeps the table within ACL_SPARSE_SLOTS)
 *       [4] the group's lowest rule index  [5] src_msk | dst_msk << 8  [6] keys
 *   tables: slots of ACL_SLOT_WORDS (16 bytes, 16-byte aligned in the image):
 *       [0] src & src mask  [1] dst & dst mask
 *       [2] 0 = empty, else (lowest rule index with this key + 1) | deny << 31
 *       [3] 0
 *   Open addressing, linear probing: at most half the slots are taken, so a
 *   probe sequence always meets an empty slot. */
#define ACL_MAGIC 0x314c4341u
#define ACL_HDR_WORDS 8u
#define ACL_DESC_WORDS 8u
#define ACL_SLOT_WORDS 4u
#define ACL_VAL_DENY 0x80000000u
#define ACL_VAL_IDX1 0x7fffffffu
#define ACL_GROUPS_MAX (33u * 33u)
#define ACL_SPARSE_SLOTS 65536u /* 1 MiB */

struct cndp_acl_tbl {
    pthread_mutex_t lock;        /* serialises changes, builds, the host twin and GPU calls */
    struct cndp_acl_rule *rules; /* the rule vector: acl_rules of acl-func.c */
    uint32_t n, cap;
    uint32_t *img;               /* NULL = no image (never built, or the last build failed) */
    size_t img_words;
    uint64_t gen;                /* bumped by every build */
    void *dev;                   /* the device mirror's state, owned by cndp_acl.hip */
    void (*dev_release)(void *dev);
};

static inline ACL_HD uint32_t acl_mask(uint32_t len) { return len ? 0xffffffffu << (32u - len) : 0u; }

static inline ACL_HD uint32_t acl_hash(uint32_t ks, uint32_t kd)
{
    uint32_t h = ks * 0x9E3779B1u + ((kd << 13) | (kd >> 19)) * 0x85EBCA77u;
    h ^= h >> 16;
    h *= 0xC2B2AE3Du;
    return h ^ (h >> 13);
}

/* Slot (h & slots - 1) of the group's table: key words and value word.  The
 * slot lies inside the table whatever h is. */
static inline ACL_HD void acl_slot(const uint32_t *img, const uint32_t *d, uint32_t h, uint32_t *s0, uint32_t *s1,
                                   uint32_t *v)
{
    const uint32_t *s = img + d[2] + (size_t)(h & d[3]) * ACL_SLOT_WORDS;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t acl_u32x4 __attribute__((ext_vector_type(4)));
    const acl_u32x4 q = *(const acl_u32x4 *)s; /* one 16-byte gather */
    *s0 = q.x, *s1 = q.y, *v = q.z;
#else
    *s0 = s[0], *s1 = s[1], *v = s[2];
#endif
}

/* The probe sequence for key (ks, kd) from slot h + 1 on, after slot h held
 * another key: the entry's value word, or 0.  Bounded by the slot count for an
 * image that is not ours. */
static inline ACL_HD uint32_t acl_probe_on(const uint32_t *img, const uint32_t *d, uint32_t ks, uint32_t kd, uint32_t h)
{
    for (uint32_t step = 0; step < d[3]; step++) {
        uint32_t s0, s1, v;
        acl_slot(img, d, ++h, &s0, &s1, &v);
        if (!v || (s0 == ks && s1 == kd))
            return v;
    }
    return 0u;
}

/* The group's table entry for (src, dst): its value word, or 0.  d is the
 * group's descriptor. */
static inline ACL_HD uint32_t acl_probe(const uint32_t *img, const uint32_t *d, uint32_t src, uint32_t dst)
{
    const uint32_t ks = src & d[0], kd = dst & d[1], h = acl_hash(ks, kd);
    uint32_t s0, s1, v;
    acl_slot(img, d, h, &s0, &s1, &v);
    return !v || (s0 == ks && s1 == kd) ? v : acl_probe_on(img, d, ks, kd, h);
}

/* Nothing in this group or a later one can beat `best` (a value word, 0 = no
 * match yet): its index lies below the group's lowest, and the groups ascend. */
static inline ACL_HD int acl_done(const uint32_t *d, uint32_t best)
{
    return best && (best & ACL_VAL_IDX1) <= d[4];
}

/* of two value words the one of the lower rule index; 0 = none */
static inline ACL_HD uint32_t acl_better(uint32_t a, uint32_t b)
{
    if (!a || !b)
        return a | b;
    return (a & ACL_VAL_IDX1) <= (b & ACL_VAL_IDX1) ? a : b;
}

/* rule->data.userdata of acl_tbl_write_rule, or 0 for no match */
static inline ACL_HD uint32_t acl_userdata(uint32_t v)
{
    return v ? (v & ACL_VAL_IDX1) - 1u + ((v & ACL_VAL_DENY) ? CNDP_ACL_DENY_SIGNATURE : 1u) : 0u;
}

/* cne_acl_classify's result for one packet over the whole image */
static inline ACL_HD uint32_t acl_lookup(const uint32_t *img, uint32_t src, uint32_t dst)
{
    uint32_t best = 0;
    for (uint32_t g = 0; g < img[1]; g++) {
        const uint32_t *d = img + ACL_HDR_WORDS + (size_t)g * ACL_DESC_WORDS;
        if (acl_done(d, best))
            break;
        best = acl_better(best, acl_probe(img, d, src, dst));
    }
    return acl_userdata(best);
}

/* validate_ipv4_pkt: w0 is frame bytes 14-17 as a little-endian load, len_ok
 * the link-length test.  Non-zero = the frame is dropped. */
static inline ACL_HD int acl_prefilter(uint32_t w0, int len_ok)
{
    const uint32_t vi = w0 & 0xffu, tot = ((w0 >> 8) & 0xff00u) | (w0 >> 24);
    return !len_ok || (vi >> 4) != 4u || (vi & 0xfu) < 5u || tot < 20u;
}

/* acl_fwd_test's decision for a classified frame: CNDP_ACL_FORWARD or _DENY */
static inline ACL_HD uint32_t acl_decide(uint32_t res, uint32_t mode)
{
    const int deny = (res & CNDP_ACL_DENY_SIGNATURE) != 0, permit = res != 0;
    return !deny && (mode == CNDP_ACL_PERMISSIVE || permit) ? CNDP_ACL_FORWARD : CNDP_ACL_DENY;
}

/* jcfg_lport_by_index(dst_lport) ? dst_lport : the incoming port */
static inline ACL_HD uint32_t acl_tx_lport(uint32_t dmac5, uint64_t m0, uint64_t m1, uint64_t m2, uint64_t m3,
                                           uint32_t in_lport)
{
    const uint64_t m = dmac5 < 64u ? m0 : dmac5 < 128u ? m1 : dmac5 < 192u ? m2 : m3;
    return (m >> (dmac5 & 63u)) & 1u ? dmac5 : in_lport;
}

/* argument checks shared by the host twin and the GPU call: 0 or -EINVAL */
int acl_io_check(const struct cndp_batch *b, uint32_t mode, uint32_t flags, const struct cndp_acl_io *io);

/* The device mirror's reader protocol (cndp_acl.hip), for a launch that reads
 * the image on `stream` of device `dev`: acl_dev_begin takes t->lock, answers
 * -ENOENT for a table without an image, binds the device, makes `stream` wait
 * for the last reader when that was another stream, brings the mirror up to
 * date and hands out the image's device address.  It returns 0 with t->lock
 * HELD, or a negative errno with the lock released.  acl_dev_end, called after
 * the launch is enqueued (launched != 0) or given up (0), records the reader's
 * end on `stream` for the next call and releases the lock. */
int acl_dev_begin(struct cndp_acl_tbl *t, int dev, void *stream, const uint32_t **img, int *cus);
int acl_dev_end(struct cndp_acl_tbl *t, void *stream, int launched);

#ifdef __cplusplus
}
#endif
#endif

/*
 * cndp_cfwd.h -- the fwd and l3fwd forwarding modes of examples/cndpfwd on
 * MI355X (CNDP v25.08.0, examples/cndpfwd/main.c, l3-fwd.c, main.h;
 * lib/include/cne_inet4.h), one frame per lane.  p is the frame's first byte
 * (pktmbuf_mtod).
 *
 * CNDP_CFWD_L3FWD, _l3fwd_test (main.c:257-314):
 *   main.c:225-237   ipv4_adjust_cksum at p + 14: p[22]-- (0 wraps to 255), and
 *                    with ck = p[24] | p[25] << 8 (the little-endian load)
 *                    c = (ck ^ 0xFFFF) + htobe16(0xFEFF), stored ~(c + (c >> 16))
 *   main.c:282       ip = ntohl(load32(p + 30))
 *   l3-fwd.c:79-93   nh = the FIB's answer for ip; tx_port = (uint16_t)(nh >> 48),
 *                    the MAC is inet_h64tom(nh): octet[0] = bits 47..40 down to
 *                    octet[5] = bits 7..0 (cne_inet4.h:150-159)
 *   main.c:289-296   tx_port names a known lport: MAC_REWRITE writes the six
 *                    octets to p[0..5] (main.h:299; the source MAC stays) and the
 *                    frame goes to tx_port; else MAC_SWAP (main.h:303-315) and it
 *                    goes back to in_lport
 * CNDP_CFWD_FWD, _fwd_test (main.c:164-206):
 *   main.c:181-190   dst_lport = p[5], read before the swap; the target is that
 *                    port when it is known, else in_lport; MAC_SWAP always.  No
 *                    FIB, TTL or checksum.
 *
 * Reference quirks kept:
 *   - L3FWD edits every taken frame: neither the ethertype, the version, the IHL
 *     nor any length is looked at, so an ARP frame loses a "TTL" too
 *   - a FIB miss answers the default 0xFFFFFFFFFFFF, which reads as port 0 with
 *     MAC ff:ff:ff:ff:ff:ff: a miss is broadcast out of port 0 whenever port 0
 *     exists
 *   - MAC_REWRITE leaves the source MAC as it came in
 * Not modelled: l3fwd_fib_lookup's memset(nexthop, 0, n) (l3-fwd.c:83 clears n
 * bytes of an array the lookup then overwrites whole: no visible effect), the
 * txbuff queues and their flush (the stage hands out tx_lport and bin_of; the
 * host or cndp_gpu_bin_partition makes the per-port lists), the rule-string
 * parser of l3fwd_fib_populate (l3-fwd.c:26-76).
 *
 * Where the reference is silent this build defines:
 *   - the known ports are the 256-bit lport_mask; a tx_port of 256 or more is
 *     unknown
 *   - bytes at or past slab + slab_len read as zero and are never written
 *   - offsets must name frames that do not overlap (a frame is bytes 0..33)
 *   - n == 0 brings the FIB's mirror up to date and launches nothing
 *
 * Errors are negative errno values.
 */
#ifndef CNDP_CFWD_H
#define CNDP_CFWD_H

#include <stdint.h>

#include "cndp_fib.h"
#include "cndp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNDP_CFWD_FWD 0u   /* _fwd_test */
#define CNDP_CFWD_L3FWD 1u /* _l3fwd_test */

#define CNDP_CFWD_DEFAULT_NH 0xFFFFFFFFFFFFull /* l3-fwd.c:100 */
#define CNDP_CFWD_MAX_ROUTES (1 << 16)         /* l3-fwd.c:99 */
#define CNDP_CFWD_PORT_MAX 0x7FFFu             /* the highest tx_port a route can carry, see below */
#define CNDP_CFWD_LPORT_NONE 0xFFFFu           /* tx_lport[i] of a frame that is not taken */
#define CNDP_CFWD_STAT_FORWARD 0               /* frames sent to the port the FIB / p[5] named */
#define CNDP_CFWD_STAT_ECHO 1                  /* frames sent back to in_lport */
#define CNDP_CFWD_NSTATS 2

/* l3fwd_fib_init: a CNE_FIB_DUMMY FIB with max_routes = 1 << 16 and default_nh
 * = 0xFFFFFFFFFFFF.  NULL for a NULL name or without memory.  Freed with
 * cne_fib_free. */
struct cne_fib *cndp_cfwd_fib_create(const char *name);
/* l3-fwd.c:64-67: (uint64_t)tx_port << 48 | inet_mtoh64(mac).  0 for a NULL mac. */
uint64_t cndp_cfwd_nexthop(const uint8_t mac[6], uint16_t tx_port);
/* cne_fib_add(fib, ip, depth, cndp_cfwd_nexthop(mac, tx_port)); ip in host
 * order.  -EINVAL for a NULL fib or mac and for tx_port > CNDP_CFWD_PORT_MAX:
 * the image of a DUMMY FIB keeps 63 bits of a next hop (8-byte DIR-24-8 entries
 * give one bit to the extension flag), so the top bit of a higher port would
 * not come back from a lookup.  Otherwise cne_fib_add's result. */
int cndp_cfwd_route_add(struct cne_fib *fib, uint32_t ip, uint8_t depth, const uint8_t mac[6], uint16_t tx_port);

/* Arrays of n elements; device memory for cndp_gpu_cfwd, host memory for
 * cndp_cfwd_host.  The inputs are read only. */
struct cndp_cfwd_io {
    const uint8_t *sel;     /* in, optional: frame i is taken when sel[i] != 0; NULL = all */
    uint32_t in_lport;      /* the port the burst came in on, < 256 */
    uint64_t lport_mask[4]; /* bit p set = jcfg_lport_by_index knows port p */
    uint64_t *nh;           /* out, optional: the FIB's raw answer; 0 in FWD mode and for frames not taken */
    uint16_t *tx_lport;     /* out, required: the port the frame leaves on, CNDP_CFWD_LPORT_NONE for
                             * frames not taken */
    uint8_t *echoed;        /* out, optional: 1 = the target was unknown and the frame goes back to
                             * in_lport (MAC_SWAP in L3FWD mode), else 0 */
    uint16_t *bin_of;       /* out, optional, input for cndp_gpu_bin_partition: tx_lport for taken
                             * frames, n_bins for the rest */
    uint32_t n_bins;        /* with bin_of: above in_lport and the highest port of lport_mask, and at
                             * most CNDP_PART_BINS_MAX */
    uint64_t *stats;        /* optional, CNDP_CFWD_NSTATS counters, accumulated (+=); a frame that is not
                             * taken counts nowhere */
};

/* Enqueue one mode's per-frame work over the frames of `b`, which gives the
 * layout only (n, slab, slab_len, stride / offsets, data_off).  The frames are
 * edited in place: FWD changes bytes 0-11, L3FWD bytes 22, 24-25 and 0-5 (0-11
 * for an echoed frame); every other byte of the slab keeps its value (L3FWD
 * stores bytes 0-31 of a 16-byte aligned frame back whole, the unchanged ones
 * as they were read), and a frame that is not taken is not written at all.
 * The outputs are written for all n frames.  `fib` may be NULL in FWD mode; in
 * L3FWD mode it must have 8-byte entries (a DUMMY FIB or CNE_FIB_DIR24_8_8B).  The call returns without waiting for the kernel;
 * routes added or deleted since the last call are brought to the FIB's device
 * mirror first.  Calls are serialised and ordered across streams per device.
 * -EINVAL: a NULL argument, a missing slab or tx_lport, an unknown mode, a FIB
 * of another entry width, in_lport above 255, an n_bins that breaks the rule
 * above, a slab_len of 2^63 or more; -ENOMEM, -ENODEV, -EIO as for
 * cndp_gpu_acl_fwd. */
int cndp_gpu_cfwd(cndp_gpu_ctx_t *ctx, struct cne_fib *fib, const struct cndp_batch *b, uint32_t mode,
                  const struct cndp_cfwd_io *io, void *stream);

/* The same rule on the calling thread over host memory (b->slab, b->offsets and
 * io's arrays are host pointers): the CPU baseline, and the rule's test on a
 * machine without a GPU.  -EINVAL as above. */
int cndp_cfwd_host(struct cne_fib *fib, const struct cndp_batch *b, uint32_t mode, const struct cndp_cfwd_io *io);

#ifdef __cplusplus
}
#endif
#endif

/* The transmit stage behind include/cndp_tx.h, shared by tx.c (host, plain C)
 * and cndp_tx.hip (the device mirrors). */
#ifndef CNDP_TX_INTERNAL_H
#define CNDP_TX_INTERNAL_H

#include "../../include/cndp_tx.h"
#include "fwd_internal.h"
#include "pcb_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Transmit image of a PCB table (u32 words), rebuilt by tx_pcb_image() when the
 * table changed:
 *   [0] n (the vector's length)  [1] [2] [3] 0
 *   word[n]: TXW_LIVE | TXW_CKSUM (CNDP_UDP_CHKSUM_FLAG) | tos << 16 | ttl << 8 | ip_proto
 * A deleted entry's word is 0.  4 + 4096 words = 16400 bytes at most. */
#define TXI_HDR 4u
#define TXW_LIVE 0x80000000u
#define TXW_CKSUM 0x01000000u
#define TXI_WORDS(n) (TXI_HDR + (size_t)(n))

#define TX_TTL_DEFAULT 64u /* cnet_ipv4.h:32-33 */
#define TX_TOS_DEFAULT 0u

/* Call with tbl->lock held: bring tbl->ximg up to date.  0 or -ENOMEM. */
int tx_pcb_image(struct cndp_pcb_tbl *tbl);

#ifdef __cplusplus
}
#endif
#endif

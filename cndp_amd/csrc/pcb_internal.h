/* The PCB table behind include/cndp_l4.h and include/cndp_tcp.h, shared by pcb.c
 * (host, plain C) and cndp_l4.hip / cndp_tcp.hip (the device mirrors). */
#ifndef CNDP_PCB_INTERNAL_H
#define CNDP_PCB_INTERNAL_H

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/cndp_tcp.h" /* includes cndp_l4.h */
#include "../../include/cndp_mql4.h"
#include "../../include/cndp_mqtcp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCB_F_PUNT 1u
#define PCB_F_TCP 2u

/* Device image (u32 words), rebuilt by pcb_image() when the table changed:
 *   [0] n  [1] H  [2] flags  [3] total words
 *   laddr[n]  faddr[n]  ports[n] (fport | lport << 16)  slots[H]  idxf[(n + 1) / 2]
 * Entries are sorted by (lport, index), so all entries of one local port form a
 * run.  slots is an open-addressed (linear probing, load <= 1/2) map from a
 * local port to the start of its run: PCB_SLOT_VALID | lport << 12 | start;
 * the run ends where ports[j] >> 16 changes.  idxf holds u16 values:
 * the entry's index in vector order | PCB_IDXF_CKSUM when it has
 * CNDP_UDP_CHKSUM_FLAG. */
#define PCB_IMG_HDR 4u
#define PCB_SLOT_VALID 0x80000000u
#define PCB_IDXF_CKSUM 0x8000u
#define PCB_IDXF_IDX 0x0fffu

#if defined(__HIPCC__)
#define PCB_HD __host__ __device__
#else
#define PCB_HD
#endif
static inline PCB_HD uint32_t pcb_port_hash(uint32_t lport, uint32_t H)
{
    return ((lport * 0x9E3779B1u) >> 15) & (H - 1u);
}

struct cndp_pcb_tbl {
    pthread_mutex_t lock;   /* serialises changes, lookups and GPU calls */
    uint32_t max;
    uint32_t count;         /* vector length, deleted entries included */
    uint32_t flags;         /* PCB_F_* */
    struct cndp_pcb_entry *vec;
    uint8_t *closed;        /* 1 = deleted (zeroed, still in the vector) */
    uint64_t gen;           /* bumped by every change */
    uint32_t *img;          /* device image, host copy */
    uint32_t img_words;
    uint64_t img_gen;       /* gen the image was built from (0 = never) */
    void *dev;              /* the device mirror's state, owned by cndp_l4.hip */
    void (*dev_release)(void *dev);
    uint32_t *timg;         /* TCP index image (below), host copy, allocated on first use */
    uint32_t timg_words;
    uint64_t timg_gen;      /* gen the TCP image was built from (0 = never) */
    void *tdev;             /* the TCP stage's device mirror, owned by cndp_tcp.hip */
    void (*tdev_release)(void *tdev);
    /* transmit side (include/cndp_tx.h), kept by tx.c */
    uint8_t *txa;           /* per entry: tos, ttl, ip_proto; allocated on first use */
    uint32_t txa_n;         /* entries of the vector given their defaults so far */
    uint32_t *ximg;         /* transmit image (tx_internal.h), host copy */
    uint64_t ximg_gen;      /* gen the transmit image was built from (0 = never) */
    void *xdev;             /* the transmit stage's device mirror, owned by cndp_tx.hip */
    void (*xdev_release)(void *xdev);
    /* host only (cndp_pcb_user_set, cndp_mql4.h): per entry what udp_input stores in
     * m->userptr, the entry's index by default; max values, never part of an image */
    uint64_t *user;
};

/* Call with tbl->lock held: bring tbl->img up to date.  0 or -ENOMEM. */
int pcb_image(struct cndp_pcb_tbl *tbl);

/* Readers of the image's device mirror (cndp_l4.hip): cndp_gpu_udp_input and the
 * mbuf queue's CNDP_MQ_UDP_INPUT kernel in cndp_gpu.hip.  pcb_dev_begin takes
 * tbl->lock, binds the table to device `dev` (-EINVAL when it is bound to
 * another), orders `stream` after the last reader when that was on another
 * stream, brings the host image and the mirror up to date (a copy is waited
 * for, so the table may change once the lock is dropped) and hands out the
 * mirror's address.  On 0 the lock is held until pcb_dev_end, which records the
 * reader's end on `stream` when `launched` and drops it; on an error it is not. */
int pcb_dev_begin(struct cndp_pcb_tbl *tbl, int dev, void *stream, const uint32_t **img);
int pcb_dev_end(struct cndp_pcb_tbl *tbl, void *stream, int launched);
/* -EINVAL when the table's mirror lives on another device than `dev`, else 0 */
int pcb_dev_check(struct cndp_pcb_tbl *tbl, int dev);

/* ---- ip4_proto + udp_input per frame (cndp_mql4.h): the text the queue's
 * kernel k_mq_udp_input and the host twin cndp_udp_input_node_host both compile */

/* ip4_proto (ip4_proto.c:30-195) on header byte 9 with the table's flags:
 * 0 = on to udp_input, else 1 + the node's edge (drop 0, tcp_input 2) */
static inline PCB_HD uint32_t pcb_ip4_proto(uint32_t proto, uint32_t flags)
{
    if (proto == 17u)
        return 0u;
    return proto == 6u && (flags & PCB_F_TCP) ? 1u + CNDP_IP4_PROTO_TCP : 1u + CNDP_IP4_PROTO_DROP;
}

/* pcb_v4_lookup, BEST_MATCH, answered from the UDP image `img`: the port
 * directory, then a walk of that port's run, which is in vector order, so the
 * first entry with the fewest wildcards wins and an exact match ends the walk.
 * Returns the entry's idxf value (its vector index | PCB_IDXF_CKSUM) or
 * CNDP_PCB_NONE. */
static inline PCB_HD uint32_t pcb_udp_lookup(const uint32_t *img, uint32_t laddr, uint32_t faddr, uint32_t lport,
                                             uint32_t fport)
{
    const uint32_t n = img[0], H = img[1];
    const uint32_t *t_laddr = img + PCB_IMG_HDR, *t_faddr = t_laddr + n, *t_ports = t_faddr + n;
    const uint32_t *slots = t_ports + n;
    const uint16_t *idxf = (const uint16_t *)(slots + H);
    uint32_t s;
    for (uint32_t h = pcb_port_hash(lport, H);; h = (h + 1u) & (H - 1u)) {
        s = slots[h];
        if (!(s & PCB_SLOT_VALID))
            return CNDP_PCB_NONE;
        if (((s >> 12) & 0xffffu) == lport)
            break;
    }
    uint32_t bestw = 3, bestj = 0;
    for (uint32_t j = s & 0xfffu; j < n; j++) {
        const uint32_t pp = t_ports[j];
        if ((pp >> 16) != lport)
            break;
        const uint32_t el = t_laddr[j], ef = t_faddr[j];
        uint32_t w = 0;
        if (el != 0) {
            if (laddr == 0)
                w++;
            else if (el != laddr)
                continue;
        } else if (laddr != 0)
            w++;
        if (ef != 0) {
            if (faddr == 0)
                w++;
            else if (ef != faddr || (pp & 0xffffu) != fport)
                continue;
        } else if (faddr != 0)
            w++;
        if (w < bestw) {
            bestw = w;
            bestj = j;
            if (w == 0)
                break;
        }
    }
    return bestw == 3 ? CNDP_PCB_NONE : (uint32_t)idxf[bestj];
}

/* The folds of cne_ipv4_udptcp_cksum_verify (net/cne_ip.h:131-178, :235-260,
 * :275-349) once the datagram's bytes are summed: S = the sum of its bytes at
 * even offsets + 256 * the sum of those at odd offsets (its little-endian 16-bit
 * words, a last odd byte as a low byte), below 2^32 for every length; faddr /
 * laddr / proto as loaded from the header, L = total_length - IHL * 4.
 * 1 = the verify passes. */
static inline PCB_HD uint32_t pcb_udp_phdr_sum(uint32_t faddr, uint32_t laddr, uint32_t proto, uint32_t L)
{
    uint32_t ph = (faddr & 0xffffu) + (faddr >> 16) + (laddr & 0xffffu) + (laddr >> 16) + ((proto & 0xffu) << 8) +
                  (((L & 0xffu) << 8) | ((L >> 8) & 0xffu));
    ph = (ph >> 16) + (ph & 0xffffu);
    ph = (ph >> 16) + (ph & 0xffffu);
    return ph & 0xffffu;
}

static inline PCB_HD uint32_t pcb_udp_cksum_ok(uint32_t S, uint32_t ph)
{
    S = (S >> 16) + (S & 0xffffu); /* cne_raw_cksum's reduce */
    S = (S >> 16) + (S & 0xffffu);
    S &= 0xffffu;
    uint32_t c = S + ph;           /* + cne_ipv4_phdr_cksum, __ipv4_udptcp_cksum's fold */
    c = ((c >> 16) + (c & 0xffffu)) & 0xffffu;
    return c == 0xffffu;
}

/* pktmbuf_t fields (pktmbuf.h:102-204) and struct cnet_metadata {faddr, laddr}
 * (cnet_meta.h:20-25), two struct in_caddr of 20 bytes (cne_inet.h:37-45) */
#define PCB_MB_BUF_ADDR 8
#define PCB_MB_DATA_OFF 24
#define PCB_MB_BUF_LEN 28
#define PCB_MB_DATA_LEN 30
#define PCB_MB_TX_OFFLOAD 40
#define PCB_MB_USERPTR 56
#define PCB_MD_LADDR 20
#define PCB_AF_INET 2

/* udp_input's writes for one mbuf whose edge is a udp_input edge and whose
 * metadata is md (udp_input.c:95-96, :110-120), on the host: the twin makes
 * them as it goes, cndp_gpu_mq_poll from the device's record.  user is the
 * matched PCB's user value (chnl_recv only). */
static inline void pcb_udp_apply(uint8_t *m, uint8_t *md, uint32_t edge, uint64_t user, uint32_t ports, uint32_t faddr,
                                 uint32_t laddr)
{
    const uint16_t fport = (uint16_t)ports, lport = (uint16_t)(ports >> 16);
    memcpy(md + 2, &fport, 2);
    memcpy(md + PCB_MD_LADDR + 2, &lport, 2);
    if (edge & CNDP_MQ_EDGE_L4_CKSUM)
        return; /* verify < 0: userptr and the header stay */
    if ((edge & 0xffu) != CNDP_UDP_INPUT_CHNL_RECV) {
        memset(m + PCB_MB_USERPTR, 0, 8); /* m->userptr = NULL */
        return;
    }
    memcpy(m + PCB_MB_USERPTR, &user, 8);
    md[0] = md[PCB_MD_LADDR] = PCB_AF_INET; /* in_caddr_copy of the key: the rest of the union is zero */
    md[1] = md[PCB_MD_LADDR + 1] = 4;
    memcpy(md + 4, &faddr, 4);
    memset(md + 8, 0, 12);
    memcpy(md + PCB_MD_LADDR + 4, &laddr, 4);
    memset(md + PCB_MD_LADDR + 8, 0, 12);
    /* pktmbuf_adj_offset(m, l3_len + l4_len), pktmbuf.h:961-971 */
    uint64_t txo;
    uint16_t doff, blen, dlen;
    memcpy(&txo, m + PCB_MB_TX_OFFLOAD, 8);
    memcpy(&doff, m + PCB_MB_DATA_OFF, 2);
    memcpy(&blen, m + PCB_MB_BUF_LEN, 2);
    memcpy(&dlen, m + PCB_MB_DATA_LEN, 2);
    const uint32_t len = (uint32_t)((txo >> 7) & 0x1ffu) + (uint32_t)((txo >> 16) & 0xffu);
    if (len > dlen || len + doff > blen)
        return;
    doff = (uint16_t)(doff + len);
    dlen = (uint16_t)(dlen - len);
    memcpy(m + PCB_MB_DATA_OFF, &doff, 2);
    memcpy(m + PCB_MB_DATA_LEN, &dlen, 2);
}

/* TCP index image (u32 words), rebuilt by pcb_tcp_image() when the table changed.
 * A TCP vector is thousands of connections on a few listening ports, so a key is
 * answered from an exact 4-tuple hash and only falls back to a walk of its
 * port's wildcard entries:
 *   [0] n  [1] HE  [2] flags  [3] total words  [4] HP  [5] fully specified entries
 *   [6] [7] 0
 *   laddr[n]  faddr[n]  ports[n] (fport | lport << 16)  eslots[HE]  pslots[HP]
 *   idx[(n + 1) / 2]  (u16: the entry's index in vector order)
 * Entries are sorted by (lport, fully specified, index): a port's entries form
 * a run, its wildcard entries (a zero address; deleted entries are any/any on
 * port 0) first and in vector order, its fully specified entries after them.
 *   eslots  open-addressed (linear probing, load <= 1/2) over the fully
 *           specified entries' (laddr, faddr, ports): PCB_SLOT_VALID |
 *           tag << 12 | position, tag = the hash's top 19 bits, so a probe that
 *           does not own the slot almost never reads the three entry words.
 *           Equal tuples are inserted once, for their lowest vector index.
 *   pslots  the UDP image's port directory: PCB_SLOT_VALID | lport << 12 | run start.
 * At 4096 entries: 8 + 3 * 4096 + 8192 + 8192 + 2048 = 30728 words = 122912
 * bytes at most (every entry fully specified and on a port of its own),
 * inside the 160 KiB of LDS a block can have; 4096 connections on one port
 * take 8 + 3 * 4096 + 8192 + 2 + 2048 words = 90152 bytes.
 * A slot is one dword because lanes of a wave probe scattered slots: each
 * probe is one 4-byte LDS read whose bank is random, and a wider slot would
 * put more bytes behind the same conflicts. */
#define TCB_IMG_HDR 8u
#define TCB_IMG_WORDS(max, he, hp) (TCB_IMG_HDR + 3u * (max) + (he) + (hp) + ((max) + 1u) / 2u)

static inline PCB_HD uint32_t pcb_tcp_hash(uint32_t laddr, uint32_t faddr, uint32_t ports)
{
    /* every input bit reaches the slot bits and the tag: tuples that differ in
     * one address byte or in a port's byte order must not share a chain */
    uint32_t x = laddr * 0x9E3779B1u;
    x ^= x >> 15;
    x += faddr * 0x85EBCA77u;
    x ^= x >> 13;
    x += ports * 0xC2B2AE3Du;
    x ^= x >> 16;
    x *= 0x27D4EB2Fu;
    x ^= x >> 15;
    return x;
}

/* pcb_v4_lookup, BEST_MATCH, answered from the TCP image `img` (host memory or
 * the kernel's LDS copy): the entry's vector index or CNDP_PCB_NONE.
 *  - key with both addresses non-zero: a fully specified entry matches it only
 *    when all four fields are equal, with 0 wildcards, and every wildcard entry
 *    scores >= 1, so an exact-hash hit (lowest index of equal tuples) is the
 *    linear walk's answer.  Without one, only wildcard entries can match: the
 *    first of the port's wildcard run with the fewest wildcards.
 *  - key with a zero address: fully specified entries match with wildcards too;
 *    the whole run is walked and the least (wildcards, index) wins. */
static inline PCB_HD uint32_t pcb_tcp_lookup(const uint32_t *img, uint32_t laddr, uint32_t faddr,
                                             uint32_t lport, uint32_t fport)
{
    const uint32_t n = img[0], HE = img[1], HP = img[4];
    const uint32_t *t_laddr = img + TCB_IMG_HDR, *t_faddr = t_laddr + n, *t_ports = t_faddr + n;
    const uint32_t *es = t_ports + n, *ps = es + HE;
    const uint16_t *idx = (const uint16_t *)(ps + HP);
    const uint32_t ports = fport | lport << 16;
    const int full_key = laddr != 0 && faddr != 0;
    if (full_key) {
        const uint32_t x = pcb_tcp_hash(laddr, faddr, ports), tag = x >> 13;
        for (uint32_t h = x & (HE - 1u);; h = (h + 1u) & (HE - 1u)) {
            const uint32_t s = es[h];
            if (!(s & PCB_SLOT_VALID))
                break;
            if (((s >> 12) & 0x7ffffu) == tag) {
                const uint32_t j = s & 0xfffu;
                if (t_laddr[j] == laddr && t_faddr[j] == faddr && t_ports[j] == ports)
                    return idx[j];
            }
        }
    }
    uint32_t s;
    for (uint32_t h = pcb_port_hash(lport, HP);; h = (h + 1u) & (HP - 1u)) {
        s = ps[h];
        if (!(s & PCB_SLOT_VALID))
            return CNDP_PCB_NONE;
        if (((s >> 12) & 0xffffu) == lport)
            break;
    }
    uint32_t bestw = 3, besti = CNDP_PCB_NONE;
    for (uint32_t j = s & 0xfffu; j < n; j++) {
        const uint32_t pp = t_ports[j];
        if ((pp >> 16) != lport)
            break;
        const uint32_t el = t_laddr[j], ef = t_faddr[j];
        if (full_key && el != 0 && ef != 0)
            break; /* the run's fully specified part: the exact probe answered for it */
        uint32_t w = 0;
        if (el != 0) {
            if (laddr == 0)
                w++;
            else if (el != laddr)
                continue;
        } else if (laddr != 0)
            w++;
        if (ef != 0) {
            if (faddr == 0)
                w++;
            else if (ef != faddr || (pp & 0xffffu) != fport)
                continue;
        } else if (faddr != 0)
            w++;
        const uint32_t i = idx[j];
        if (w < bestw || (w == bestw && i < besti)) {
            bestw = w;
            besti = i;
            if (full_key && w == 1)
                break; /* wildcard entries are in vector order and none scores 0 */
        }
    }
    return besti;
}

/* Call with tbl->lock held: bring tbl->timg up to date.  0 or -ENOMEM. */
int pcb_tcp_image(struct cndp_pcb_tbl *tbl);

/* Readers of the TCP image's device mirror (cndp_tcp.hip): cndp_gpu_tcp_input
 * and the mbuf queue's CNDP_MQ_TCP_INPUT kernel in cndp_gpu.hip.  The protocol
 * is pcb_dev_begin / _end / _check's, over tbl->tdev and the TCP image. */
int pcb_tdev_begin(struct cndp_pcb_tbl *tbl, int dev, void *stream, const uint32_t **img);
int pcb_tdev_end(struct cndp_pcb_tbl *tbl, void *stream, int launched);
int pcb_tdev_check(struct cndp_pcb_tbl *tbl, int dev);

/* cndp_tcp_input_node_host's per-mbuf walk (pcb.c), for the twins of both TCP
 * queue modes; call with tbl->lock held.  optw: n * PCB_TCP_OPT_WORDS words. */
#define PCB_TCP_OPT_WORDS 11u /* TCB_OPT_WORDS (tcb_internal.h) */
int pcb_tcp_node_walk(struct cndp_pcb_tbl *tbl, void *const *mbufs, uint32_t n, uint16_t *edges,
                      struct cndp_tcp_seg *segs, uint32_t *hits, uint32_t *optw, const void *readable_end,
                      uint32_t stage_max, void *(*metadata)(const void *m));

/* ---- tcp_input per frame (cndp_mqtcp.h): the text the queue's kernel
 * k_mq_tcp_input and the host twin cndp_tcp_input_node_host both compile */

#define PCB_TCP_E(e) CNDP_MQ_EDGE(CNDP_MQ_NODE_TCP_INPUT, e)

/* tcp_input's decision for one frame once its key is looked up (tcp_input.c:95-108)
 * and the record of cnet_tcp_input's opening (cnet_tcp.c:3386-3414), from the words
 * as loaded: hit = pcb_tcp_lookup's answer, flags the image's, w0 the IPv4
 * header's first word, th[1..4] TCP header words 1-4.  Returns the edge that
 * stands unless the sum fails: no match (final), total_length < IHL * 4, where
 * __ipv4_udptcp_cksum sums to 0, which fails (final), else SEGMENT with *L the
 * bytes to sum.  seg[] is struct cndp_tcp_seg as four words, computed for every
 * frame: its offset field is the header length whatever it is, and the host side
 * (pcb_tcp_apply) clears the record where the edge is not SEGMENT. */
static inline PCB_HD uint32_t pcb_tcp_rule(uint32_t hit, uint32_t flags, uint32_t w0, const uint32_t *th, uint32_t l3,
                                           uint32_t *seg, uint32_t *L)
{
    const uint32_t ihl = (w0 & 0xfu) * 4u, tot = ((w0 >> 8) & 0xff00u) | (w0 >> 24);
    const uint32_t offset = (th[3] & 0xf0u) >> 2, fl = (th[3] >> 8) & 0x3fu;
    const uint32_t synfin = (fl & 1u) + ((fl >> 1) & 1u); /* tcp_syn_fin_cnt[flags & SYN_FIN] */
    const uint32_t s = th[1], a = th[2];
    seg[0] = (s >> 24) | ((s >> 8) & 0xff00u) | ((s << 8) & 0xff0000u) | (s << 24);
    seg[1] = (a >> 24) | ((a >> 8) & 0xff00u) | ((a << 8) & 0xff0000u) | (a << 24);
    seg[2] = (((th[3] >> 8) & 0xff00u) | (th[3] >> 24)) | (((th[4] >> 8) & 0xff00u) | (th[4] >> 24)) << 16;
    seg[3] = ((tot - (offset + l3) + synfin) & 0xffffu) | fl << 16 | offset << 24;
    *L = 0;
    if (hit == CNDP_PCB_NONE)
        return PCB_TCP_E((flags & PCB_F_PUNT) ? CNDP_TCP_INPUT_PKT_PUNT : CNDP_TCP_INPUT_PKT_DROP);
    if (tot < ihl)
        return PCB_TCP_E(CNDP_TCP_INPUT_PKT_DROP) | CNDP_MQ_EDGE_L4_CKSUM;
    *L = tot - ihl;
    return PCB_TCP_E(CNDP_TCP_INPUT_SEGMENT);
}

/* Steps 1 and 5-10 of cndp_mqtcp.h for one mbuf on the host: the twin makes them
 * as it goes, cndp_gpu_mq_poll from the device's record.  edge is the frame's
 * decision with the verify's verdict in (pcb_tcp_rule, then CNDP_MQ_EDGE_L4_CKSUM
 * where the sum failed); md is metadata(m) or NULL; user the matched PCB's user
 * value; tot the header's total_length; *seg pcb_tcp_rule's record, cleared here
 * unless the mbuf leaves on SEGMENT.  Returns the mbuf's edge | its
 * CNDP_MQ_STAT_TCP_* key << 16. */
static inline uint32_t pcb_tcp_apply(uint8_t *m, uint8_t *md, uint32_t edge, uint64_t user, uint32_t ports,
                                     uint32_t faddr, uint32_t laddr, uint32_t tot, struct cndp_tcp_seg *seg)
{
    const uint32_t drop = PCB_TCP_E(CNDP_TCP_INPUT_PKT_DROP);
    const uint32_t offset = seg->offset;
    uint32_t out;
    if (!md) { /* tcp_input.c:55-57 */
        out = drop | CNDP_MQ_STAT_TCP_NOMD << 16;
        goto clear;
    }
    {
        const uint16_t fport = (uint16_t)ports, lport = (uint16_t)(ports >> 16);
        memcpy(md + 2, &fport, 2); /* :91-92, before the lookup */
        memcpy(md + PCB_MD_LADDR + 2, &lport, 2);
    }
    if (edge != PCB_TCP_E(CNDP_TCP_INPUT_SEGMENT)) { /* no PCB, or verify < 0: userptr and the header stay */
        out = edge | (uint32_t)((edge & CNDP_MQ_EDGE_L4_CKSUM) ? CNDP_MQ_STAT_TCP_CKSUM : CNDP_MQ_STAT_TCP_NOMATCH) << 16;
        goto clear;
    }
    memcpy(m + PCB_MB_USERPTR, &user, 8);
    md[0] = md[PCB_MD_LADDR] = PCB_AF_INET; /* in_caddr_copy of the key: the rest of the union is zero */
    md[1] = md[PCB_MD_LADDR + 1] = 4;
    memcpy(md + 4, &faddr, 4);
    memset(md + 8, 0, 12);
    memcpy(md + PCB_MD_LADDR + 4, &laddr, 4);
    memset(md + PCB_MD_LADDR + 8, 0, 12);
    {
        uint64_t txo;
        uint16_t doff, blen, dlen;
        memcpy(&txo, m + PCB_MB_TX_OFFLOAD, 8);
        memcpy(&doff, m + PCB_MB_DATA_OFF, 2);
        memcpy(&blen, m + PCB_MB_BUF_LEN, 2);
        memcpy(&dlen, m + PCB_MB_DATA_LEN, 2);
        const uint32_t l3 = (uint32_t)((txo >> 7) & 0x1ffu);
        const int badoff = offset < 20u || offset > tot;
        if (l3 != 20u) { /* IPv4 options: the mbuf stays as cnet_tcp_input is handed it */
            if (badoff)
                memset(seg, 0, sizeof(*seg)); /* what cndp_gpu_tcp_input records for it */
            return edge | CNDP_MQ_EDGE_TCP_IPOPT | CNDP_MQ_STAT_TCP_IPOPT << 16;
        }
        /* pktmbuf_adjust(m, l3_len), pktmbuf.h:955-971 */
        if (l3 > dlen || l3 + doff > blen) {
            out = drop | CNDP_MQ_STAT_TCP_ADJUST << 16;
            goto clear;
        }
        doff = (uint16_t)(doff + l3);
        dlen = (uint16_t)(dlen - l3);
        memcpy(m + PCB_MB_DATA_OFF, &doff, 2);
        memcpy(m + PCB_MB_DATA_LEN, &dlen, 2);
        if (dlen < 20u) { /* rx_short: the adjust stays */
            out = drop | CNDP_MQ_STAT_TCP_SHORT << 16;
            goto clear;
        }
        if (offset <= dlen && offset + doff <= blen) { /* pktmbuf_adj_offset(m, offset): silent when it does not fit */
            doff = (uint16_t)(doff + offset);
            dlen = (uint16_t)(dlen - offset);
            memcpy(m + PCB_MB_DATA_OFF, &doff, 2);
            memcpy(m + PCB_MB_DATA_LEN, &dlen, 2);
        }
        if (badoff) { /* rx_badoff, after the adj_offset */
            out = drop | CNDP_MQ_STAT_TCP_BADOFF << 16;
            goto clear;
        }
    }
    return edge | CNDP_MQ_STAT_TCP_SEGMENT << 16;
clear:
    memset(seg, 0, sizeof(*seg));
    return out;
}

#ifdef __cplusplus
}
#endif
#endif

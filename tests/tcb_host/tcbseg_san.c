/* tcb.c (cndp_tcb_*, cndp_tcp_segment_host) under -fsanitize=address,undefined:
 * TCBs set, read back and cleared across the whole table, PCB deletes taking
 * their TCBs along, and options parsed at the last bytes of heap buffers sized
 * exactly to their frames -- the parser's one read past the header then lies
 * past the allocation, and must come back as zero without being made.  Prints
 * PASS and exits 0; any check that fails exits 1, a sanitizer report aborts. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cndp_amd/csrc/tcb_internal.h"

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            exit(1);                                                 \
        }                                                            \
    } while (0)

#define L2 14u
#define L3 20u
#define SEG_EDGE CNDP_L4_EDGE(CNDP_L4_NODE_TCP_INPUT, CNDP_TCP_INPUT_SEGMENT)

static struct cndp_tcb est(uint32_t k)
{
    struct cndp_tcb t;
    memset(&t, 0, sizeof(t));
    t.rcv_nxt = 1000u + k;
    t.snd_una = 5000u;
    t.snd_nxt = t.snd_max = 6000u;
    t.snd_wnd = 8192u;
    t.snd_cwnd = 10000u;
    t.ts_recent = 500u;
    t.last_ack_sent = 900u;
    t.rcv_space = 100u;
    t.max_mss = 1460u;
    t.state = CNDP_TCPS_ESTABLISHED;
    t.snd_scale = 3;
    t.flags = CNDP_TCB_REASS_EMPTY;
    return t;
}

/* One segment in a heap buffer of exactly L2 + L3 + 20 + optlen + paylen bytes. */
static uint8_t run_one(cndp_tcb_tbl_t *tt, uint32_t pcb, uint8_t flags, const uint8_t *opts, uint32_t optlen,
                       const uint8_t *pay, uint32_t paylen, uint32_t seq, struct cndp_tcp_opt *opt)
{
    const size_t len = L2 + L3 + 20u + optlen + paylen;
    uint8_t *f = malloc(len);
    CHECK(f);
    memset(f, 0xEE, len);
    if (optlen)
        memcpy(f + L2 + L3 + 20u, opts, optlen);
    if (paylen)
        memcpy(f + L2 + L3 + 20u + optlen, pay, paylen);
    uint32_t rx = L2 | L3 << 7, p = pcb;
    uint8_t edge = SEG_EDGE, verdict = 0xAA;
    /* opt and seg on the heap too: 16-byte records, nothing behind them */
    struct cndp_tcp_seg *sg = malloc(sizeof(*sg));
    struct cndp_tcp_opt *o = malloc(sizeof(*o));
    CHECK(sg && o);
    memset(sg, 0, sizeof(*sg));
    sg->seq = seq;
    sg->ack = 5500u;
    sg->wnd = 1024u;
    sg->len = (uint16_t)paylen;
    sg->flags = flags;
    sg->offset = (uint8_t)(20u + optlen);
    struct cndp_batch b;
    memset(&b, 0, sizeof(b));
    b.n = 1;
    b.slab = f;
    b.slab_len = len;
    b.rxmeta = &rx;
    struct cndp_tcpseg_io io;
    memset(&io, 0, sizeof(io));
    io.l4edge = &edge;
    io.pcb = &p;
    io.seg = sg;
    io.opt = o;
    io.verdict = &verdict;
    CHECK(cndp_tcp_segment_host(tt, 1000000u, &b, &io) == 0);
    CHECK(edge == SEG_EDGE && p == pcb && rx == (L2 | L3 << 7));
    *opt = *o;
    free(o);
    free(sg);
    free(f);
    return verdict;
}

int main(void)
{
    cndp_pcb_tbl_t *pt = NULL;
    cndp_tcb_tbl_t *tt = NULL;
    const uint32_t N = CNDP_PCB_MAX_ENTRIES;
    CHECK(cndp_pcb_create(N, &pt) == 0);
    CHECK(cndp_tcb_tbl_create(NULL, &tt) == -EINVAL && cndp_tcb_tbl_create(pt, NULL) == -EINVAL);
    CHECK(cndp_tcb_tbl_create(pt, &tt) == 0);
    struct cndp_tcb t = est(0), g;
    CHECK(cndp_tcb_set(tt, 0, &t) == -EINVAL); /* the vector is empty */
    for (uint32_t i = 0; i < N; i++) {
        struct cndp_pcb_entry e = {0x0100040Au, 0x010012C6u + ((i & 0xffu) << 16), 0x5000, (uint16_t)(1000u + i), 0};
        CHECK(cndp_pcb_add(pt, &e) == (int)i);
    }
    CHECK(cndp_tcb_set(tt, N, &t) == -EINVAL && cndp_tcb_get(tt, N, &g) == -EINVAL && cndp_tcb_clear(tt, N) == -EINVAL);
    CHECK(cndp_tcb_set(tt, 0xFFFFFFFFu, &t) == -EINVAL);
    t.state = 12;
    CHECK(cndp_tcb_set(tt, 0, &t) == -EINVAL);
    /* the whole table: set, read back, clear every third, read again */
    for (uint32_t i = 0; i < N; i++) {
        CHECK(cndp_tcb_get(tt, i, &g) == -ENOENT);
        t = est(i);
        t.state = (uint8_t)(i % 12u);
        memset(t.rsvd, 0xFF, sizeof(t.rsvd));
        t.flags = (uint8_t)(0xFEu | (i & 1u));
        CHECK(cndp_tcb_set(tt, i, &t) == 0);
    }
    for (uint32_t i = 0; i < N; i++) {
        CHECK(cndp_tcb_get(tt, i, &g) == 0);
        t = est(i);
        t.state = (uint8_t)(i % 12u);
        t.flags = (uint8_t)(i & 1u);
        CHECK(memcmp(&g, &t, sizeof(t)) == 0);
        if (i % 3u == 0) {
            CHECK(cndp_tcb_clear(tt, i) == 0 && cndp_tcb_clear(tt, i) == -ENOENT);
            CHECK(cndp_tcb_get(tt, i, &g) == -ENOENT);
        }
    }
    /* a PCB delete takes the TCB with it, at the table's two ends and in between */
    const uint32_t del[] = {1, 2048, N - 1};
    for (uint32_t k = 0; k < 3; k++) {
        CHECK(cndp_tcb_get(tt, del[k], &g) == 0 || del[k] % 3u == 0);
        CHECK(cndp_pcb_del(pt, del[k]) == 0);
        CHECK(cndp_tcb_get(tt, del[k], &g) == -ENOENT);
        t = est(0);
        CHECK(cndp_tcb_set(tt, del[k], &t) == -ENOENT);
    }
    CHECK(cndp_tcb_get(tt, N - 2, &g) == 0 && g.rcv_nxt == 1000u + N - 2);

    /* segments at the end of exactly sized buffers */
    struct cndp_tcp_opt o;
    const uint32_t P = 5; /* established, rcv_nxt 1005 */
    t = est(P);
    CHECK(cndp_tcb_set(tt, P, &t) == 0);
    const uint8_t F = CNDP_TCPSEG_FIRST;
    CHECK(run_one(tt, P, 0x10, NULL, 0, NULL, 0, 1005, &o) == (CNDP_TCPSEG_PRED_ACK | F) && o.wnd == 8192u);
    CHECK(run_one(tt, 3, 0x10, NULL, 0, NULL, 0, 1005, &o) == (CNDP_TCPSEG_RESET | F)); /* cleared above */
    /* a timestamp that ends with the buffer */
    const uint8_t ts[12] = {1, 1, 8, 10, 0, 0, 1, 0xF4, 0, 0, 0, 9};
    CHECK(run_one(tt, P, 0x10, ts, 12, NULL, 0, 1005, &o) == (CNDP_TCPSEG_PRED_ACK | CNDP_TCPSEG_TS_UPDATE | F));
    CHECK(o.ts_val == 500u && o.ts_ecr == 9u && o.sflags == CNDP_SEG_TS_PRESENT && o.mss == 0);
    /* a known kind in the buffer's last byte: its length lies past the allocation and reads as zero */
    for (uint32_t optlen = 4; optlen <= 40; optlen += 4) {
        uint8_t op[40];
        memset(op, 1, sizeof(op));
        const uint8_t kinds[] = {2, 3, 4, 8};
        for (uint32_t k = 0; k < 4; k++) {
            op[optlen - 1] = kinds[k];
            CHECK(run_one(tt, P, 0x10, op, optlen, NULL, 0, 1005, &o) == (CNDP_TCPSEG_BADOPT | F));
            CHECK(o.ts_val == 0 && o.ts_ecr == 0 && o.wnd == 0 && o.mss == 0 && o.sflags == 0);
            /* with one payload byte behind it, that byte is the length */
            const uint8_t one = 1, two = 2;
            CHECK(run_one(tt, P, 0x10, op, optlen, &one, 1, 1005, &o) == (CNDP_TCPSEG_PRED_NONE | F)); /* ack != snd_una */
            CHECK(run_one(tt, P, 0x10, op, optlen, &two, 1, 1005, &o) == (CNDP_TCPSEG_BADOPT | F));
        }
        op[optlen - 1] = 5; /* unknown kind: the zero length fails it all the same */
        CHECK(run_one(tt, P, 0x10, op, optlen, NULL, 0, 1005, &o) == (CNDP_TCPSEG_BADOPT | F));
        op[optlen - 2] = 99; /* unknown kind, length 200: walks off the end, success */
        op[optlen - 1] = 200;
        CHECK(run_one(tt, P, 0x10, op, optlen, NULL, 0, 1005, &o) == (CNDP_TCPSEG_PRED_ACK | F));
    }
    /* SYN options on a listener, the buffer ending with the window scale */
    t = est(0);
    t.state = CNDP_TCPS_LISTEN;
    CHECK(cndp_tcb_set(tt, 7, &t) == 0);
    const uint8_t syn[8] = {2, 4, 0x23, 0x28, 1, 3, 3, 15};
    CHECK(run_one(tt, 7, 0x02, syn, 8, NULL, 0, 1, &o) == (CNDP_TCPSEG_SLOW | F));
    CHECK(o.mss == 1460u && o.sflags == (CNDP_SEG_MSS_PRESENT | CNDP_SEG_WS_PRESENT | 14u) && o.wnd == 1024u);

    cndp_tcb_tbl_destroy(tt);
    cndp_tcb_tbl_destroy(NULL);
    cndp_pcb_free(pt);
    printf("PASS\n");
    return 0;
}

/* cndp_tcp_segment_node_host and the TCB table (include/cndp_mqtcb.h,
 * include/cndp_tcb.h, cndp_amd/csrc/tcb.c over pcb.c's walk) under the address
 * and undefined-behaviour sanitizers: a pool of 2 KiB mbufs in one heap block of
 * exactly its size, so a read or write past the region's end is caught; segments
 * with 12 and 40 option bytes at every mtod alignment (odd ones among them),
 * their headers ending inside the readable bytes, exactly at data_len, at
 * stage_max, at the buffer's end and at the region's end, and cut there in the
 * middle of the options; a full 4096-entry table with a TCB on its last index;
 * TCBs set, cleared and taken away by cndp_pcb_del between calls; FIRST behind
 * dropped mbufs; NULL outputs; a hook that answers NULL; a TCB table over another
 * PCB table.  Prints PASS. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cndp_mqtcb.h"

#define FRAME 2048u
#define NMB 64u
#define E_NONE 0xFFFFu
#define E_DROP 0x0500u
#define E_SEG 0x0501u
#define E_CK 0x0080u
#define E_OPT 0x0040u
#define NOW 100000u

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);               \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static uint8_t *pool;

static uint8_t *mb(uint32_t i) { return pool + (size_t)i * FRAME; }

static void put16(uint8_t *p, uint16_t v) { memcpy(p, &v, 2); }
static uint16_t get16(const uint8_t *p)
{
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
}
static void be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

/* ones-complement sum of big-endian 16-bit words */
static uint32_t sum_be(const uint8_t *p, uint32_t n, uint32_t s)
{
    for (uint32_t k = 0; k < n; k++)
        s += (k & 1u) ? p[k] : (uint32_t)p[k] << 8;
    return s;
}

/* mbuf i: an IPv4 header of l3 bytes and a pure ACK of connection sport with nopt
 * option bytes (NOP NOP, a timestamp ts_val / NOW - 5, NOPs behind it) at
 * buf_addr + doff, as far as it fits into the pool; seq / ack / wnd as given; the
 * checksum is right over the frame's first `clip` bytes with zeros behind them;
 * data_len = dlen */
static void put(uint32_t i, uint32_t doff, uint32_t l3, uint32_t nopt, uint16_t sport, uint32_t seq, uint32_t ack,
                uint16_t wnd, uint32_t ts_val, uint16_t blen, uint32_t dlen, uint32_t clip)
{
    uint8_t f[160];
    memset(f, 0, sizeof(f));
    const uint32_t seg = 20 + nopt, tot = l3 + seg;
    f[0] = (uint8_t)(0x40u | l3 / 4u);
    f[2] = (uint8_t)(tot >> 8);
    f[3] = (uint8_t)tot;
    f[9] = 6;
    const uint8_t src[4] = {198, 18, 0, 1}, dst[4] = {10, 4, 0, 7};
    memcpy(f + 12, src, 4);
    memcpy(f + 16, dst, 4);
    uint8_t *u = f + l3;
    u[0] = (uint8_t)(sport >> 8);
    u[1] = (uint8_t)sport;
    u[2] = (uint8_t)(5000 >> 8);
    u[3] = (uint8_t)5000;
    be32(u + 4, seq);
    be32(u + 8, ack);
    u[12] = (uint8_t)((seg / 4u) << 4);
    u[13] = 0x10;
    u[14] = (uint8_t)(wnd >> 8);
    u[15] = (uint8_t)wnd;
    if (nopt) {
        memset(u + 20, 1, nopt);
        u[22] = 8;
        u[23] = 10;
        be32(u + 24, ts_val);
        be32(u + 28, NOW - 5u);
    }
    uint8_t g[160];
    memcpy(g, f, sizeof(g));
    if (clip < tot)
        memset(g + clip, 0, tot - clip);
    uint32_t s = sum_be(g + 12, 8, 0) + 6u + seg;
    s = sum_be(g + l3, seg, s);
    while (s >> 16)
        s = (s & 0xffffu) + (s >> 16);
    const uint16_t c = (uint16_t)~s;
    if (l3 + 17 < clip) { /* else the field itself reads as zero */
        u[16] = (uint8_t)(c >> 8);
        u[17] = (uint8_t)c;
    }
    uint8_t *m = mb(i);
    memset(m, 0, 64);
    uint64_t buf = (uint64_t)(uintptr_t)(m + 64);
    memcpy(m + 8, &buf, 8);
    put16(m + 24, (uint16_t)doff);
    put16(m + 28, blen);
    put16(m + 30, (uint16_t)dlen);
    const uint64_t txo = 14u | (uint64_t)l3 << 7 | 20ull << 16;
    memcpy(m + 40, &txo, 8);
    size_t o = (size_t)i * FRAME + 64 + doff, room = (size_t)NMB * FRAME - o;
    memcpy(pool + o, f, tot < room ? tot : room);
}

static void *md_some(const void *m)
{
    const uint32_t i = (uint32_t)(((const uint8_t *)m - pool) / FRAME);
    return i < 2u ? NULL : (uint8_t *)(uintptr_t)m + 128;
}

static uint16_t net16(uint16_t v) { return (uint16_t)(v >> 8 | v << 8); }

int main(void)
{
    pool = malloc((size_t)NMB * FRAME);
    CHECK(pool);
    memset(pool, 0x5A, (size_t)NMB * FRAME);
    cndp_pcb_tbl_t *t, *t2;
    cndp_tcb_tbl_t *tc, *tc2;
    CHECK(cndp_pcb_create(4096, &t) == 0 && cndp_pcb_create(4, &t2) == 0);
    const uint32_t LADDR = 0x0700040Au, PEER = 0x010012C6u; /* 10.4.0.7, 198.18.0.1 as loaded */
    const struct cndp_pcb_entry any = {0, 0, net16(5000), 0, 0};
    CHECK(cndp_pcb_add(t, &any) == 0);
    for (uint32_t k = 1; k < 4096; k++) { /* a full table: connection k has foreign port 20000 + k */
        const struct cndp_pcb_entry c = {LADDR, PEER, net16(5000), net16((uint16_t)(20000 + k)), 0};
        CHECK(cndp_pcb_add(t, &c) == (int)k);
    }
    CHECK(cndp_tcb_tbl_create(t, &tc) == 0 && cndp_tcb_tbl_create(t2, &tc2) == 0);
    struct cndp_tcb est;
    memset(&est, 0, sizeof(est));
    est.rcv_nxt = 1000;
    est.snd_una = 500;
    est.snd_nxt = est.snd_max = 700;
    est.snd_wnd = 512;
    est.snd_cwnd = 4000;
    est.ts_recent = 90;
    est.last_ack_sent = 990;
    est.rcv_space = 4000;
    est.max_mss = 1460;
    est.state = CNDP_TCPS_ESTABLISHED;
    est.flags = CNDP_TCB_REASS_EMPTY;
    CHECK(cndp_tcb_set(tc, 1, &est) == 0 && cndp_tcb_set(tc, 4095, &est) == 0 && cndp_tcb_set(tc, 7, &est) == 0);

    void *ptrs[256];
    uint16_t e[256];
    struct cndp_tcp_seg sg[256];
    struct cndp_tcp_opt op[256];
    uint8_t v[256];
    const void *end = pool + (size_t)NMB * FRAME;

    /* 12 and 40 option bytes at sixteen alignments, connections 1 and 4095 alternating */
    for (uint32_t i = 0; i < 32; i++) {
        const uint32_t nopt = i & 1u ? 40u : 12u;
        put(i, 192 + i % 16u, 20, nopt, (uint16_t)(20000 + (i & 2u ? 4095u : 1u)), 1000, 600, 512, 95, 1984, 40 + nopt, 4096);
        ptrs[i] = mb(i);
    }
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 32, e, sg, op, v, end, 0, NULL) == 0);
    for (uint32_t i = 0; i < 32; i++) {
        CHECK(e[i] == E_SEG && sg[i].offset == (i & 1u ? 60 : 32) && sg[i].seq == 1000);
        CHECK(v[i] == (CNDP_TCPSEG_PRED_ACK | (i == 0 || i == 2 ? CNDP_TCPSEG_FIRST : 0)));
        CHECK(op[i].ts_val == 95 && op[i].ts_ecr == NOW - 5u && op[i].wnd == 512 && op[i].sflags == CNDP_SEG_TS_PRESENT);
        CHECK(get16(mb(i) + 24) == 192 + i % 16u + 20 + sg[i].offset && get16(mb(i) + 30) == 0);
    }
    /* `now` behind the echo: it is zeroed; a timestamp at ts_recent: TS_UPDATE */
    put(0, 193, 20, 12, 20001, 1000, 600, 512, 90, 1984, 52, 4096);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW - 6u, ptrs, 1, e, sg, op, v, end, 0, NULL) == 0);
    CHECK(v[0] == (CNDP_TCPSEG_PRED_ACK | CNDP_TCPSEG_TS_UPDATE | CNDP_TCPSEG_FIRST) && op[0].ts_ecr == 0 && op[0].ts_val == 90);

    /* the header's end against each bound.  Clipped at frame byte 43 the timestamp's kind is readable
     * and its length byte is not: BADOPT; clipped at 52 a 60-byte header's options end in zeros: EOL */
    static const struct {
        uint32_t nopt, clip, verdict, ts;
    } cut[4] = {{12, 43, CNDP_TCPSEG_BADOPT, 0}, {12, 52, CNDP_TCPSEG_PRED_ACK, 95},
                {40, 52, CNDP_TCPSEG_PRED_ACK, 95}, {40, 80, CNDP_TCPSEG_PRED_ACK, 95}};
    for (uint32_t how = 0; how < 4; how++)
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t tot = 40 + cut[k].nopt, clip = cut[k].clip, last = NMB - 1;
            ptrs[0] = mb(last);
            int r;
            if (how == 0) { /* data_len */
                put(last, 201, 20, cut[k].nopt, 20007, 1000, 600, 512, 95, 1984, clip, clip);
                r = cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 1, e, sg, op, v, end, 0, NULL);
            } else if (how == 1) { /* stage_max */
                put(last, 201, 20, cut[k].nopt, 20007, 1000, 600, 512, 95, 1984, tot, clip);
                r = cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 1, e, sg, op, v, NULL, clip, NULL);
            } else if (how == 2) { /* the buffer's end */
                put(last, 201, 20, cut[k].nopt, 20007, 1000, 600, 512, 95, (uint16_t)(201 + clip), tot, clip);
                r = cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 1, e, sg, op, v, end, 0, NULL);
            } else { /* the region's end: the heap block ends with the frame's last readable byte */
                put(last, 1984 - clip, 20, cut[k].nopt, 20007, 1000, 600, 512, 95, 4000, tot, clip);
                r = cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 1, e, sg, op, v, end, 0, NULL);
            }
            CHECK(r == 0 && e[0] == E_SEG);
            CHECK(v[0] == (cut[k].verdict | CNDP_TCPSEG_FIRST) && op[0].ts_val == cut[k].ts);
        }

    /* FIRST behind dropped mbufs: a bad sum, a NULL hook answer (mbufs 0 and 1), a frame too short to adjust,
     * rx_short, rx_badoff, then IPv4 options with a header offset that stands (judged) */
    for (uint32_t i = 0; i < 8; i++) {
        put(i, 200 + i, 20, 12, 20007, 1000, 600, 512, 95, 1984, 52, 4096);
        ptrs[i] = mb(i);
    }
    mb(2)[64 + 202 + 51] ^= 0x10;                                         /* the sum fails */
    put(3, 203, 20, 12, 20007, 1000, 600, 512, 95, 1984, 19, 19);         /* l3_len > data_len */
    put(4, 204, 20, 12, 20007, 1000, 600, 512, 95, 1984, 39, 39);         /* rx_short */
    put(5, 205, 20, 12, 20007, 1000, 600, 512, 95, 1984, 52, 4096);
    mb(5)[64 + 205 + 32] = 0x40;                                          /* offset 16 */
    mb(5)[64 + 205 + 36] ^= 0x40;                                         /* ... and the sum stays right */
    put(6, 206, 24, 12, 20007, 1000, 600, 512, 95, 1984, 56, 4096);       /* IPOPT: judged */
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 8, e, sg, op, v, end, 0, md_some) == 0);
    CHECK(e[0] == E_DROP && e[1] == E_DROP && e[2] == (E_DROP | E_CK) && e[4] == E_DROP && e[5] == E_DROP);
    CHECK((e[3] & 0xFF00u) == 0x0500u && e[3] != E_SEG);
    CHECK(e[6] == (E_SEG | E_OPT) && e[7] == E_SEG);
    for (uint32_t i = 0; i < 6; i++)
        CHECK(v[i] == CNDP_TCPSEG_NONE && op[i].wnd == 0 && op[i].ts_val == 0);
    CHECK(v[6] == (CNDP_TCPSEG_PRED_ACK | CNDP_TCPSEG_FIRST) && v[7] == CNDP_TCPSEG_PRED_ACK && op[6].ts_val == 95);
    CHECK(get16(mb(6) + 24) == 206 && mb(6)[128] == 2);

    /* TCBs changed between calls: cleared (RESET), closed, taken away by cndp_pcb_del (no match: the listener, no TCB) */
    put(0, 192, 20, 0, 20007, 1000, 600, 512, 0, 1984, 40, 4096);
    CHECK(cndp_tcb_clear(tc, 7) == 0);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 1, e, NULL, NULL, v, end, 0, NULL) == 0);
    CHECK(e[0] == E_SEG && v[0] == (CNDP_TCPSEG_RESET | CNDP_TCPSEG_FIRST));
    est.state = CNDP_TCPS_CLOSED;
    CHECK(cndp_tcb_set(tc, 7, &est) == 0);
    put(0, 192, 20, 0, 20007, 1000, 600, 512, 0, 1984, 40, 4096);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 1, e, sg, op, NULL, end, 0, NULL) == 0 && op[0].wnd == 0);
    put(0, 192, 20, 0, 20007, 1000, 600, 512, 0, 1984, 40, 4096);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 1, e, sg, op, v, end, 0, NULL) == 0);
    CHECK(v[0] == (CNDP_TCPSEG_CLOSED | CNDP_TCPSEG_FIRST));
    CHECK(cndp_pcb_del(t, 7) == 0);
    put(0, 192, 20, 0, 20007, 1000, 600, 512, 0, 1984, 40, 4096);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 1, e, sg, op, v, end, 0, NULL) == 0);
    CHECK(e[0] == E_SEG && v[0] == (CNDP_TCPSEG_RESET | CNDP_TCPSEG_FIRST)); /* the wildcard listener answers: no TCB */
    struct cndp_tcb got;
    CHECK(cndp_tcb_get(tc, 7, &got) == -2);

    /* mbufs that are not taken, and the argument checks */
    void *odd[2] = {NULL, mb(0)};
    put(0, 192, 20, 0, 20001, 1000, 600, 512, 0, 1984, 40, 4096);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, odd, 2, e, sg, op, v, end, 0, NULL) == 0);
    CHECK(e[0] == E_NONE && v[0] == CNDP_TCPSEG_NONE && e[1] == E_SEG && (v[1] & CNDP_TCPSEG_FIRST));
    CHECK(cndp_tcp_segment_node_host(NULL, tc, NOW, ptrs, 1, e, sg, op, v, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_segment_node_host(t, NULL, NOW, ptrs, 1, e, sg, op, v, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_segment_node_host(t, tc2, NOW, ptrs, 1, e, sg, op, v, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_segment_node_host(t2, tc, NOW, ptrs, 1, e, sg, op, v, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, NULL, 1, e, sg, op, v, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 1, NULL, sg, op, v, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, ptrs, 257, e, sg, op, v, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_segment_node_host(t, tc, NOW, NULL, 0, NULL, NULL, NULL, NULL, NULL, 0, NULL) == 0);
    cndp_tcb_tbl_destroy(tc2);
    cndp_tcb_tbl_destroy(tc);
    cndp_pcb_free(t2);
    cndp_pcb_free(t);
    free(pool);
    printf("PASS\n");
    return 0;
}

/* tcpout.c (cndp_tcp_output_host, cndp_tcp_send_optlen) and the transmit
 * attributes of tcb.c under -fsanitize=address,undefined: both modes over heap
 * buffers sized to end at every byte of a frame's header, options, payload and
 * zero fill -- a store past the slab is then a store past the allocation -- and
 * send buffers that end inside the payload.  What a cut buffer holds must equal
 * the same bytes of the uncut run.  Prints PASS and exits 0; any check that fails
 * exits 1, a sanitizer report aborts. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cndp_amd/csrc/tcpout_internal.h"

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            exit(1);                                                 \
        }                                                            \
    } while (0)

#define H 9u /* H + 26 is odd: no store of the header is aligned */
#define NF 3u
#define SLOT 257u

struct out {
    uint16_t len[NF];
    uint32_t faddr[NF], laddr[NF];
    uint8_t taken[NF];
    uint64_t stats[CNDP_TCPOUT_NSTATS];
};

/* One call over a heap slab of exactly slab_len bytes (filled with 0xEE) and a
 * heap send buffer of exactly snd_len bytes; every io array on the heap too. */
static uint8_t *run(cndp_tcb_tbl_t *tt, uint32_t mode, uint64_t slab_len, uint32_t snd_len, const uint32_t *plen,
                    const uint8_t *flags, int desc, struct out *o)
{
    uint8_t *slab = malloc(slab_len ? slab_len : 1);
    uint8_t *snd = malloc(snd_len ? snd_len : 1);
    uint32_t *pcb = malloc(NF * sizeof(*pcb));
    uint64_t *src = malloc(NF * sizeof(*src));
    uint8_t *sel = malloc(NF), *verdict = malloc(NF);
    struct cndp_tcp_txseg *d = aligned_alloc(16, NF * sizeof(*d));
    struct cndp_tcp_seg *sg = aligned_alloc(16, NF * sizeof(*sg));
    CHECK(slab && snd && pcb && src && sel && verdict && d && sg);
    memset(slab, 0xEE, slab_len);
    for (uint32_t k = 0; k < snd_len; k++)
        snd[k] = (uint8_t)(k * 7u + 1u);
    for (uint32_t i = 0; i < NF; i++) {
        pcb[i] = i;
        src[i] = 40u * i;
        sel[i] = 1;
        verdict[i] = CNDP_TCPSEG_RESET | CNDP_TCPSEG_FIRST;
        memset(&d[i], 0, sizeof(d[i]));
        d[i].seq = 0x01020304u + i;
        d[i].ack = 0xA1A2A3A4u;
        d[i].wnd = 0x1122;
        d[i].urp = 0x3344;
        d[i].len = (uint16_t)plen[i];
        d[i].flags = flags[i];
        memset(&sg[i], 0, sizeof(sg[i]));
        sg[i].seq = 77;
        sg[i].ack = 0xB1B2B3B4u;
        sg[i].len = (uint16_t)plen[i];
        sg[i].flags = flags[i];
        sg[i].offset = 20;
    }
    struct cndp_tcpout_io io;
    memset(&io, 0, sizeof(io));
    memset(o, 0, sizeof(*o));
    io.pcb = pcb;
    if (mode == CNDP_TCPOUT_SEGMENT || desc)
        io.txseg = d;
    else
        io.seg = sg;
    io.sel = desc ? sel : NULL;
    io.verdict = verdict;
    if (mode == CNDP_TCPOUT_SEGMENT && snd_len) {
        io.snd = snd;
        io.snd_len = snd_len;
        io.src_off = src;
    }
    io.len = o->len;
    io.faddr = o->faddr;
    io.laddr = o->laddr;
    io.taken = o->taken;
    io.stats = o->stats;
    CHECK(cndp_tcp_output_host(tt, mode, 0x01020304u, slab, slab_len, SLOT, NULL, H, NF, &io) == 0);
    for (uint32_t i = 0; i < NF; i++)
        CHECK(pcb[i] == i && src[i] == 40u * i && d[i].len == plen[i] && sg[i].seq == 77);
    free(sg);
    free(d);
    free(verdict);
    free(sel);
    free(src);
    free(pcb);
    free(snd);
    return slab;
}

int main(void)
{
    cndp_pcb_tbl_t *pt = NULL;
    cndp_tcb_tbl_t *tt = NULL;
    CHECK(cndp_pcb_create(NF + 1, &pt) == 0 && cndp_tcb_tbl_create(pt, &tt) == 0);
    for (uint32_t i = 0; i < NF; i++) {
        struct cndp_pcb_entry e = {0x0100040Au, 0x010012C6u, 0x5000, (uint16_t)(0x409Cu + i), 0};
        CHECK(cndp_pcb_add(pt, &e) == (int)i);
    }
    struct cndp_tcb_tx a = {0xFF, 7, 3, 0xFF}, g;
    CHECK(cndp_tcb_tx_set(tt, 0, &a) == -ENOENT && cndp_tcb_tx_get(tt, 0, &g) == -ENOENT);
    CHECK(cndp_tcb_tx_set(tt, NF, &a) == -EINVAL && cndp_tcb_tx_set(NULL, 0, &a) == -EINVAL);
    struct cndp_tcb t;
    memset(&t, 0, sizeof(t));
    t.state = CNDP_TCPS_ESTABLISHED;
    t.max_mss = 200;
    t.ts_recent = 0x0A0B0C0Du;
    t.rcv_space = 1u << 20;
    for (uint32_t i = 0; i < 2; i++) { /* PCB 2 has no TCB */
        CHECK(cndp_tcb_set(tt, i, &t) == 0);
        CHECK(cndp_tcb_tx_get(tt, i, &g) == 0 && g.tflags == 0 && g.req_recv_scale == 0 && g.rcv_scale == 0);
    }
    CHECK(cndp_tcb_tx_set(tt, 0, &a) == 0 && cndp_tcb_tx_get(tt, 0, &g) == 0);
    CHECK(g.tflags == 0x0F && g.req_recv_scale == 7 && g.rcv_scale == 3 && g.rsvd == 0);
    CHECK(cndp_tcb_set(tt, 0, &t) == 0 && cndp_tcb_tx_get(tt, 0, &g) == 0 && g.tflags == 0x0F);
    for (uint32_t tf = 0; tf < 16; tf++)
        for (uint32_t fl = 0; fl < 64; fl++) {
            const uint32_t n = cndp_tcp_send_optlen((uint8_t)tf, (uint8_t)fl);
            CHECK(n % 4u == 0 && n <= 20u && ((fl & 2u) || n == 0 || n == 12u));
        }
    CHECK(cndp_tcp_send_optlen(0x0F, 0x02) == 20 && cndp_tcp_send_optlen(0x0F, 0x04) == 0);

    struct out full, cut;
    const uint64_t whole = (uint64_t)NF * SLOT;
    /* SEGMENT: a SYN with every option (optlen 20) and a short payload, a bare ACK with a long
     * payload, and the PCB without a TCB; snd_len 0 = no send buffer, the payload is in place */
    const uint32_t plen[NF] = {5, 150, 9};
    const uint8_t fl[NF] = {0x02, 0x10, 0x10};
    for (uint32_t snd_len = 0; snd_len <= 230; snd_len += (snd_len < 60 ? 1 : 23)) {
        uint8_t *ref = run(tt, CNDP_TCPOUT_SEGMENT, whole, snd_len, plen, fl, 1, &full);
        CHECK(full.taken[0] == 1 && full.taken[1] == 1 && full.taken[2] == 0);
        CHECK(full.len[0] == 20 + 20 + 5 && full.len[1] == 20 + 150 && full.len[2] == 0);
        CHECK(full.stats[CNDP_TCPOUT_STAT_SENT] == 2 && full.stats[CNDP_TCPOUT_STAT_NOPCB] == 1);
        for (uint32_t k = 0; k < H + 26; k++)
            CHECK(ref[k] == 0xEE && ref[SLOT + k] == 0xEE);
        for (uint32_t k = 0; k < SLOT; k++)
            CHECK(ref[2 * SLOT + k] == 0xEE);
        /* frame 0: P = H + 66, 5 payload bytes (what snd holds of them, or left in place), then zeroes up to P + 66 */
        for (uint32_t k = 0; k < 66; k++)
            CHECK(ref[H + 66 + k] == (k >= 5 ? 0 : !snd_len ? 0xEE : k < snd_len ? (uint8_t)(k * 7u + 1u) : 0));
        CHECK(ref[H + 66 + 66] == 0xEE);
        /* every cut through frame 1 (header at SLOT + H + 26, payload up to SLOT + H + 46 + 150) and frame 0 */
        for (uint64_t L = 0; L <= SLOT + H + 46 + 150 + 2; L += (L > H + 140 && L < SLOT ? 50 : 1)) {
            uint8_t *s = run(tt, CNDP_TCPOUT_SEGMENT, L, snd_len, plen, fl, 1, &cut);
            CHECK(memcmp(s, ref, L) == 0);
            CHECK(memcmp(&cut, &full, sizeof(cut)) == 0); /* the outputs do not depend on the slab's end */
            free(s);
        }
        free(ref);
    }
    /* RESPOND from segments (an ACK, a SYN, an RST) and from descriptors (timestamps on PCB 0) */
    const uint8_t rfl[NF] = {0x10, 0x02, 0x04};
    for (int desc = 0; desc < 2; desc++) {
        uint8_t *ref = run(tt, CNDP_TCPOUT_RESPOND, whole, 0, plen, desc ? fl : rfl, desc, &full);
        CHECK(full.taken[0] == 1 && full.taken[1] == 1 && full.taken[2] == (desc ? 1 : 0));
        CHECK(full.len[1] == 20 && full.len[0] == (desc ? 40 : 20) && full.len[2] == (desc ? 20 : 0));
        for (uint64_t L = 0; L <= whole; L += (L % SLOT > H + 80 ? 40 : 1)) {
            uint8_t *s = run(tt, CNDP_TCPOUT_RESPOND, L, 0, plen, desc ? fl : rfl, desc, &cut);
            CHECK(memcmp(s, ref, L) == 0 && memcmp(&cut, &full, sizeof(cut)) == 0);
            free(s);
        }
        free(ref);
    }
    /* a PCB delete takes the attributes along */
    CHECK(cndp_pcb_del(pt, 0) == 0 && cndp_tcb_tx_get(tt, 0, &g) == -ENOENT && cndp_tcb_tx_set(tt, 0, &a) == -ENOENT);
    uint8_t *s = run(tt, CNDP_TCPOUT_SEGMENT, whole, 64, plen, fl, 1, &full);
    CHECK(full.taken[0] == 0 && full.taken[1] == 1);
    free(s);
    cndp_tcb_tbl_destroy(tt);
    cndp_pcb_free(pt);
    printf("PASS\n");
    return 0;
}

/* cndp_tcp_input_node_host (include/cndp_mqtcp.h, cndp_amd/csrc/pcb.c) under the
 * address and undefined-behaviour sanitizers: a pool of 2 KiB mbufs in one heap
 * block of exactly its size, so a read or write past the region's end is caught;
 * segments of every length class at every mtod alignment, ending at the buffer's
 * end, at the region's end, and with a total_length that reaches past both;
 * connections behind two listeners, a deleted entry, a 4096-entry table; every
 * header step of cnet_tcp_input's opening; a metadata hook that answers NULL and
 * m + 128; NULL entries; the user values.  Prints PASS. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cndp_mqtcp.h"

#define FRAME 2048u
#define NMB 128u
#define E_NONE 0xFFFFu
#define E_DROP 0x0500u
#define E_SEG 0x0501u
#define E_PUNT 0x0502u
#define E_CK 0x0080u
#define E_OPT 0x0040u
#define UNTOUCHED 0xABABABABABABABABull

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
static uint64_t get64(const uint8_t *p)
{
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

/* ones-complement sum of big-endian 16-bit words */
static uint32_t sum_be(const uint8_t *p, uint32_t n, uint32_t s)
{
    for (uint32_t k = 0; k < n; k++)
        s += (k & 1u) ? p[k] : (uint32_t)p[k] << 8;
    return s;
}

/* mbuf i: an IPv4 header of l3 bytes and a TCP segment of seg bytes (header
 * included, data offset nibble nib, flags fl) with a good checksum at
 * buf_addr + doff, as far as it fits into the pool; data_len = dlen */
static void put(uint32_t i, uint32_t doff, uint32_t l3, uint32_t seg, uint16_t sport, uint16_t dport, uint8_t nib,
                uint8_t fl, uint16_t blen, uint32_t dlen)
{
    uint8_t f[2048];
    memset(f, 0, sizeof(f));
    const uint32_t tot = l3 + seg;
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
    u[2] = (uint8_t)(dport >> 8);
    u[3] = (uint8_t)dport;
    for (uint32_t k = 4; k < seg; k++)
        u[k] = (uint8_t)(k * 37u + i);
    u[12] = (uint8_t)(nib << 4);
    u[13] = fl;
    u[16] = u[17] = 0;
    uint32_t s = sum_be(f + 12, 8, 0) + 6u + seg;
    s = sum_be(u, seg, s);
    while (s >> 16)
        s = (s & 0xffffu) + (s >> 16);
    const uint16_t c = (uint16_t)~s;
    u[16] = (uint8_t)(c >> 8);
    u[17] = (uint8_t)c;
    uint8_t *m = mb(i);
    memset(m, 0, 64);
    uint64_t buf = (uint64_t)(uintptr_t)(m + 64);
    memcpy(m + 8, &buf, 8);
    put16(m + 24, (uint16_t)doff);
    put16(m + 28, blen);
    put16(m + 30, (uint16_t)dlen);
    const uint64_t txo = 14u | (uint64_t)l3 << 7 | 20ull << 16, up = UNTOUCHED;
    memcpy(m + 40, &txo, 8);
    memcpy(m + 56, &up, 8);
    size_t o = (size_t)i * FRAME + 64 + doff, room = (size_t)NMB * FRAME - o;
    memcpy(pool + o, f, tot < room ? tot : room);
}

static void *md_some(const void *m)
{
    const uint32_t i = (uint32_t)(((const uint8_t *)m - pool) / FRAME);
    return i % 4u == 3u ? NULL : (uint8_t *)(uintptr_t)m + 128;
}

static uint16_t net16(uint16_t v) { return (uint16_t)(v >> 8 | v << 8); }

int main(void)
{
    pool = malloc((size_t)NMB * FRAME);
    CHECK(pool);
    memset(pool, 0x5A, (size_t)NMB * FRAME);
    cndp_pcb_tbl_t *t;
    CHECK(cndp_pcb_create(4096, &t) == 0);
    const uint32_t LADDR = 0x0700040Au, PEER = 0x010012C6u; /* 10.4.0.7, 198.18.0.1 as loaded */
    const struct cndp_pcb_entry any = {0, 0, net16(5000), 0, 0};
    const struct cndp_pcb_entry bound = {LADDR, 0, net16(5000), 0, 0};
    CHECK(cndp_pcb_add(t, &any) == 0 && cndp_pcb_add(t, &bound) == 1);
    for (uint32_t k = 0; k < 4094; k++) { /* a full table: 4094 connections behind the two listeners */
        const struct cndp_pcb_entry c = {LADDR, PEER, net16(5000), net16((uint16_t)(20000 + k)), 0};
        CHECK(cndp_pcb_add(t, &c) == (int)(2 + k));
    }
    CHECK(cndp_pcb_user_set(t, 2, 0x1122334455667788ull) == 0);
    CHECK(cndp_pcb_del(t, 3) == 0); /* 20001: falls back to the bound listener */

    void *ptrs[256];
    uint16_t e[256];
    struct cndp_tcp_seg sg[256];
    const void *end = pool + (size_t)NMB * FRAME;
    static const uint32_t lens[13] = {20, 21, 23, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1460};
    for (uint32_t i = 0; i < 104; i++) { /* every length at eight alignments, connections 2 + i * 39 */
        put(i, 192 + (i * 5u) % 16u, 20, lens[i % 13], (uint16_t)(20000 + i * 39u), 5000, 5, 0x10, 1984, 20 + lens[i % 13]);
        ptrs[i] = mb(i);
    }
    pool[(size_t)12 * FRAME + 64 + 192 + (12 * 5) % 16 + 20 + 1459] ^= 0x01; /* i = 12: the last byte of its 1460 */
    CHECK(cndp_tcp_input_node_host(t, ptrs, 104, e, sg, end, 0, NULL) == 0);
    for (uint32_t i = 0; i < 104; i++) {
        if (i == 12) {
            CHECK(e[i] == (E_DROP | E_CK) && get64(mb(i) + 56) == UNTOUCHED && get16(mb(i) + 24) == 192 + (12 * 5) % 16);
            CHECK(sg[i].offset == 0 && sg[i].seq == 0);
            continue;
        }
        CHECK(e[i] == E_SEG);
        CHECK(get64(mb(i) + 56) == (i == 0 ? 0x1122334455667788ull : 2 + i * 39u));
        CHECK(get16(mb(i) + 24) == 192 + (i * 5u) % 16u + 40 && get16(mb(i) + 30) == lens[i % 13] - 20);
        CHECK(sg[i].offset == 20 && sg[i].flags == 0x10 && sg[i].len == lens[i % 13] - 20);
        const uint8_t *md = mb(i) + 64;
        CHECK(md[0] == 2 && md[1] == 4 && md[4] == 198 && md[7] == 1 && md[8] == 0 && md[19] == 0 && md[20] == 2 &&
              md[21] == 4 && md[24] == 10 && md[27] == 7 && md[39] == 0);
    }
    /* the deleted connection, a port nobody listens on, another local address, punt off */
    put(0, 192, 20, 30, 20001, 5000, 5, 0x10, 1984, 50);
    put(1, 193, 20, 30, 20000, 4999, 5, 0x10, 1984, 50);
    put(2, 194, 20, 30, 20000, 5000, 5, 0x10, 1984, 50);
    mb(2)[64 + 194 + 19] = 9; /* dst 10.4.0.9: only the wildcard listener; the sum no longer agrees */
    CHECK(cndp_tcp_input_node_host(t, ptrs, 3, e, NULL, end, 0, NULL) == 0);
    CHECK(e[0] == E_SEG && get64(mb(0) + 56) == 1 && e[1] == E_PUNT && get64(mb(1) + 56) == UNTOUCHED);
    CHECK(e[2] == (E_DROP | E_CK));
    CHECK(cndp_pcb_set_flags(t, 0, 0) == 0);
    put(1, 193, 20, 30, 20000, 4999, 5, 0x10, 1984, 50);
    CHECK(cndp_tcp_input_node_host(t, ptrs + 1, 1, e, sg, end, 0, NULL) == 0 && e[0] == E_DROP);
    CHECK(get16(mb(1) + 64 + 22) == net16(4999)); /* the ports are written before the lookup */

    /* the header steps */
    put(0, 192, 24, 40, 20000, 5000, 5, 0x10, 1984, 64);  /* IPOPT */
    put(1, 192, 20, 40, 20000, 5000, 5, 0x10, 192 + 59, 60); /* the buffer ends a byte early: the sum fails */
    put(2, 192, 20, 20, 20000, 5000, 5, 0x10, 1984, 40);  /* 20 left: SEGMENT */
    put(3, 192, 20, 40, 20000, 5000, 4, 0x10, 1984, 60);  /* offset 16: rx_badoff after the adj_offset */
    put(4, 192, 20, 40, 20000, 5000, 15, 0x10, 1984, 60); /* offset 60 > data_len 40: SEGMENT, no adj, len wraps */
    put(5, 192, 20, 24, 20000, 5000, 15, 0x10, 1984, 44); /* offset 60 > total_length 44: rx_badoff */
    put(6, 192, 20, 21, 20000, 5000, 5, 0x03, 1984, 41);  /* SYN | FIN */
    put(7, 192, 20, 40, 20000, 5000, 5, 0x10, 1984, 40);  /* total_length beyond data_len: zeros are summed */
    CHECK(cndp_tcp_input_node_host(t, ptrs, 8, e, sg, end, 0, NULL) == 0);
    CHECK(e[0] == (E_SEG | E_OPT) && get16(mb(0) + 24) == 192 && get16(mb(0) + 30) == 64 && sg[0].offset == 20 &&
          sg[0].len == 20 && get64(mb(0) + 56) == 0x1122334455667788ull);
    CHECK(e[1] == (E_DROP | E_CK) && get16(mb(1) + 24) == 192);
    CHECK(e[2] == E_SEG && get16(mb(2) + 24) == 232 && get16(mb(2) + 30) == 0 && sg[2].len == 0);
    CHECK(e[3] == E_DROP && get16(mb(3) + 24) == 228 && get16(mb(3) + 30) == 24 && sg[3].offset == 0);
    CHECK(e[4] == E_SEG && get16(mb(4) + 24) == 212 && get16(mb(4) + 30) == 40 && sg[4].len == 0xFFEC && sg[4].offset == 60);
    CHECK(e[5] == E_DROP && get16(mb(5) + 24) == 212 && get16(mb(5) + 30) == 24);
    CHECK(e[6] == E_SEG && sg[6].len == 3 && sg[6].flags == 3);
    CHECK(e[7] == (E_DROP | E_CK));

    /* total_length past the region's end, past the buffer's end and past stage_max:
     * zeros are read, nothing outside is touched */
    for (uint32_t k = 0; k < 3; k++) {
        put(NMB - 1, 1984 - 20 - 100 + 1 + 7 * k, 20, 100, 20000, 5000, 5, 0x10, 1984, 120);
        ptrs[0] = mb(NMB - 1);
        CHECK(cndp_tcp_input_node_host(t, ptrs, 1, e, sg, end, 0, NULL) == 0 && (e[0] & 0xFF00u) == 0x0500u);
    }
    put(NMB - 1, 1984 - 20 - 100, 20, 100, 20000, 5000, 5, 0x10, 1984, 120); /* ends exactly at both ends */
    CHECK(cndp_tcp_input_node_host(t, ptrs, 1, e, sg, end, 0, NULL) == 0 && e[0] == E_SEG);
    put(10, 192, 20, 400, 20000, 5000, 5, 0x10, 1984, 420);
    ptrs[0] = mb(10);
    CHECK(cndp_tcp_input_node_host(t, ptrs, 1, e, sg, NULL, 128, NULL) == 0 && e[0] == (E_DROP | E_CK));
    put(10, 192, 20, 400, 20000, 5000, 5, 0x10, 1984, 420);
    CHECK(cndp_tcp_input_node_host(t, ptrs, 1, e, sg, NULL, 2048, NULL) == 0 && e[0] == E_SEG);
    /* a frame that begins at the region's end, an mbuf whose header crosses it, a NULL entry */
    put(NMB - 1, 1984, 20, 26, 20000, 5000, 5, 0x10, 4000, 46);
    void *odd[3] = {mb(NMB - 1), NULL, mb(NMB - 1)};
    CHECK(cndp_tcp_input_node_host(t, odd, 3, e, sg, end, 0, NULL) == 0 && e[0] == E_NONE && e[1] == E_NONE);
    CHECK(cndp_tcp_input_node_host(t, odd, 1, e, sg, pool + (size_t)(NMB - 1) * FRAME + 63, 0, NULL) == 0 && e[0] == E_NONE);

    /* a hook that answers NULL for every fourth mbuf and m + 128 for the rest */
    for (uint32_t i = 0; i < 16; i++) {
        put(i, 200, 20, 64, 20000, 5000, 5, 0x10, 1984, 84);
        ptrs[i] = mb(i);
    }
    CHECK(cndp_tcp_input_node_host(t, ptrs, 16, e, sg, end, 0, md_some) == 0);
    for (uint32_t i = 0; i < 16; i++) {
        if (i % 4 == 3) {
            CHECK(e[i] == E_DROP && get64(mb(i) + 56) == UNTOUCHED && get16(mb(i) + 24) == 200 && sg[i].offset == 0);
        } else {
            CHECK(e[i] == E_SEG && mb(i)[128] == 2 && mb(i)[128 + 20] == 2 && get16(mb(i) + 24) == 240);
        }
    }
    /* argument checks */
    CHECK(cndp_tcp_input_node_host(NULL, ptrs, 1, e, sg, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_input_node_host(t, NULL, 1, e, sg, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_input_node_host(t, ptrs, 1, NULL, sg, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_input_node_host(t, ptrs, 257, e, sg, NULL, 0, NULL) == -22);
    CHECK(cndp_tcp_input_node_host(t, NULL, 0, NULL, NULL, NULL, 0, NULL) == 0);
    cndp_pcb_free(t);
    free(pool);
    printf("PASS\n");
    return 0;
}

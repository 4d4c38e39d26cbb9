/* cndp_udp_input_node_host (include/cndp_mql4.h, cndp_amd/csrc/pcb.c) under the
 * address and undefined-behaviour sanitizers: a pool of 2 KiB mbufs in one heap
 * block of exactly its size, so a read or write past the region's end is caught;
 * frames whose datagram ends at the buffer's end, at the region's end, and whose
 * total_length reaches past both; every mtod alignment; a metadata hook that
 * answers NULL; NULL entries; the user values.  Prints PASS. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cndp_mql4.h"

#define FRAME 2048u
#define NMB 64u
#define E_NONE 0xFFFFu
#define E_PDROP 0x0300u
#define E_TCP 0x0302u
#define E_DROP 0x0400u
#define E_RECV 0x0401u
#define E_PUNT 0x0402u
#define E_CK 0x0080u

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

/* mbuf i: an IPv4 header of l3 bytes and a UDP datagram of dgram bytes with a
 * good checksum at buf_addr + doff, as far as it fits into the pool */
static void put(uint32_t i, uint32_t doff, uint32_t l3, uint32_t dgram, uint8_t proto, uint16_t dport, uint16_t blen)
{
    uint8_t f[2048];
    memset(f, 0, sizeof(f));
    const uint32_t tot = l3 + dgram;
    f[0] = (uint8_t)(0x40u | l3 / 4u);
    f[2] = (uint8_t)(tot >> 8);
    f[3] = (uint8_t)tot;
    f[9] = proto;
    const uint8_t src[4] = {198, 18, 0, 1}, dst[4] = {10, 4, 0, 7};
    memcpy(f + 12, src, 4);
    memcpy(f + 16, dst, 4);
    uint8_t *u = f + l3;
    u[0] = 0x9C;
    u[1] = 0x40;
    u[2] = (uint8_t)(dport >> 8);
    u[3] = (uint8_t)dport;
    u[4] = (uint8_t)(dgram >> 8);
    u[5] = (uint8_t)dgram;
    for (uint32_t k = 8; k < dgram; k++)
        u[k] = (uint8_t)(k * 37u + i);
    uint32_t s = sum_be(f + 12, 8, 0) + proto + dgram;
    s = sum_be(u, dgram, s);
    while (s >> 16)
        s = (s & 0xffffu) + (s >> 16);
    uint16_t c = (uint16_t)~s;
    if (!c)
        c = 0xffff;
    u[6] = (uint8_t)(c >> 8);
    u[7] = (uint8_t)c;
    uint8_t *m = mb(i);
    memset(m, 0, 64);
    uint64_t buf = (uint64_t)(uintptr_t)(m + 64);
    memcpy(m + 8, &buf, 8);
    put16(m + 24, (uint16_t)doff);
    put16(m + 28, blen);
    put16(m + 30, (uint16_t)tot);
    const uint64_t txo = 14u | (uint64_t)l3 << 7 | 8ull << 16, up = 0xABABABABABABABABull;
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

int main(void)
{
    pool = malloc((size_t)NMB * FRAME);
    CHECK(pool);
    memset(pool, 0x5A, (size_t)NMB * FRAME);
    cndp_pcb_tbl_t *t;
    CHECK(cndp_pcb_create(16, &t) == 0);
    const struct cndp_pcb_entry any = {0, 0, 0x8813 /* 5000 */, 0, 0};
    const struct cndp_pcb_entry ck = {0, 0, 0x8A13 /* 5002 */, 0, CNDP_UDP_CHKSUM_FLAG};
    CHECK(cndp_pcb_add(t, &any) == 0 && cndp_pcb_add(t, &ck) == 1);
    CHECK(cndp_pcb_user_set(t, 1, 0x1122334455667788ull) == 0);
    uint64_t uv = 0;
    CHECK(cndp_pcb_user_get(t, 0, &uv) == 0 && uv == 0);
    CHECK(cndp_pcb_user_set(t, 2, 1) == -22 && cndp_pcb_user_get(t, 2, &uv) == -22);

    void *ptrs[256];
    uint16_t e[256];
    const void *end = pool + (size_t)NMB * FRAME;
    /* every alignment, three header lengths, odd and even datagram lengths, both tables' sockets */
    static const uint32_t l3s[3] = {20, 24, 60}, lens[6] = {8, 9, 33, 255, 257, 1472};
    for (uint32_t i = 0; i < NMB - 4; i++) {
        put(i, 192 + i % 16, l3s[i % 3], lens[i % 6], 17, i % 5 == 4 ? 5000 : 5002, 1984);
        ptrs[i] = mb(i);
    }
    /* a corrupted byte; a protocol that is not UDP; TCP; no socket */
    pool[(size_t)5 * FRAME + 64 + 192 + 5 + 60 + 20] ^= 0x10; /* i = 5: l3 60, a payload byte of its 1472 */
    put(NMB - 4, 192, 20, 26, 1, 5002, 1984);
    put(NMB - 3, 192, 20, 26, 6, 5002, 1984);
    put(NMB - 2, 193, 20, 26, 17, 4999, 1984);
    /* the last mbuf: its datagram ends exactly at the region's end, which is its buffer's end too */
    put(NMB - 1, 1984 - 24 - 100, 24, 100, 17, 5002, 1984);
    for (uint32_t i = NMB - 4; i < NMB; i++)
        ptrs[i] = mb(i);
    CHECK(cndp_udp_input_node_host(t, ptrs, NMB, e, end, 0, NULL) == 0);
    for (uint32_t i = 0; i < NMB - 4; i++) {
        const uint32_t l3 = l3s[i % 3];
        if (i == 5) {
            CHECK(e[i] == (E_DROP | E_CK) && get64(mb(i) + 56) == 0xABABABABABABABABull);
            CHECK(get16(mb(i) + 24) == 192 + 5);
            continue;
        }
        CHECK(e[i] == E_RECV);
        CHECK(get64(mb(i) + 56) == (i % 5 == 4 ? 0 : 0x1122334455667788ull));
        CHECK(get16(mb(i) + 24) == 192 + i % 16 + l3 + 8 && get16(mb(i) + 30) == lens[i % 6] - 8);
        const uint8_t *md = mb(i) + 64;
        CHECK(md[0] == 2 && md[1] == 4 && md[2] == 0x9C && md[3] == 0x40 && md[4] == 198 && md[7] == 1 && md[8] == 0 &&
              md[19] == 0 && md[20] == 2 && md[21] == 4 && md[24] == 10 && md[27] == 7 && md[39] == 0);
    }
    CHECK(e[NMB - 4] == E_PDROP && e[NMB - 3] == E_PDROP && e[NMB - 2] == E_PUNT && e[NMB - 1] == E_RECV);
    CHECK(get64(mb(NMB - 2) + 56) == 0 && get64(mb(NMB - 4) + 56) == 0xABABABABABABABABull);

    /* flags: TCP on, punt off */
    CHECK(cndp_pcb_set_flags(t, 0, 1) == 0);
    put(NMB - 3, 192, 20, 26, 6, 5002, 1984);
    put(NMB - 2, 193, 20, 26, 17, 4999, 1984);
    CHECK(cndp_udp_input_node_host(t, ptrs + NMB - 3, 2, e, NULL, 0, NULL) == 0);
    CHECK(e[0] == E_TCP && e[1] == E_DROP);

    /* total_length past the region's end, past the buffer's end and past stage_max:
     * zeros are read, nothing outside is touched */
    for (uint32_t k = 0; k < 3; k++) {
        put(NMB - 1, 1984 - 24 - 100 + 1 + 7 * k, 24, 100, 17, 5002, 1984);
        CHECK(cndp_udp_input_node_host(t, ptrs + NMB - 1, 1, e, end, 0, NULL) == 0);
        CHECK((e[0] & 0xFF00u) == 0x0400u);
    }
    put(10, 192, 20, 400, 17, 5002, 192 + 20 + 399); /* the buffer ends one byte early */
    CHECK(cndp_udp_input_node_host(t, ptrs + 10, 1, e, NULL, 0, NULL) == 0 && (e[0] & 0xFF00u) == 0x0400u);
    put(10, 192, 20, 400, 17, 5002, 1984);
    CHECK(cndp_udp_input_node_host(t, ptrs + 10, 1, e, NULL, 128, NULL) == 0 && (e[0] & 0xFF00u) == 0x0400u);
    put(10, 192, 20, 400, 17, 5002, 1984);
    CHECK(cndp_udp_input_node_host(t, ptrs + 10, 1, e, NULL, 2048, NULL) == 0 && e[0] == E_RECV);
    /* a frame that begins at the region's end, an mbuf whose header crosses it, a NULL entry */
    put(NMB - 1, 1984, 20, 26, 17, 5002, 4000);
    void *odd[3] = {mb(NMB - 1), NULL, mb(NMB - 1)};
    CHECK(cndp_udp_input_node_host(t, odd, 3, e, end, 0, NULL) == 0 && e[0] == E_NONE && e[1] == E_NONE);
    CHECK(cndp_udp_input_node_host(t, odd, 1, e, pool + (size_t)(NMB - 1) * FRAME + 63, 0, NULL) == 0 && e[0] == E_NONE);

    /* a hook that answers NULL for every fourth mbuf and m + 128 for the rest */
    for (uint32_t i = 0; i < 16; i++)
        put(i, 200, 20, 64, 17, 5002, 1984);
    CHECK(cndp_udp_input_node_host(t, ptrs, 16, e, end, 0, md_some) == 0);
    for (uint32_t i = 0; i < 16; i++) {
        if (i % 4 == 3) {
            CHECK(e[i] == E_DROP && get64(mb(i) + 56) == 0xABABABABABABABABull && get16(mb(i) + 24) == 200);
        } else {
            CHECK(e[i] == E_RECV && mb(i)[128] == 2 && mb(i)[128 + 20] == 2 && get16(mb(i) + 24) == 228);
        }
    }
    /* delete resets the user value */
    CHECK(cndp_pcb_del(t, 1) == 0 && cndp_pcb_user_get(t, 1, &uv) == 0 && uv == 1);
    /* argument checks */
    CHECK(cndp_udp_input_node_host(NULL, ptrs, 1, e, NULL, 0, NULL) == -22);
    CHECK(cndp_udp_input_node_host(t, NULL, 1, e, NULL, 0, NULL) == -22);
    CHECK(cndp_udp_input_node_host(t, ptrs, 1, NULL, NULL, 0, NULL) == -22);
    CHECK(cndp_udp_input_node_host(t, ptrs, 257, e, NULL, 0, NULL) == -22);
    CHECK(cndp_udp_input_node_host(t, NULL, 0, NULL, NULL, 0, NULL) == 0);
    cndp_pcb_free(t);
    free(pool);
    printf("PASS\n");
    return 0;
}

/* pcb.c under -fsanitize=address,undefined: add / delete / lookup sequences,
 * the full table, zeroed entries, and the device image rebuilt after every
 * change (its directory must send every port to its run).  Prints PASS and
 * exits 0; any check that fails exits 1, a sanitizer report aborts. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cndp_amd/csrc/pcb_internal.h"

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            exit(1);                                                 \
        }                                                            \
    } while (0)

static uint32_t rnd_state = 12345;
static uint32_t rnd(uint32_t m)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return (rnd_state >> 8) % m;
}

/* every entry is reachable through the image's directory, in index order */
static void check_image(struct cndp_pcb_tbl *t)
{
    pthread_mutex_lock(&t->lock);
    CHECK(pcb_image(t) == 0);
    const uint32_t n = t->img[0], H = t->img[1];
    CHECK(n == t->count && (H & (H - 1)) == 0 && H >= 2 && t->img[3] == t->img_words);
    const uint32_t *pp = t->img + PCB_IMG_HDR + 2 * n, *slots = pp + n;
    const uint16_t *idxf = (const uint16_t *)(slots + H);
    uint32_t seen = 0;
    for (uint32_t port = 0; port < 65536; port++) {
        uint32_t h = pcb_port_hash(port, H), probes = 0;
        while ((slots[h] & PCB_SLOT_VALID) && ((slots[h] >> 12) & 0xffffu) != port) {
            h = (h + 1) & (H - 1);
            CHECK(++probes < H);
        }
        if (!(slots[h] & PCB_SLOT_VALID))
            continue;
        uint32_t last = 0, first = 1;
        for (uint32_t j = slots[h] & 0xfffu; j < n && (pp[j] >> 16) == port; j++, seen++) {
            uint32_t i = idxf[j] & PCB_IDXF_IDX;
            CHECK(i < n && t->vec[i].lport == port && (first || i > last));
            CHECK(!!(idxf[j] & PCB_IDXF_CKSUM) == !!(t->vec[i].opt_flag & CNDP_UDP_CHKSUM_FLAG));
            last = i;
            first = 0;
        }
    }
    CHECK(seen == n);
    pthread_mutex_unlock(&t->lock);
}

int main(void)
{
    cndp_pcb_tbl_t *t = NULL;
    CHECK(cndp_pcb_create(0, &t) == -EINVAL);
    CHECK(cndp_pcb_create(CNDP_PCB_MAX_ENTRIES + 1, &t) == -EINVAL);
    CHECK(cndp_pcb_create(8, NULL) == -EINVAL);

    /* a small table filled to the brim */
    CHECK(cndp_pcb_create(8, &t) == 0);
    check_image(t);
    struct cndp_pcb_key k = {.laddr = 0x0100000a, .faddr = 0x0200000a, .lport = 0x8813, .fport = 0x0900};
    uint32_t idx = 7;
    CHECK(cndp_pcb_lookup(t, &k, 1, &idx) == 0 && idx == CNDP_PCB_NONE);
    for (int i = 0; i < 8; i++) {
        struct cndp_pcb_entry e = {.laddr = i & 1 ? k.laddr : 0, .lport = k.lport, .opt_flag = i & 2 ? 0x80 : 0};
        CHECK(cndp_pcb_add(t, &e) == i);
    }
    struct cndp_pcb_entry extra = {.lport = 1};
    CHECK(cndp_pcb_add(t, &extra) == -ENOSPC);
    CHECK(cndp_pcb_add(t, NULL) == -EINVAL);
    CHECK(cndp_pcb_count(t) == 8);
    CHECK(cndp_pcb_lookup(t, &k, 1, &idx) == 0 && idx == 1); /* bound beats any/any, first of them */
    CHECK(cndp_pcb_del(t, 8) == -EINVAL);
    CHECK(cndp_pcb_del(t, 1) == 0);
    CHECK(cndp_pcb_del(t, 1) == -ENOENT);
    CHECK(cndp_pcb_count(t) == 8); /* the zeroed entry stays in the vector */
    CHECK(cndp_pcb_lookup(t, &k, 1, &idx) == 0 && idx == 3);
    /* ... and answers local port 0 as an any/any entry */
    struct cndp_pcb_key k0 = {.laddr = k.laddr, .faddr = k.faddr, .lport = 0, .fport = 5};
    CHECK(cndp_pcb_lookup(t, &k0, 1, &idx) == 0 && idx == 1);
    check_image(t);
    CHECK(cndp_pcb_set_flags(t, 0, 1) == 0);
    check_image(t);
    CHECK(t->img[2] == PCB_F_TCP);
    cndp_pcb_free(t);

    /* the largest table: random adds and deletes, many ports, lookups between */
    CHECK(cndp_pcb_create(CNDP_PCB_MAX_ENTRIES, &t) == 0);
    struct cndp_pcb_key keys[64];
    uint32_t out[64];
    for (uint32_t i = 0; i < CNDP_PCB_MAX_ENTRIES; i++) {
        struct cndp_pcb_entry e = {.laddr = rnd(4), .faddr = rnd(3), .lport = (uint16_t)(i < 3000 ? i : rnd(16)),
                                   .fport = (uint16_t)rnd(4), .opt_flag = (uint16_t)(rnd(2) * 0x80)};
        CHECK(cndp_pcb_add(t, &e) == (int)i);
        if (i % 5 == 4) {
            int r = cndp_pcb_del(t, rnd(i + 1));
            CHECK(r == 0 || r == -ENOENT);
        }
        if (i % 512 == 511 || i < 4) {
            check_image(t);
            for (int q = 0; q < 64; q++)
                keys[q] = (struct cndp_pcb_key){.laddr = rnd(4), .faddr = rnd(3), .lport = (uint16_t)rnd(20),
                                                .fport = (uint16_t)rnd(4)};
            CHECK(cndp_pcb_lookup(t, keys, 64, out) == 0);
            for (int q = 0; q < 64; q++)
                CHECK(out[q] == CNDP_PCB_NONE || out[q] <= i);
        }
    }
    CHECK(cndp_pcb_add(t, &extra) == -ENOSPC);
    CHECK(cndp_pcb_lookup(t, NULL, 0, NULL) == 0);
    CHECK(cndp_pcb_lookup(t, NULL, 1, out) == -EINVAL);
    check_image(t);
    cndp_pcb_free(t);
    cndp_pcb_free(NULL);
    puts("PASS");
    return 0;
}

/* The TCP index of pcb.c (pcb_tcp_image, cndp_pcb_lookup_indexed) under
 * -fsanitize=address,undefined: tables grown and shrunk between lookups, the
 * fullest table with every tuple distinct and every port distinct (the largest
 * image), one port holding every connection, and the image's own invariants
 * after every rebuild.  Every indexed answer is compared with the linear
 * cndp_pcb_lookup.  Prints PASS and exits 0; any check that fails exits 1, a
 * sanitizer report aborts. */
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

static uint32_t rnd_state = 4242;
static uint32_t rnd(uint32_t m)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return (rnd_state >> 8) % m;
}

/* The image's invariants: sizes, every entry present once, runs ordered
 * (wildcards first, each part by index), every fully specified tuple reachable
 * from its hash slot for its lowest index, chains short.  Returns the longest
 * exact-hash chain walked. */
static uint32_t check_image(struct cndp_pcb_tbl *t)
{
    pthread_mutex_lock(&t->lock);
    CHECK(pcb_tcp_image(t) == 0);
    const uint32_t *img = t->timg;
    const uint32_t n = img[0], HE = img[1], HP = img[4], nfull = img[5];
    CHECK(n == t->count && img[2] == t->flags && img[3] == t->timg_words);
    CHECK((HE & (HE - 1)) == 0 && HE >= 2 && HE >= 2 * nfull && (HP & (HP - 1)) == 0 && HP >= 2);
    CHECK(img[3] == TCB_IMG_WORDS(n, HE, HP) && img[3] * 4u <= 160u * 1024u - 256u);
    const uint32_t *la = img + TCB_IMG_HDR, *fa = la + n, *pp = fa + n, *es = pp + n, *ps = es + HE;
    const uint16_t *idx = (const uint16_t *)(ps + HP);
    uint8_t *seen = calloc(n ? n : 1, 1);
    CHECK(seen);
    uint32_t full = 0;
    for (uint32_t j = 0; j < n; j++) {
        uint32_t i = idx[j];
        CHECK(i < n && !seen[i]);
        seen[i] = 1;
        const struct cndp_pcb_entry *e = &t->vec[i];
        CHECK(la[j] == e->laddr && fa[j] == e->faddr && pp[j] == ((uint32_t)e->fport | (uint32_t)e->lport << 16));
        int f = e->laddr != 0 && e->faddr != 0;
        full += (uint32_t)f;
        if (j && (pp[j - 1] >> 16) == (pp[j] >> 16)) {
            int fprev = la[j - 1] != 0 && fa[j - 1] != 0;
            CHECK(fprev <= f && (fprev != f || idx[j - 1] < i));
        } else if (j)
            CHECK((pp[j - 1] >> 16) < (pp[j] >> 16));
    }
    CHECK(full == nfull);
    free(seen);
    uint32_t used = 0, longest = 0;
    for (uint32_t h = 0; h < HE; h++)
        used += !!(es[h] & PCB_SLOT_VALID);
    CHECK(used <= nfull);
    for (uint32_t j = 0; j < n; j++) {
        if (!(la[j] != 0 && fa[j] != 0))
            continue;
        uint32_t x = pcb_tcp_hash(la[j], fa[j], pp[j]), h = x & (HE - 1), probes = 1;
        for (;; h = (h + 1) & (HE - 1), probes++) {
            CHECK(es[h] & PCB_SLOT_VALID);
            uint32_t q = es[h] & 0xfffu;
            if (la[q] == la[j] && fa[q] == fa[j] && pp[q] == pp[j]) {
                CHECK(((es[h] >> 12) & 0x7ffffu) == x >> 13 && idx[q] <= idx[j]);
                break;
            }
        }
        if (probes > longest)
            longest = probes;
    }
    pthread_mutex_unlock(&t->lock);
    return longest;
}

static void same_as_linear(cndp_pcb_tbl_t *t, const struct cndp_pcb_key *keys, uint32_t n)
{
    uint32_t *a = malloc((n ? n : 1) * sizeof(uint32_t)), *b = malloc((n ? n : 1) * sizeof(uint32_t));
    CHECK(a && b);
    CHECK(cndp_pcb_lookup(t, keys, n, a) == 0 && cndp_pcb_lookup_indexed(t, keys, n, b) == 0);
    for (uint32_t k = 0; k < n; k++)
        if (a[k] != b[k]) {
            fprintf(stderr, "key %u (%08x %08x %04x %04x): linear %u indexed %u\n", k, keys[k].laddr,
                    keys[k].faddr, keys[k].lport, keys[k].fport, a[k], b[k]);
            exit(1);
        }
    free(a);
    free(b);
}

static struct cndp_pcb_key rnd_key(uint32_t addrs, uint32_t ports)
{
    return (struct cndp_pcb_key){.laddr = rnd(addrs), .faddr = rnd(addrs), .lport = (uint16_t)rnd(ports),
                                 .fport = (uint16_t)rnd(ports)};
}

int main(void)
{
    cndp_pcb_tbl_t *t = NULL;
    uint32_t out[4];
    struct cndp_pcb_key k1 = {.laddr = 1, .faddr = 2, .lport = 3, .fport = 4};

    CHECK(cndp_pcb_lookup_indexed(NULL, &k1, 1, out) == -EINVAL);
    CHECK(cndp_pcb_create(1, &t) == 0);
    CHECK(cndp_pcb_lookup_indexed(t, NULL, 1, out) == -EINVAL);
    CHECK(cndp_pcb_lookup_indexed(t, &k1, 1, NULL) == -EINVAL);
    CHECK(cndp_pcb_lookup_indexed(t, NULL, 0, NULL) == 0);
    CHECK(cndp_pcb_lookup_indexed(t, &k1, 1, out) == 0 && out[0] == CNDP_PCB_NONE); /* empty */
    check_image(t);
    struct cndp_pcb_entry e1 = {.laddr = 1, .faddr = 2, .lport = 3, .fport = 4};
    CHECK(cndp_pcb_add(t, &e1) == 0);
    CHECK(cndp_pcb_lookup_indexed(t, &k1, 1, out) == 0 && out[0] == 0);
    CHECK(cndp_pcb_del(t, 0) == 0);
    CHECK(cndp_pcb_lookup_indexed(t, &k1, 1, out) == 0 && out[0] == CNDP_PCB_NONE);
    k1.lport = 0;
    CHECK(cndp_pcb_lookup_indexed(t, &k1, 1, out) == 0 && out[0] == 0); /* zeroed: any/any on port 0 */
    check_image(t);
    cndp_pcb_free(t);

    /* a small pool: collisions, duplicates, listeners, deletes, lookups between changes */
    enum { NK = 512 };
    static struct cndp_pcb_key keys[NK];
    CHECK(cndp_pcb_create(CNDP_PCB_MAX_ENTRIES, &t) == 0);
    for (uint32_t i = 0; i < CNDP_PCB_MAX_ENTRIES; i++) {
        struct cndp_pcb_entry e = {.laddr = rnd(4), .faddr = rnd(4), .lport = (uint16_t)rnd(6),
                                   .fport = (uint16_t)rnd(6), .opt_flag = (uint16_t)rnd(2)};
        CHECK(cndp_pcb_add(t, &e) == (int)i);
        if (i % 7 == 6) {
            int r = cndp_pcb_del(t, rnd(i + 1));
            CHECK(r == 0 || r == -ENOENT);
        }
        if (i % 256 == 255 || i < 8) {
            check_image(t);
            for (int q = 0; q < NK; q++)
                keys[q] = rnd_key(5, 7);
            same_as_linear(t, keys, NK);
        }
    }
    cndp_pcb_free(t);

    /* the largest image: 4096 distinct tuples on 4096 distinct ports */
    CHECK(cndp_pcb_create(CNDP_PCB_MAX_ENTRIES, &t) == 0);
    for (uint32_t i = 0; i < CNDP_PCB_MAX_ENTRIES; i++) {
        struct cndp_pcb_entry e = {.laddr = 0x0a000001, .faddr = 0xc6120000 + i, .lport = (uint16_t)(i * 16 + 1),
                                   .fport = (uint16_t)i};
        CHECK(cndp_pcb_add(t, &e) == (int)i);
    }
    check_image(t);
    pthread_mutex_lock(&t->lock);
    CHECK(t->timg_words == TCB_IMG_WORDS(4096u, 8192u, 8192u)); /* 30728 words */
    pthread_mutex_unlock(&t->lock);
    for (int q = 0; q < NK; q++) {
        uint32_t i = rnd(CNDP_PCB_MAX_ENTRIES + 64);
        keys[q] = (struct cndp_pcb_key){.laddr = q % 9 ? 0x0a000001 : 0, .faddr = q % 11 ? 0xc6120000 + i : 0,
                                        .lport = (uint16_t)(i * 16 + 1), .fport = (uint16_t)i};
    }
    same_as_linear(t, keys, NK);
    cndp_pcb_free(t);

    /* one port, every connection on it, tuples that differ in one byte only */
    CHECK(cndp_pcb_create(CNDP_PCB_MAX_ENTRIES, &t) == 0);
    for (uint32_t i = 0; i < CNDP_PCB_MAX_ENTRIES; i++) {
        struct cndp_pcb_entry e = {.laddr = 0x0104040a, .faddr = 0x000012c6u | (i & 0xffu) << 24 | 0x10000u,
                                   .lport = 0x5000, .fport = (uint16_t)((i >> 8) & 1 ? 0x0100u << (i >> 9) : 1u << (i >> 9))};
        if (i == 2000)
            e = (struct cndp_pcb_entry){.lport = 0x5000}; /* the listener */
        CHECK(cndp_pcb_add(t, &e) == (int)i);
    }
    uint32_t longest = check_image(t);
    CHECK(longest <= 24); /* a hash that dropped those bytes would chain hundreds */
    for (int q = 0; q < NK; q++)
        keys[q] = (struct cndp_pcb_key){.laddr = q % 13 ? 0x0104040a : rnd(2), .faddr = 0x000012c6u | rnd(300) << 24 | 0x10000u,
                                        .lport = 0x5000, .fport = (uint16_t)(rnd(2) ? 0x0100u << rnd(8) : 1u << rnd(8))};
    same_as_linear(t, keys, NK);
    for (uint32_t i = 0; i < CNDP_PCB_MAX_ENTRIES; i += 3)
        CHECK(cndp_pcb_del(t, i) == 0);
    check_image(t);
    same_as_linear(t, keys, NK);
    CHECK(cndp_pcb_del(t, 2000) == 0 || 2000 % 3 == 0);
    same_as_linear(t, keys, NK);
    cndp_pcb_free(t);
    puts("PASS");
    return 0;
}

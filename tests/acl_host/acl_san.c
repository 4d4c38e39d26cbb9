/* acl.c (cndp_acl_*, cndp_acl_classify_host) under -fsanitize=address,undefined:
 * add, clear, build, the error ladder, a table without an image, the default
 * rules and a 100000-rule build, each classified over a few hundred frames in
 * heap buffers sized exactly to them and compared with a first-match loop over
 * the rule vector.  Prints PASS and exits 0; any check that fails exits 1, a
 * sanitizer report aborts. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cndp_amd/csrc/acl_internal.h"

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            exit(1);                                                 \
        }                                                            \
    } while (0)

static uint32_t rnd_state = 0x2545F491u;
static uint32_t rnd(void)
{
    rnd_state ^= rnd_state << 13;
    rnd_state ^= rnd_state >> 17;
    rnd_state ^= rnd_state << 5;
    return rnd_state;
}

static uint32_t brute(cndp_acl_tbl_t *t, uint32_t n_img, uint32_t src, uint32_t dst)
{
    for (uint32_t k = 0; k < n_img; k++) {
        struct cndp_acl_rule r;
        CHECK(cndp_acl_get(t, k, &r) == 0);
        if (!((src ^ r.src_addr) & acl_mask(r.src_msk)) && !((dst ^ r.dst_addr) & acl_mask(r.dst_msk)))
            return k + (r.deny ? CNDP_ACL_DENY_SIGNATURE : 1u);
    }
    return 0;
}

static void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

/* n frames of 34 bytes in a heap slab of exactly 34 n bytes, drawn from the
 * first n_img rules; every output array is sized exactly as well */
static void run(cndp_acl_tbl_t *t, uint32_t n_img, uint32_t n, uint32_t mode)
{
    uint8_t *slab = malloc((size_t)34 * n), *verdict = malloc(n), *tx = malloc(n), *want_slab = malloc((size_t)34 * n);
    uint32_t *res = malloc(4u * n);
    uint16_t *bin = malloc(2u * n), *len = malloc(2u * n);
    CHECK(slab && verdict && tx && res && bin && len && want_slab);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t *f = slab + 34u * i;
        for (uint32_t k = 0; k < 34; k++)
            f[k] = (uint8_t)rnd();
        struct cndp_acl_rule r;
        CHECK(cndp_acl_get(t, rnd() % n_img, &r) == 0);
        uint32_t src = (r.src_addr & acl_mask(r.src_msk)) | (rnd() & ~acl_mask(r.src_msk));
        uint32_t dst = (r.dst_addr & acl_mask(r.dst_msk)) | (rnd() & ~acl_mask(r.dst_msk));
        if (i % 5 == 0)
            src ^= 0x80000000u;
        f[5] = (uint8_t)(i % 4);
        f[14] = i % 17 == 3 ? 0x65 : i % 17 == 4 ? 0x44 : 0x45 + (uint8_t)(i % 3);
        f[16] = 0, f[17] = i % 19 == 5 ? 19 : 20;
        put_be32(f + 26, src);
        put_be32(f + 30, dst);
        len[i] = i % 23 == 7 ? 19 : 34;
    }
    memcpy(want_slab, slab, (size_t)34 * n);
    struct cndp_batch b;
    memset(&b, 0, sizeof(b));
    b.n = n, b.slab = slab, b.slab_len = (uint64_t)34 * n, b.stride = 34;
    struct cndp_acl_io io;
    memset(&io, 0, sizeof(io));
    uint64_t st[CNDP_ACL_NSTATS] = {5, 6, 7}, want[CNDP_ACL_NSTATS] = {5, 6, 7};
    io.len = len, io.in_lport = 2, io.lport_mask[0] = 0x5, io.result = res, io.verdict = verdict, io.tx_lport = tx;
    io.bin_of = bin, io.n_bins = 3, io.stats = st;
    CHECK(cndp_acl_classify_host(t, &b, mode, CNDP_ACL_F_MAC_SWAP, &io) == 0);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t *f = want_slab + 34u * i;
        const int ok = len[i] >= 20 && (f[14] >> 4) == 4 && (f[14] & 15) >= 5 && f[17] >= 20;
        const uint32_t w = ok ? brute(t, n_img, (uint32_t)f[26] << 24 | f[27] << 16 | f[28] << 8 | f[29],
                                      (uint32_t)f[30] << 24 | f[31] << 16 | f[32] << 8 | f[33]) : 0u;
        const int fwd = ok && !(w & CNDP_ACL_DENY_SIGNATURE) && (w || mode == CNDP_ACL_PERMISSIVE);
        const uint32_t v = !ok ? CNDP_ACL_PREFILTER : fwd ? CNDP_ACL_FORWARD : CNDP_ACL_DENY;
        const uint32_t port = !fwd ? CNDP_ACL_LPORT_NONE : (f[5] == 0 || f[5] == 2) ? f[5] : 2u;
        CHECK(res[i] == w && verdict[i] == v && tx[i] == port);
        CHECK(bin[i] == (fwd ? port : v == CNDP_ACL_DENY ? 3u : 4u));
        want[v - 1u]++;
        if (fwd) {
            uint8_t m[6];
            memcpy(m, f, 6), memcpy(f, f + 6, 6), memcpy(f + 6, m, 6);
        }
    }
    CHECK(!memcmp(slab, want_slab, (size_t)34 * n) && !memcmp(st, want, sizeof(st)));
    free(slab), free(verdict), free(tx), free(res), free(bin), free(len), free(want_slab);
}

int main(void)
{
    cndp_acl_tbl_t *t = NULL;
    struct cndp_acl_rule r = {0x0A000001u, 0xC0000201u, 32, 24, 1, 0}, g;
    CHECK(cndp_acl_tbl_create(NULL) == -EINVAL && cndp_acl_tbl_create(&t) == 0);
    CHECK(cndp_acl_add(NULL, &r) == -EINVAL && cndp_acl_add(t, NULL) == -EINVAL && cndp_acl_count(NULL) == -EINVAL);
    CHECK(cndp_acl_build(NULL) == -EINVAL && cndp_acl_clear(NULL) == -EINVAL && cndp_acl_get(t, 0, &g) == -EINVAL);
    r.src_msk = 33;
    CHECK(cndp_acl_add(t, &r) == -EINVAL);
    r.src_msk = 32, r.dst_msk = 33;
    CHECK(cndp_acl_add(t, &r) == -EINVAL && cndp_acl_count(t) == 0);

    /* no image: a build on zero rules fails and classify answers -ENOENT, writing nothing */
    uint8_t frame[34] = {0}, v1 = 0xAA;
    struct cndp_batch b;
    memset(&b, 0, sizeof(b));
    b.n = 1, b.slab = frame, b.slab_len = sizeof(frame), b.stride = 34;
    struct cndp_acl_io io;
    memset(&io, 0, sizeof(io));
    io.verdict = &v1;
    CHECK(cndp_acl_build(t) == -EINVAL);
    CHECK(cndp_acl_classify_host(t, &b, CNDP_ACL_STRICT, 0, &io) == -ENOENT && v1 == 0xAA);
    CHECK(cndp_acl_classify_host(t, &b, 2, 0, &io) == -EINVAL && cndp_acl_classify_host(t, &b, 0, 2, &io) == -EINVAL);

    /* the default rules */
    CHECK(cndp_acl_add_init_rules(t) == 0 && cndp_acl_count(t) == (int)CNDP_ACL_INIT_RULES);
    CHECK(cndp_acl_get(t, 4225, &g) == 0 && g.src_addr == 0xD2000FFFu && g.dst_addr == 0x6E000FFFu && !g.deny);
    CHECK(cndp_acl_get(t, 4226, &g) == -EINVAL);
    CHECK(cndp_acl_build(t) == 0);
    run(t, CNDP_ACL_INIT_RULES, 300, CNDP_ACL_STRICT);
    run(t, CNDP_ACL_INIT_RULES, 300, CNDP_ACL_PERMISSIVE);

    /* rules added or cleared after a build are invisible until the next one */
    CHECK(cndp_acl_clear(t) == 0 && cndp_acl_count(t) == 0);
    frame[14] = 0x45, frame[17] = 20;
    put_be32(frame + 26, 0xD2000001u), put_be32(frame + 30, 0x6E000001u);
    uint32_t res = 0;
    io.result = &res;
    CHECK(cndp_acl_classify_host(t, &b, CNDP_ACL_STRICT, 0, &io) == 0 && res == 130u + 1u + 1u);
    CHECK(cndp_acl_build(t) == -EINVAL); /* the image is gone with the failed build */
    CHECK(cndp_acl_classify_host(t, &b, CNDP_ACL_STRICT, 0, &io) == -ENOENT);

    /* up to the cap: 90000 /32:/32, then mixed lengths, duplicates and a /0:/0 */
    static const uint8_t lens[] = {0, 1, 7, 8, 9, 16, 17, 24, 31, 32};
    for (uint32_t i = 0; i < CNDP_ACL_MAX_RULES; i++) {
        struct cndp_acl_rule q = {0x0B000000u + 7u * (i % 90000u), 0xC0A80000u + 13u * (i % 90000u), 32, 32,
                                  (uint8_t)(i % 3u == 0), 0};
        if (i >= 90000u) {
            q.src_msk = lens[rnd() % 10u], q.dst_msk = lens[rnd() % 10u];
            if (i == 95000u)
                q.src_msk = q.dst_msk = 0;
        }
        CHECK(cndp_acl_add(t, &q) == 0);
    }
    CHECK(cndp_acl_add(t, &r) == -EINVAL); /* still the bad mask */
    r.dst_msk = 24;
    CHECK(cndp_acl_add(t, &r) == -ENOSPC && cndp_acl_add_init_rules(t) == -ENOSPC);
    CHECK(cndp_acl_count(t) == (int)CNDP_ACL_MAX_RULES && cndp_acl_build(t) == 0);
    run(t, CNDP_ACL_MAX_RULES, 200, CNDP_ACL_STRICT);
    CHECK(cndp_acl_build(t) == 0); /* a rebuild replaces the image */
    run(t, CNDP_ACL_MAX_RULES, 100, CNDP_ACL_PERMISSIVE);
    cndp_acl_tbl_destroy(t);
    cndp_acl_tbl_destroy(NULL);
    puts("PASS");
    return 0;
}

/*
 * tcpout.c -- include/cndp_tcpout.h on the host: the PCB key image, and
 * tcp_output's mbuf build + tcp_send_segment
 * (lib/cnet/tcp/cnet_tcp.c:836-870, :371-517) and tcp_drop_with_reset +
 * tcp_do_response (:1120-1149, :1020-1108) frame by frame over host memory.  The
 * transmit attributes themselves live in tcb.c, with the TCB image.  Plain C, no
 * HIP: it also builds into a stand-alone program (tests/tcpout_host).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "tcpout_internal.h"

uint32_t cndp_tcp_send_optlen(uint8_t tcb_tflags, uint8_t seg_flags) { return tout_optlen(tcb_tflags, seg_flags); }

int tcpout_key_image(struct cndp_tcb_tbl *t)
{
    struct cndp_pcb_tbl *p = t->pcb;
    int r = 0;
    pthread_mutex_lock(&p->lock);
    if (t->kimg_gen != p->gen || !t->kimg) {
        if (!t->kimg)
            t->kimg = calloc((size_t)t->cap * TOK_WORDS, sizeof(uint32_t));
        if (!t->kimg)
            r = -ENOMEM;
        else {
            for (uint32_t i = 0; i < p->count; i++) {
                uint32_t *k = t->kimg + (size_t)i * TOK_WORDS;
                const struct cndp_pcb_entry *e = &p->vec[i];
                const int live = !p->closed[i];
                k[0] = live ? e->laddr : 0u;
                k[1] = live ? e->faddr : 0u;
                k[2] = live ? (uint32_t)e->fport | (uint32_t)e->lport << 16 : 0u;
                k[3] = live ? TOK_LIVE : 0u;
            }
            t->kimg_gen = p->gen;
        }
    }
    pthread_mutex_unlock(&p->lock);
    return r;
}

struct span {
    uint8_t *slab;
    uint64_t len;
};

static inline uint32_t rd8(const struct span *s, uint64_t o) { return o < s->len ? s->slab[o] : 0u; }
static inline void wr8(const struct span *s, uint64_t o, uint32_t v)
{
    if (o < s->len)
        s->slab[o] = (uint8_t)v;
}

int cndp_tcp_output_host(cndp_tcb_tbl_t *t, uint32_t mode, uint32_t now, void *slab, uint64_t slab_len,
                         uint64_t stride, const uint64_t *offsets, uint32_t data_off, uint32_t n,
                         const struct cndp_tcpout_io *io)
{
    if (!t || !io || mode > CNDP_TCPOUT_RESPOND)
        return -EINVAL;
    const int desc = io->txseg != NULL;
    if (n && (!slab || !io->pcb || !io->len || !io->faddr || !io->laddr || !io->taken || (slab_len >> 63) ||
              ((uintptr_t)io->txseg & 15u) || ((uintptr_t)io->seg & 15u) || (io->snd && !io->src_off) ||
              (mode == CNDP_TCPOUT_SEGMENT ? !desc : desc ? !io->sel : (!io->seg || (!io->sel && !io->verdict)))))
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    (void)tcb_reconcile(t);
    int r = tcpout_key_image(t);
    if (r) {
        pthread_mutex_unlock(&t->lock);
        return r;
    }
    static const uint32_t none[TCB_WORDS];
    const struct span s = {(uint8_t *)slab, slab_len};
    const uint8_t *snd = mode == CNDP_TCPOUT_SEGMENT ? (const uint8_t *)io->snd : NULL;
    uint64_t st[CNDP_TCPOUT_NSTATS] = {0};
    for (uint32_t i = 0; i < n; i++) {
        uint32_t w[TOUT_WORDS], optlen = 0, plen = 0, v = CNDP_TCPOUT_STAT_NOTSEL;
        const int cand = io->sel ? io->sel[i] != 0
                                 : mode == CNDP_TCPOUT_SEGMENT || (io->verdict[i] & CNDP_TCPSEG_VERDICT) == CNDP_TCPSEG_RESET;
        const uint64_t base = (offsets ? offsets[i] : (uint64_t)i * stride) + data_off;
        const uint32_t *k = none;
        if (cand) {
            const uint32_t p = io->pcb[i];
            const uint32_t *e = none;
            if (p < t->cap) { /* CNDP_PCB_NONE is above every capacity */
                k = t->kimg + (size_t)p * TOK_WORDS;
                e = t->img + (size_t)p * TCB_WORDS;
            }
            uint32_t rec[4];
            memcpy(rec, desc ? (const void *)&io->txseg[i] : (const void *)&io->seg[i], sizeof(rec));
            int mc = 0;
            if (mode == CNDP_TCPOUT_RESPOND && !desc && io->rxmeta) {
                const uint64_t ip = base + CNDP_RXMETA_L2(io->rxmeta[i]) + 16u;
                const uint32_t dst = rd8(&s, ip) | rd8(&s, ip + 1) << 8 | rd8(&s, ip + 2) << 16 | rd8(&s, ip + 3) << 24;
                mc = tout_ip_mcast(dst) || (rd8(&s, base) & 1u);
            }
            v = tout_frame(mode, desc, k, e, rec, mc, now, w, &optlen, &plen);
        }
        const int taken = v == CNDP_TCPOUT_STAT_SENT;
        if (taken) {
            if (mode == CNDP_TCPOUT_SEGMENT) { /* the memset of :862-863 and tcp_mbuf_copydata, both at P */
                const uint64_t P = base + TOUT_PAY + optlen;
                const uint32_t ztot = TOUT_PAY + optlen;
                uint64_t avail = 0;
                if (snd && io->src_off[i] < io->snd_len)
                    avail = io->snd_len - io->src_off[i];
                if (snd)
                    for (uint32_t q = 0; q < plen; q++)
                        wr8(&s, P + q, q < avail ? snd[io->src_off[i] + q] : 0u);
                for (uint32_t q = plen; q < ztot; q++)
                    wr8(&s, P + q, 0);
            }
            for (uint32_t q = 0; q < 20u + optlen; q++)
                wr8(&s, base + TOUT_HDR + q, w[q >> 2] >> (8u * (q & 3u)));
            if (optlen)
                st[CNDP_TCPOUT_STAT_OPTS]++;
        }
        io->len[i] = taken ? (uint16_t)(20u + optlen + plen) : 0;
        io->faddr[i] = taken ? k[1] : 0u;
        io->laddr[i] = taken ? k[0] : 0u;
        io->taken[i] = (uint8_t)taken;
        st[v]++;
    }
    if (io->stats)
        for (int q = 0; q < CNDP_TCPOUT_NSTATS; q++)
            io->stats[q] += st[q];
    pthread_mutex_unlock(&t->lock);
    return 0;
}

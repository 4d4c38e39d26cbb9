/*
 * tcb.c -- the TCB table of include/cndp_tcb.h: a per-PCB snapshot of what
 * cnet_tcp_input reads of a connection between "Segment Arrives" and the end of
 * the header-prediction tests (lib/cnet/tcp/cnet_tcp.c:3425-3482, :3214-3281),
 * kept as the image the device stage mirrors, the stage's rule on the host
 * (cndp_tcp_segment_host), and the mbuf queue's CNDP_MQ_TCP_SEGMENT mode on the
 * host (cndp_tcp_segment_node_host, include/cndp_mqtcb.h).  Plain C, no HIP: it also builds into a stand-alone
 * program (tests/tcb_host).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/cndp_mqtcb.h"
#include "../../include/cndp_tcpout.h"
#include "tcb_internal.h"

#define EDGE_SEG CNDP_L4_EDGE(CNDP_L4_NODE_TCP_INPUT, CNDP_TCP_INPUT_SEGMENT)
_Static_assert(PCB_TCP_OPT_WORDS == TCB_OPT_WORDS, "pcb.c's walk hands over the option words tcb_segment() reads");

int cndp_tcb_tbl_create(cndp_pcb_tbl_t *pcb_tbl, cndp_tcb_tbl_t **out)
{
    if (!pcb_tbl || !out)
        return -EINVAL;
    struct cndp_tcb_tbl *t = calloc(1, sizeof(*t));
    if (!t)
        return -ENOMEM;
    t->cap = pcb_tbl->max;
    t->img = calloc((size_t)t->cap * TCB_WORDS, sizeof(uint32_t));
    t->seen = calloc(t->cap, sizeof(uint32_t));
    if (!t->img || !t->seen || pthread_mutex_init(&t->lock, NULL)) {
        free(t->seen);
        free(t->img);
        free(t);
        return -ENOMEM;
    }
    t->pcb = pcb_tbl;
    t->gen = 1;
    t->d_lo = 0;
    t->d_hi = t->cap;
    *out = t;
    return 0;
}

void cndp_tcb_tbl_destroy(cndp_tcb_tbl_t *t)
{
    if (!t)
        return;
    if (t->dev && t->dev_release)
        t->dev_release(t->dev);
    free(t->kimg);
    pthread_mutex_destroy(&t->lock);
    free(t->seen);
    free(t->img);
    free(t);
}

/* call with the lock held: entry idx of the image changed */
static void touched(struct cndp_tcb_tbl *t, uint32_t idx)
{
    if (idx < t->d_lo)
        t->d_lo = idx;
    if (idx + 1u > t->d_hi)
        t->d_hi = idx + 1u;
    t->gen++;
}

uint32_t tcb_reconcile(struct cndp_tcb_tbl *t)
{
    struct cndp_pcb_tbl *p = t->pcb;
    pthread_mutex_lock(&p->lock);
    const uint32_t count = p->count;
    if (t->pcb_gen != p->gen) {
        for (uint32_t i = 0; i < count; i++) {
            uint32_t *e = t->img + (size_t)i * TCB_WORDS;
            if (p->closed[i] && (e[10] & TCB_PRESENT)) { /* cnet_pcb_free's memset took pcb->tcb with it */
                memset(e, 0, TCB_WORDS * sizeof(uint32_t));
                touched(t, i);
            }
        }
        t->pcb_gen = p->gen;
    }
    pthread_mutex_unlock(&p->lock);
    return count;
}

/* call with t->lock held: 0, -EINVAL (outside the vector) or -ENOENT (deleted) */
static int slot_ok(struct cndp_tcb_tbl *t, uint32_t idx)
{
    if (idx >= tcb_reconcile(t))
        return -EINVAL;
    pthread_mutex_lock(&t->pcb->lock);
    const int closed = t->pcb->closed[idx];
    pthread_mutex_unlock(&t->pcb->lock);
    return closed ? -ENOENT : 0;
}

int cndp_tcb_set(cndp_tcb_tbl_t *t, uint32_t idx, const struct cndp_tcb *tcb)
{
    if (!t || !tcb || tcb->state > CNDP_TCPS_TIME_WAIT)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = slot_ok(t, idx);
    if (!r) {
        uint32_t *e = t->img + (size_t)idx * TCB_WORDS;
        e[0] = tcb->rcv_nxt;
        e[1] = tcb->snd_una;
        e[2] = tcb->snd_nxt;
        e[3] = tcb->snd_max;
        e[4] = tcb->snd_wnd;
        e[5] = tcb->snd_cwnd;
        e[6] = tcb->ts_recent;
        e[7] = tcb->last_ack_sent;
        e[8] = tcb->rcv_space;
        e[9] = tcb->max_mss | (uint32_t)tcb->state << 16 | (uint32_t)tcb->snd_scale << 24;
        if (!(e[10] & TCB_PRESENT))
            e[11] = 0; /* a fresh TCB: no transmit attributes; an existing one keeps them */
        e[10] = (tcb->flags & CNDP_TCB_REASS_EMPTY) | TCB_PRESENT;
        touched(t, idx);
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_tcb_clear(cndp_tcb_tbl_t *t, uint32_t idx)
{
    if (!t)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = idx >= tcb_reconcile(t) ? -EINVAL : 0;
    if (!r) {
        uint32_t *e = t->img + (size_t)idx * TCB_WORDS;
        if (!(e[10] & TCB_PRESENT))
            r = -ENOENT;
        else {
            memset(e, 0, TCB_WORDS * sizeof(uint32_t));
            touched(t, idx);
        }
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_tcb_get(cndp_tcb_tbl_t *t, uint32_t idx, struct cndp_tcb *out)
{
    if (!t || !out)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = idx >= tcb_reconcile(t) ? -EINVAL : 0;
    if (!r) {
        const uint32_t *e = t->img + (size_t)idx * TCB_WORDS;
        if (!(e[10] & TCB_PRESENT))
            r = -ENOENT;
        else {
            memset(out, 0, sizeof(*out));
            out->rcv_nxt = e[0];
            out->snd_una = e[1];
            out->snd_nxt = e[2];
            out->snd_max = e[3];
            out->snd_wnd = e[4];
            out->snd_cwnd = e[5];
            out->ts_recent = e[6];
            out->last_ack_sent = e[7];
            out->rcv_space = e[8];
            out->max_mss = (uint16_t)e[9];
            out->state = (uint8_t)(e[9] >> 16);
            out->snd_scale = (uint8_t)(e[9] >> 24);
            out->flags = (uint8_t)(e[10] & CNDP_TCB_REASS_EMPTY);
        }
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

/* ---- transmit attributes (include/cndp_tcpout.h): word 11 of the entry ------ */
#define TCB_TX_FLAGS (CNDP_TCBF_REQ_SCALE | CNDP_TCBF_RCVD_SCALE | CNDP_TCBF_REQ_TSTAMP | CNDP_TCBF_RCVD_TSTAMP)

int cndp_tcb_tx_set(cndp_tcb_tbl_t *t, uint32_t idx, const struct cndp_tcb_tx *a)
{
    if (!t || !a)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = slot_ok(t, idx);
    if (!r) {
        uint32_t *e = t->img + (size_t)idx * TCB_WORDS;
        if (!(e[10] & TCB_PRESENT))
            r = -ENOENT;
        else {
            e[11] = (a->tflags & TCB_TX_FLAGS) | (uint32_t)a->req_recv_scale << 8 | (uint32_t)a->rcv_scale << 16;
            touched(t, idx);
        }
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

int cndp_tcb_tx_get(cndp_tcb_tbl_t *t, uint32_t idx, struct cndp_tcb_tx *a)
{
    if (!t || !a)
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    int r = idx >= tcb_reconcile(t) ? -EINVAL : 0;
    if (!r) {
        const uint32_t *e = t->img + (size_t)idx * TCB_WORDS;
        if (!(e[10] & TCB_PRESENT))
            r = -ENOENT;
        else {
            a->tflags = (uint8_t)e[11];
            a->req_recv_scale = (uint8_t)(e[11] >> 8);
            a->rcv_scale = (uint8_t)(e[11] >> 16);
            a->rsvd = 0;
        }
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

/* the option words at byte offset o of the slab, bytes at or past len as zero */
static void rd_opt_words(const uint8_t *s, uint64_t len, uint64_t o, uint32_t *w)
{
    uint8_t b[TCB_OPT_WORDS * 4u];
    if (o < len && len - o >= sizeof(b))
        memcpy(b, s + o, sizeof(b));
    else {
        memset(b, 0, sizeof(b));
        if (o < len)
            memcpy(b, s + o, (size_t)(len - o));
    }
    for (uint32_t k = 0; k < TCB_OPT_WORDS; k++)
        w[k] = b[4u * k] | (uint32_t)b[4u * k + 1u] << 8 | (uint32_t)b[4u * k + 2u] << 16 |
               (uint32_t)b[4u * k + 3u] << 24;
}

int cndp_tcp_segment_host(cndp_tcb_tbl_t *t, uint32_t now, const struct cndp_batch *b,
                          const struct cndp_tcpseg_io *io)
{
    if (!t || !b || !io)
        return -EINVAL;
    if (b->n && (!b->slab || !b->rxmeta || !io->pcb || !io->seg || !io->opt || !io->verdict ||
                 (!io->sel && !io->l4edge) || (b->slab_len >> 63)))
        return -EINVAL;
    pthread_mutex_lock(&t->lock);
    (void)tcb_reconcile(t);
    const uint8_t *slab = b->slab;
    const uint32_t n = b->n;
    /* the first taken frame of each PCB: frames are walked in batch order */
    uint8_t *seen = calloc(t->cap, 1);
    if (!seen) {
        pthread_mutex_unlock(&t->lock);
        return -ENOMEM;
    }
    static const uint32_t none[TCB_OPT_WORDS];
    for (uint32_t i = 0; i < n; i++) {
        uint32_t o[4] = {0, 0, 0, 0}, v = CNDP_TCPSEG_NONE;
        const uint32_t p = io->pcb[i];
        const int taken = (io->sel ? io->sel[i] != 0 : io->l4edge[i] == EDGE_SEG) && p < t->cap;
        if (taken) {
            const struct cndp_tcp_seg *sg = &io->seg[i];
            uint32_t w[TCB_OPT_WORDS];
            const uint32_t *wp = none;
            if (sg->offset > TCB_HDR_LEN) {
                const uint32_t rx = b->rxmeta[i];
                const uint64_t m = (b->offsets ? b->offsets[i] : (uint64_t)i * b->stride) + b->data_off +
                                   CNDP_RXMETA_L2(rx);
                rd_opt_words(slab, b->slab_len, m + CNDP_RXMETA_L3(rx) + TCB_HDR_LEN, w);
                wp = w;
            }
            v = tcb_segment(t->img + (size_t)p * TCB_WORDS, sg->seq, sg->ack, sg->wnd, sg->len, sg->flags,
                            sg->offset, wp, now, o);
            if (!seen[p]) {
                seen[p] = 1;
                v |= CNDP_TCPSEG_FIRST;
            }
        }
        io->opt[i].ts_val = o[0];
        io->opt[i].ts_ecr = o[1];
        io->opt[i].wnd = o[2];
        io->opt[i].mss = (uint16_t)o[3];
        io->opt[i].sflags = (uint16_t)(o[3] >> 16);
        io->verdict[i] = (uint8_t)v;
        if (io->stats)
            io->stats[v & CNDP_TCPSEG_VERDICT]++;
    }
    free(seen);
    pthread_mutex_unlock(&t->lock);
    return 0;
}

/* ---- cndp_mqtcb.h: tcp_input, cnet_tcp_input's opening, tcp_do_options and the
 * prediction tests over mbufs on the host ------------------------------------- */

int cndp_tcp_segment_node_host(cndp_pcb_tbl_t *tbl, cndp_tcb_tbl_t *t, uint32_t now, void *const *mbufs, uint32_t n,
                               uint16_t *edges, struct cndp_tcp_seg *segs, struct cndp_tcp_opt *opts,
                               uint8_t *verdicts, const void *readable_end, uint32_t stage_max,
                               void *(*metadata)(const void *m))
{
    if (!tbl || !t || t->pcb != tbl || n > 256u || (n && (!mbufs || !edges)))
        return -EINVAL;
    struct cndp_tcp_seg sg[256];
    uint32_t hits[256], optw[256u * PCB_TCP_OPT_WORDS];
    pthread_mutex_lock(&t->lock);
    (void)tcb_reconcile(t);
    pthread_mutex_lock(&tbl->lock);
    const int r = pcb_tcp_node_walk(tbl, mbufs, n, edges, sg, hits, optw, readable_end, stage_max, metadata);
    pthread_mutex_unlock(&tbl->lock);
    /* FIRST: the judged mbufs are walked in batch order, and a PCB's stamp says whether this call
     * has met it; stamps of earlier calls never equal this one's, so nothing is cleared per call */
    if (++t->seen_call == 0u) {
        memset(t->seen, 0, (size_t)t->cap * sizeof(uint32_t));
        t->seen_call = 1u;
    }
    const uint32_t call = t->seen_call;
    for (uint32_t i = 0; !r && i < n; i++) {
        uint32_t o[4] = {0, 0, 0, 0}, v = CNDP_TCPSEG_NONE;
        const uint32_t p = hits[i];
        if (tcb_mq_judged(edges[i], &sg[i]) && p < t->cap) {
            v = tcb_segment(t->img + (size_t)p * TCB_WORDS, sg[i].seq, sg[i].ack, sg[i].wnd, sg[i].len, sg[i].flags,
                            sg[i].offset, optw + (size_t)i * PCB_TCP_OPT_WORDS, now, o);
            if (t->seen[p] != call) {
                t->seen[p] = call;
                v |= CNDP_TCPSEG_FIRST;
            }
        }
        if (segs)
            segs[i] = sg[i];
        if (opts) {
            opts[i].ts_val = o[0];
            opts[i].ts_ecr = o[1];
            opts[i].wnd = o[2];
            opts[i].mss = (uint16_t)o[3];
            opts[i].sflags = (uint16_t)(o[3] >> 16);
        }
        if (verdicts)
            verdicts[i] = (uint8_t)v;
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

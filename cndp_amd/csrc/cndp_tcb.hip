// cndp_tcb.hip -- tcp_do_options and the header-prediction triage on MI355X
// (include/cndp_tcb.h), for the frames cndp_gpu_tcp_input left on the SEGMENT edge.
//
// Two kernels per call, no host round trip between them:
//   tcpseg_first_kernel  one frame per lane: atomicMin of the frame index into a
//                        per-PCB word (4096 of them, reset by a memset on the
//                        same stream).  A minimum does not depend on the order the
//                        lanes arrive in, so the result is the same on every run.
//   tcpseg_kernel        one frame per lane.  The PCB's 48-byte TCB entry is
//                        gathered as three 16-byte loads.  At 4096 entries the
//                        image is 192 KiB: more than the CU's 160 KiB of LDS, so it
//                        is not staged; the kernel gathers it from L2, where it
//                        stays resident (4 MiB per XCD) after the first touch.
//                        A segment with options reads them -- 4 dwords when the
//                        header is 32 bytes or less (the timestamp-only header), 11
//                        otherwise: up to 40 option bytes and the byte at opt_end,
//                        the parser's one read past the header -- into registers
//                        and walks them there: a byte position is turned into a
//                        chain of selects over the words (tcb_internal.h), no
//                        indexed register file, no scratch.  The rule itself is
//                        tcb_segment(), the function the host twin runs.  `opt`
//                        leaves as one 16-byte store.  Counters: a ballot per
//                        verdict value per wave, an LDS add per wave, one global
//                        add per block and counter.
// Every frame read is bounded by slab_len; no load leaves the slab.
//
// The image's device mirror is one buffer guarded by an event.  Every reader --
// cndp_gpu_tcp_segment here, the mbuf queue's CNDP_MQ_TCP_SEGMENT kernels in
// cndp_gpu.hip -- brackets its launches with tcb_dev_begin / tcb_dev_end
// (tcb_internal.h).  The queue hands tcb_dev_begin a pinned snapshot buffer, so
// a TCB changed between two batches costs its launch a copy and no wait.
//
// The byte readers are those of cndp_tcp.hip (and cndp_l4.hip), kept as a copy so
// those translation units stay as they are.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tcb_internal.h"

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            fprintf(stderr, "cndp_tcb: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),   \
                    __FILE__, __LINE__);                                                         \
            return e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? -ENODEV : -EIO;       \
        }                                                                                        \
    } while (0)

#define SEG_BLOCK 256u
#define SEG_BLOCKS_PER_CU 8u
#define EDGE_SEG CNDP_L4_EDGE(CNDP_L4_NODE_TCP_INPUT, CNDP_TCP_INPUT_SEGMENT)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct SegArgs {
    const uint8_t *slab;
    uint64_t slab_len;
    uint64_t stride;
    const uint64_t *offsets;
    uint32_t data_off;
    uint32_t n;
    const uint32_t *rxmeta;
    const uint8_t *sel;
    const uint8_t *l4edge;
    const uint32_t *pcb;
    const u32x4 *seg;
    u32x4 *opt;
    uint8_t *verdict;
    unsigned long long *stats;
    const u32x4 *tcb; // device mirror of the image: 3 x 16 bytes per PCB index
    uint32_t *first;  // per PCB index: the lowest taken frame index of this batch
    uint32_t cap;     // entries of tcb and first
    uint32_t now;
};

// N little-endian dwords at byte offset o of the slab, bytes at or past len read
// as zero.  Away from the slab's edges: aligned dword loads plus a byte shift.
template <int N>
__device__ __forceinline__ void rd_words(const uint8_t *s, uint64_t len, uint64_t o, uint32_t (&w)[N])
{
    if (o >= 4 && o < len && len - o >= 4u * N + 4u) {
        uintptr_t p = (uintptr_t)s + o;
        uint32_t sh = (uint32_t)(p & 3u);
        const uint32_t *a = (const uint32_t *)(p - sh); // a >= s + 1, a + N + 1 dwords end <= s + len
        uint32_t d[N + 1];
#pragma unroll
        for (int k = 0; k < N; k++)
            d[k] = a[k];
        d[N] = sh ? a[N] : 0u;
#pragma unroll
        for (int k = 0; k < N; k++)
            w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) {
            uint32_t v = 0;
            for (uint32_t j = 0; j < 4; j++) {
                uint64_t x = o + 4u * k + j;
                if (x >= o && x < len) // x >= o: no wrap for an offset near 2^64
                    v |= (uint32_t)s[x] << (8 * j);
            }
            w[k] = v;
        }
    }
}

__device__ __forceinline__ bool seg_taken(const SegArgs &a, uint32_t i, uint32_t &p)
{
    p = a.pcb[i];
    return (a.sel ? a.sel[i] != 0 : a.l4edge[i] == EDGE_SEG) && p < a.cap;
}

__global__ __launch_bounds__(SEG_BLOCK) void tcpseg_first_kernel(SegArgs a)
{
    const uint64_t step = (uint64_t)gridDim.x * SEG_BLOCK;
    for (uint64_t i64 = (uint64_t)blockIdx.x * SEG_BLOCK + threadIdx.x; i64 < a.n; i64 += step) {
        const uint32_t i = (uint32_t)i64;
        uint32_t p;
        if (seg_taken(a, i, p)) // p < cap
            atomicMin(&a.first[p], i);
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void tcpseg_kernel(SegArgs a)
{
    __shared__ uint32_t s_stat[CNDP_TCPSEG_NSTATS];
    if (threadIdx.x < CNDP_TCPSEG_NSTATS)
        s_stat[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * SEG_BLOCK;
    for (uint64_t base = (uint64_t)blockIdx.x * SEG_BLOCK; base < a.n; base += step) {
        const uint64_t i64 = base + threadIdx.x;
        const bool live = i64 < a.n;
        const uint32_t i = (uint32_t)i64;
        uint32_t p = 0;
        const bool taken = live && seg_taken(a, i, p);
        uint32_t o[4] = {0u, 0u, 0u, 0u}, v = CNDP_TCPSEG_NONE;
        if (taken) {
            const u32x4 sg = a.seg[i];
            const u32x4 *tp = a.tcb + (size_t)p * 3u; // p < cap
            const u32x4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
            const uint32_t fi = a.first[p]; // with the gather, not behind the parse
            const uint32_t e[TCB_WORDS] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
            const uint32_t offset = sg.w >> 24;
            uint32_t w[TCB_OPT_WORDS];
#pragma unroll
            for (uint32_t k = 0; k < TCB_OPT_WORDS; k++)
                w[k] = 0u;
            if (offset > TCB_HDR_LEN) { // whatever the TCB says: the frame read does not wait for the gather
                const uint32_t rx = a.rxmeta[i];
                const uint64_t at = (a.offsets ? a.offsets[i] : (uint64_t)i * a.stride) + a.data_off +
                                    CNDP_RXMETA_L2(rx) + CNDP_RXMETA_L3(rx) + TCB_HDR_LEN;
                if (offset <= 32u) { // up to 12 option bytes and the byte at opt_end
                    uint32_t q[4];
                    rd_words<4>(a.slab, a.slab_len, at, q);
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        w[k] = q[k];
                } else
                    rd_words<(int)TCB_OPT_WORDS>(a.slab, a.slab_len, at, w);
            }
            v = tcb_segment(e, sg.x, sg.y, sg.z & 0xffffu, sg.w & 0xffffu, (sg.w >> 16) & 0xffu, offset, w, a.now, o);
            if (fi == i)
                v |= CNDP_TCPSEG_FIRST;
        }
        if (live) {
            a.opt[i] = u32x4{o[0], o[1], o[2], o[3]};
            a.verdict[i] = (uint8_t)v;
        }
#pragma unroll
        for (uint32_t k = 0; k < CNDP_TCPSEG_NSTATS; k++) {
            const unsigned long long m = __ballot(live && (v & CNDP_TCPSEG_VERDICT) == k);
            if (m && lane == 0)
                atomicAdd(&s_stat[k], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    if (a.stats && threadIdx.x < CNDP_TCPSEG_NSTATS && s_stat[threadIdx.x])
        atomicAdd(&a.stats[threadIdx.x], (unsigned long long)s_stat[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// host side: the image's device mirror
// ---------------------------------------------------------------------------
struct TcbDev {
    int dev;
    int cus;
    uint32_t *img;   // cap * TCB_WORDS, allocated on the first call
    uint32_t *first; // cap words
    uint64_t gen;    // table generation mirrored (0 = none)
    hipEvent_t ev;   // end of the last call's kernels
    hipStream_t last;
    int have_last;
};

static void tcb_dev_release(void *p)
{
    TcbDev *d = (TcbDev *)p;
    if (hipSetDevice(d->dev) == hipSuccess) {
        (void)hipDeviceSynchronize();
        if (d->img)
            (void)hipFree(d->img);
        if (d->first)
            (void)hipFree(d->first);
        if (d->ev)
            (void)hipEventDestroy(d->ev);
    }
    free(d);
}

static int tcb_dev_init(TcbDev *d, uint32_t cap)
{
    HIP_TRY(hipDeviceGetAttribute(&d->cus, hipDeviceAttributeMultiprocessorCount, d->dev));
    HIP_TRY(hipMalloc((void **)&d->first, (size_t)cap * sizeof(uint32_t)));
    HIP_TRY(hipEventCreateWithFlags(&d->ev, hipEventDisableTiming));
    return 0;
}

static int tcb_dev_get(struct cndp_tcb_tbl *t, int dev, TcbDev **out)
{
    TcbDev *d = (TcbDev *)t->dev;
    if (d && d->dev != dev)
        return -EINVAL; // one table, one device
    if (!d) {
        d = (TcbDev *)calloc(1, sizeof(*d));
        if (!d)
            return -ENOMEM;
        d->dev = dev;
        int r = tcb_dev_init(d, t->cap);
        if (r) {
            tcb_dev_release(d);
            return r;
        }
        t->dev = d;
        t->dev_release = tcb_dev_release;
    }
    *out = d;
    return 0;
}

// staging: NULL, or the pinned snapshot buffer of tcb_dev_begin (tcb_internal.h)
static int tcb_mirror(TcbDev *d, struct cndp_tcb_tbl *t, hipStream_t s, void *staging)
{
    (void)tcb_reconcile(t);
    if (d->gen == t->gen)
        return 0;
    uint32_t lo = t->d_lo, hi = t->d_hi;
    bool wait = staging == NULL;
    if (!d->img) {
        HIP_TRY(hipMalloc((void **)&d->img, (size_t)t->cap * TCB_WORDS * 4u));
        lo = 0;
        hi = t->cap;
        wait = true; // the first copy of a table comes from the host image itself
    }
    if (hi > lo) {
        const size_t at = (size_t)lo * TCB_WORDS, bytes = (size_t)(hi - lo) * TCB_WORDS * 4u;
        const uint32_t *src = t->img + at;
        if (!wait) { // the entries as they are now, where later changes do not reach them
            memcpy((uint32_t *)staging + at, src, bytes);
            src = (const uint32_t *)staging + at;
        }
        HIP_TRY(hipMemcpyAsync(d->img + at, src, bytes, hipMemcpyHostToDevice, s));
        if (wait)
            HIP_TRY(hipStreamSynchronize(s)); // the host table may change after we return
    }
    t->d_lo = UINT32_MAX;
    t->d_hi = 0;
    d->gen = t->gen;
    return 0;
}

// tcb_dev_begin under t->lock: the device, the wait for a reader on another
// stream, the mirror brought up to date
static int tcb_begin_locked(struct cndp_tcb_tbl *t, int dev, hipStream_t s, void *staging, TcbDev **out)
{
    HIP_TRY(hipSetDevice(dev));
    TcbDev *d = NULL;
    int r = tcb_dev_get(t, dev, &d);
    if (r)
        return r;
    if (d->have_last && d->last != s)
        HIP_TRY(hipStreamWaitEvent(s, d->ev, 0));
    if ((r = tcb_mirror(d, t, s, staging)))
        return r;
    *out = d;
    return 0;
}

// tcb_dev_end under t->lock: the reader's end recorded
static int tcb_end_locked(struct cndp_tcb_tbl *t, hipStream_t s, int launched)
{
    TcbDev *d = (TcbDev *)t->dev;
    if (!launched || !d)
        return 0;
    HIP_TRY(hipEventRecord(d->ev, s));
    d->last = s;
    d->have_last = 1;
    return 0;
}

extern "C" int tcb_dev_begin(struct cndp_tcb_tbl *t, int dev, void *stream, void *staging, const uint32_t **img)
{
    pthread_mutex_lock(&t->lock);
    TcbDev *d = NULL;
    const int r = tcb_begin_locked(t, dev, (hipStream_t)stream, staging, &d);
    if (r) {
        pthread_mutex_unlock(&t->lock);
        return r;
    }
    *img = d->img;
    return 0;
}

extern "C" int tcb_dev_end(struct cndp_tcb_tbl *t, void *stream, int launched)
{
    const int r = tcb_end_locked(t, (hipStream_t)stream, launched);
    pthread_mutex_unlock(&t->lock);
    return r;
}

extern "C" int tcb_dev_check(struct cndp_tcb_tbl *t, int dev)
{
    pthread_mutex_lock(&t->lock);
    const TcbDev *d = (const TcbDev *)t->dev;
    const int r = d && d->dev != dev ? -EINVAL : 0; // one table, one device
    pthread_mutex_unlock(&t->lock);
    return r;
}

static int tcb_run(TcbDev *d, struct cndp_tcb_tbl *t, const struct cndp_batch *b, const struct cndp_tcpseg_io *io,
                   uint32_t now, hipStream_t s)
{
    SegArgs a;
    a.slab = (const uint8_t *)b->slab;
    a.slab_len = b->slab_len;
    a.stride = b->stride;
    a.offsets = b->offsets;
    a.data_off = b->data_off;
    a.n = b->n;
    a.rxmeta = b->rxmeta;
    a.sel = io->sel;
    a.l4edge = io->l4edge;
    a.pcb = io->pcb;
    a.seg = (const u32x4 *)io->seg;
    a.opt = (u32x4 *)io->opt;
    a.verdict = io->verdict;
    a.stats = (unsigned long long *)io->stats;
    a.tcb = (const u32x4 *)d->img;
    a.first = d->first;
    a.cap = t->cap;
    a.now = now;

    const uint64_t want = ((uint64_t)b->n + SEG_BLOCK - 1u) / SEG_BLOCK;
    const uint64_t cap = (uint64_t)d->cus * SEG_BLOCKS_PER_CU;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    HIP_TRY(hipMemsetAsync(d->first, 0xff, (size_t)t->cap * sizeof(uint32_t), s));
    hipLaunchKernelGGL(tcpseg_first_kernel, dim3(grid), dim3(SEG_BLOCK), 0, s, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tcpseg_kernel, dim3(grid), dim3(SEG_BLOCK), 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int cndp_gpu_tcp_segment(cndp_gpu_ctx_t *ctx, cndp_tcb_tbl_t *t, const struct cndp_batch *b,
                                    const struct cndp_tcpseg_io *io, uint32_t now, void *stream)
{
    if (!ctx || !t || !b || !io)
        return -EINVAL;
    if (b->n && (!b->slab || !b->rxmeta || !io->pcb || !io->seg || !io->opt || !io->verdict ||
                 (!io->sel && !io->l4edge) || ((uintptr_t)io->seg & 15u) || ((uintptr_t)io->opt & 15u) ||
                 (b->slab_len >> 63)))
        return -EINVAL;
    const int dev = cndp_gpu_device(ctx);
    pthread_mutex_lock(&t->lock);
    TcbDev *d = NULL;
    int r = tcb_begin_locked(t, dev, (hipStream_t)stream, NULL, &d);
    if (!r) {
        if (b->n)
            r = tcb_run(d, t, b, io, now, (hipStream_t)stream);
        const int e = tcb_end_locked(t, (hipStream_t)stream, b->n && !r);
        r = r ? r : e;
    }
    pthread_mutex_unlock(&t->lock);
    return r;
}

// cndp_cfwd.hip -- cndpfwd's fwd and l3fwd modes on MI355X (include/cndp_cfwd.h):
// the TTL and checksum step, the 8-byte DIR-24-8 lookup, the destination port
// and MAC_REWRITE / MAC_SWAP of _l3fwd_test and _fwd_test, one frame per lane.
//
// One kernel per call, instantiated per mode:
//   cfwd_kernel<MODE>  A frame that starts on a 16-byte boundary and has its
//                   first 36 bytes inside the slab (packed 64-byte slots, the
//                   UMEM stride at +256) is read as two 16-byte loads and a
//                   dword (FWD: one 16-byte load).  L3FWD stores bytes 0-31 back
//                   as two 16-byte stores, the unchanged bytes among them with
//                   the values just read; FWD stores bytes 0-11 as three dwords.
//                   Any other frame (IMIX offsets, the slab's last frames) takes
//                   bounded byte loads and stores of the changed bytes alone,
//                   with the same results.
//                   The rule itself is cfwd_rule of cfwd_internal.h, the text the
//                   host runs: the 8-byte tbl24[ip >> 8] gather is issued first,
//                   the TTL / checksum arithmetic runs under it, and only an
//                   entry with the extension bit costs a second gather (tbl8).
//                   The table pointers are restrict kernel arguments so that the
//                   frame stores do not stand in the gathers' way.
//                   Outputs leave as coalesced stores of one element per lane.
//                   Counters: a ballot per counter per wave, an LDS add per wave,
//                   one global add per block and counter.  No atomic decides an
//                   output value.
// Every frame access is bounded by slab_len; no load or store leaves the slab.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "cfwd_internal.h"
#include "fib_internal.h"

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            fprintf(stderr, "cndp_cfwd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),  \
                    __FILE__, __LINE__);                                                         \
            return e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? -ENODEV : -EIO;       \
        }                                                                                        \
    } while (0)

#define CFWD_BLOCK 256u
#define CFWD_BLOCKS_PER_CU 8u
#define CFWD_DEVS_MAX 64

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct CfwdArgs {
    uint8_t *slab;
    uint64_t slab_len;
    uint64_t stride;
    const uint64_t *offsets;
    uint32_t data_off;
    uint32_t n;
    const uint8_t *sel;
    uint64_t *nh;
    uint16_t *tx_lport;
    uint8_t *echoed;
    uint16_t *bin_of;
    unsigned long long *stats;
    uint64_t m0, m1, m2, m3; // lport_mask
    uint32_t in_lport;
    uint32_t n_bins;
};

// byte k of the frame at slab offset at, zero at or past len
__device__ __forceinline__ uint32_t rd_byte(const uint8_t *s, uint64_t len, uint64_t at, uint32_t k)
{
    const uint64_t x = at + k;
    return x >= at && x < len ? s[x] : 0u; // x >= at: no wrap for an offset near 2^64
}

__device__ __forceinline__ uint32_t rd_le32(const uint8_t *s, uint64_t len, uint64_t at, uint32_t k)
{
    return rd_byte(s, len, at, k) | rd_byte(s, len, at, k + 1u) << 8 | rd_byte(s, len, at, k + 2u) << 16 |
           rd_byte(s, len, at, k + 3u) << 24;
}

// the low CNT bytes of v to frame bytes k ..., those inside the slab
template <uint32_t CNT>
__device__ __forceinline__ void st_bytes(uint8_t *s, uint64_t len, uint64_t at, uint32_t k, uint32_t v)
{
#pragma unroll
    for (uint32_t j = 0; j < CNT; j++) {
        const uint64_t x = at + k + j;
        if (x >= at && x < len)
            s[x] = (uint8_t)(v >> (8u * j));
    }
}

template <uint32_t MODE>
__global__ __launch_bounds__(CFWD_BLOCK) void cfwd_kernel(CfwdArgs a, const uint64_t *__restrict__ t24,
                                                          const uint64_t *__restrict__ t8)
{
    __shared__ uint32_t s_stat[CNDP_CFWD_NSTATS];
    if (threadIdx.x < CNDP_CFWD_NSTATS)
        s_stat[threadIdx.x] = 0;
    __syncthreads();
    constexpr bool l3 = MODE == CNDP_CFWD_L3FWD;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * CFWD_BLOCK;
    for (uint64_t base = (uint64_t)blockIdx.x * CFWD_BLOCK; base < a.n; base += step) {
        const uint64_t i64 = base + threadIdx.x;
        const bool live = i64 < a.n;
        const uint32_t i = (uint32_t)i64;
        const bool taken = live && (!a.sel || a.sel[i] != 0);
        uint64_t nh = 0;
        uint32_t tx = CNDP_CFWD_LPORT_NONE, echo = 0;
        if (taken) {
            const uint64_t at = (a.offsets ? a.offsets[i] : (uint64_t)i * a.stride) + a.data_off;
            const uintptr_t p = (uintptr_t)a.slab + at;
            // bytes at .. at + 35 lie inside the slab and the frame is 16-byte aligned
            const bool wide = at < a.slab_len && a.slab_len - at >= 36u && !(p & 15u);
            cfwd_frame f;
            cfwd_edit e;
            u32x4 v = {0, 0, 0, 0}, w = {0, 0, 0, 0};
            if (wide) {
                v = *(const u32x4 *)p;
                f.d0 = v.x, f.d1 = v.y, f.d2 = v.z;
                if (l3) {
                    w = *(const u32x4 *)(p + 16u);
                    const uint32_t d8 = *(const uint32_t *)(p + 32u);
                    f.ttl = (w.y >> 16) & 0xffu;                    // byte 22
                    f.ck = w.z & 0xffffu;                           // bytes 24, 25
                    f.dst = __builtin_amdgcn_alignbyte(d8, w.w, 2); // bytes 30..33
                } else {
                    f.ttl = f.ck = f.dst = 0;
                }
            } else {
                f.d0 = rd_le32(a.slab, a.slab_len, at, 0);
                f.d1 = rd_le32(a.slab, a.slab_len, at, 4);
                f.d2 = rd_le32(a.slab, a.slab_len, at, 8);
                if (l3) {
                    f.ttl = rd_byte(a.slab, a.slab_len, at, 22);
                    f.ck = rd_byte(a.slab, a.slab_len, at, 24) | rd_byte(a.slab, a.slab_len, at, 25) << 8;
                    f.dst = rd_le32(a.slab, a.slab_len, at, 30);
                } else {
                    f.ttl = f.ck = f.dst = 0;
                }
            }
            cfwd_rule(MODE, &f, t24, t8, a.m0, a.m1, a.m2, a.m3, a.in_lport, &e);
            const bool all12 = !l3 || e.echo; // MAC_SWAP: bytes 0-11; MAC_REWRITE: bytes 0-5
            if (wide && l3) {
                // bytes 0-31 go back as the two 16-byte pieces they came in, the bytes that do not
                // change with the values just read: four narrow stores of the changed bytes alone
                // (0-3, 4-5, 22, 24-25) measured 0.68 ms against 0.55 ms on the C3 batch
                v.x = e.d0, v.y = e.d1, v.z = e.d2;
                *(u32x4 *)p = v;
                w.y = (w.y & 0xFF00FFFFu) | e.ttl << 16;
                w.z = (w.z & 0xFFFF0000u) | e.ck;
                *(u32x4 *)(p + 16u) = w;
            } else if (wide) {
                uint32_t *q = (uint32_t *)p; // MAC_SWAP as k_mac_swap stores it (one 16-byte store measured the same)
                q[0] = e.d0;
                q[1] = e.d1;
                q[2] = e.d2;
            } else {
                st_bytes<4>(a.slab, a.slab_len, at, 0, e.d0);
                if (all12) {
                    st_bytes<4>(a.slab, a.slab_len, at, 4, e.d1);
                    st_bytes<4>(a.slab, a.slab_len, at, 8, e.d2);
                } else {
                    st_bytes<2>(a.slab, a.slab_len, at, 4, e.d1);
                }
                if (l3) {
                    st_bytes<1>(a.slab, a.slab_len, at, 22, e.ttl);
                    st_bytes<2>(a.slab, a.slab_len, at, 24, e.ck);
                }
            }
            nh = e.nh;
            tx = e.tx;
            echo = e.echo;
        }
        if (live) {
            if (a.nh)
                a.nh[i] = nh;
            a.tx_lport[i] = (uint16_t)tx;
            if (a.echoed)
                a.echoed[i] = (uint8_t)echo;
            if (a.bin_of)
                a.bin_of[i] = (uint16_t)(taken ? tx : a.n_bins);
        }
        const unsigned long long mf = __ballot(taken && !echo), me = __ballot(taken && echo);
        if (lane == 0) {
            if (mf)
                atomicAdd(&s_stat[CNDP_CFWD_STAT_FORWARD], (uint32_t)__popcll(mf));
            if (me)
                atomicAdd(&s_stat[CNDP_CFWD_STAT_ECHO], (uint32_t)__popcll(me));
        }
    }
    __syncthreads();
    if (a.stats && threadIdx.x < CNDP_CFWD_NSTATS && s_stat[threadIdx.x])
        atomicAdd(&a.stats[threadIdx.x], (unsigned long long)s_stat[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// Per device: the CU count and the end of the last call's kernel, so that a call
// on another stream starts after it.  Calls are serialised by one lock.
struct CfwdDev {
    int ready;
    int cus;
    hipEvent_t ev;
    hipStream_t last;
    int have_last;
};
static CfwdDev g_dev[CFWD_DEVS_MAX];
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;

static int cfwd_dev_get(int dev, CfwdDev **out)
{
    if (dev < 0 || dev >= CFWD_DEVS_MAX)
        return -EINVAL;
    CfwdDev *d = &g_dev[dev];
    if (!d->ready) {
        HIP_TRY(hipDeviceGetAttribute(&d->cus, hipDeviceAttributeMultiprocessorCount, dev));
        HIP_TRY(hipEventCreateWithFlags(&d->ev, hipEventDisableTiming));
        d->ready = 1;
    }
    *out = d;
    return 0;
}

// Sync the FIB's mirror on `s` and take a view of its buffers: read under dev_lock
// with `views` held until the launch is enqueued, so a sync on another thread
// that replaces a buffer retires it instead of freeing it (fib_internal.h).
static int fib_acquire(struct cndp_tbl *t, hipStream_t s, const uint64_t **t24, const uint64_t **t8)
{
    int r = cndp_tbl_dev_sync(t, s);
    if (r)
        return r;
    pthread_mutex_lock(&t->dev_lock);
    *t24 = (const uint64_t *)t->dev_tbl24;
    *t8 = (const uint64_t *)t->dev_tbl8;
    r = *t24 && *t8 ? 0 : -EIO;
    if (!r)
        __atomic_add_fetch(&t->views, 1u, __ATOMIC_RELAXED);
    pthread_mutex_unlock(&t->dev_lock);
    return r;
}
static inline void fib_release(struct cndp_tbl *t) { __atomic_sub_fetch(&t->views, 1u, __ATOMIC_RELEASE); }

static int cfwd_run(CfwdDev *d, struct cne_fib *fib, const struct cndp_batch *b, uint32_t mode,
                    const struct cndp_cfwd_io *io, hipStream_t s)
{
    if (d->have_last && d->last != s)
        HIP_TRY(hipStreamWaitEvent(s, d->ev, 0));
    const bool l3 = mode == CNDP_CFWD_L3FWD;
    const uint64_t *t24 = nullptr, *t8 = nullptr;
    if (l3) {
        const int r = fib_acquire(&fib->t, s, &t24, &t8);
        if (r)
            return r;
    }
    int r = 0;
    if (b->n) {
        CfwdArgs a;
        a.slab = (uint8_t *)(uintptr_t)b->slab;
        a.slab_len = b->slab_len;
        a.stride = b->stride;
        a.offsets = b->offsets;
        a.data_off = b->data_off;
        a.n = b->n;
        a.sel = io->sel;
        a.nh = io->nh;
        a.tx_lport = io->tx_lport;
        a.echoed = io->echoed;
        a.bin_of = io->bin_of;
        a.stats = (unsigned long long *)io->stats;
        a.m0 = io->lport_mask[0];
        a.m1 = io->lport_mask[1];
        a.m2 = io->lport_mask[2];
        a.m3 = io->lport_mask[3];
        a.in_lport = io->in_lport;
        a.n_bins = io->n_bins;

        const uint64_t want = ((uint64_t)b->n + CFWD_BLOCK - 1u) / CFWD_BLOCK;
        const uint64_t cap = (uint64_t)d->cus * CFWD_BLOCKS_PER_CU;
        const uint32_t grid = (uint32_t)(want < cap ? want : cap);
        if (l3)
            hipLaunchKernelGGL(cfwd_kernel<CNDP_CFWD_L3FWD>, dim3(grid), dim3(CFWD_BLOCK), 0, s, a, t24, t8);
        else
            hipLaunchKernelGGL(cfwd_kernel<CNDP_CFWD_FWD>, dim3(grid), dim3(CFWD_BLOCK), 0, s, a, t24, t8);
        if (hipGetLastError() != hipSuccess)
            r = -EIO;
    }
    if (l3)
        fib_release(&fib->t);
    if (r || b->n == 0)
        return r;
    HIP_TRY(hipEventRecord(d->ev, s));
    d->last = s;
    d->have_last = 1;
    return 0;
}

extern "C" int cndp_gpu_cfwd(cndp_gpu_ctx_t *ctx, struct cne_fib *fib, const struct cndp_batch *b, uint32_t mode,
                             const struct cndp_cfwd_io *io, void *stream)
{
    if (!ctx)
        return -EINVAL;
    int r = cfwd_io_check(fib, b, mode, io);
    if (r)
        return r;
    const int dev = cndp_gpu_device(ctx);
    HIP_TRY(hipSetDevice(dev));
    pthread_mutex_lock(&g_lock);
    CfwdDev *d = NULL;
    r = cfwd_dev_get(dev, &d);
    if (!r)
        r = cfwd_run(d, fib, b, mode, io, (hipStream_t)stream);
    pthread_mutex_unlock(&g_lock);
    return r;
}

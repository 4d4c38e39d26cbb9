// cndp_fwd.hip -- ip4_forward on MI355X (include/cndp_fwd.h).
//
// One kernel per call.  A block of 256 threads owns whole graph bursts,
// floor(256 / burst) of them per pass, so a burst's compacted stream of taken
// frames -- the node's objs[] -- never crosses a block:
//   pass 1  one frame per thread: the taken flag, a wave ballot into LDS, and from
//           the ballots of the burst's threads the frame's rank among the burst's
//           taken frames and the burst's count C; the thread's index is
//           scattered into the burst's compacted list in LDS.
//   pass 2  one thread per compacted entry: dst, TTL and checksum loaded, TTL and
//           checksum stored, the ARP lookup on dst; entries below C & ~3 form
//           the reference's groups of four consecutive RANKS and exchange their
//           hit flag, then lane 0's gateway entry, through LDS (a group can
//           straddle a DPP quad or a wave when burst is no multiple of 4 or a
//           block holds several bursts, so no cross-lane operation is used); the
//           route and gateway lookups where the rule asks for them; the MACs.
// Every frame read and write is bounded by slab_len; stores are plain vector
// stores.  Counters go through LDS to one global atomic per block and counter.
//
// The object image's device mirror is one buffer, updated in place and guarded
// by an event; the FIB mirrors are read through views.  Every reader --
// cndp_gpu_ip4_forward here, the mbuf queue's CNDP_MQ_IP4_FORWARD kernel in
// cndp_gpu.hip -- brackets its launch with fwd_dev_begin / fwd_dev_end
// (fwd_internal.h).
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fwd_internal.h"

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            fprintf(stderr, "cndp_fwd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),   \
                    __FILE__, __LINE__);                                                         \
            return e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? -ENODEV : -EIO;       \
        }                                                                                        \
    } while (0)

#define FWD_BLOCK 256u
#define FWD_BLOCKS_PER_CU 8u

// one FIB's device mirror: the /16 directory in front of tbl24 when it has one
typedef struct fwd_fibv FibDev;

struct FwdArgs {
    uint8_t *slab;
    uint64_t slab_len;
    uint64_t stride;
    const uint64_t *offsets;
    uint32_t data_off;
    uint32_t n;
    const uint32_t *nh;
    const uint32_t *ptype;
    const uint32_t *rxmeta;
    const uint8_t *sel;
    uint16_t *fwd_edge;
    uint32_t *arp_idx;
    uint16_t *bin_of;
    uint32_t n_bins;
    unsigned long long *stats;
    const uint32_t *img; // device mirror of the object image (fwd_internal.h)
    FibDev arp, rt;
    uint32_t burst;
    uint32_t per;   // frames a pass covers: floor(FWD_BLOCK / burst) * burst
    uint64_t tiles; // passes in the batch
};

// DIR-24-8 4B lookup (dir24_8.h:131-135), through the /16 directory when present
__device__ __forceinline__ uint32_t fib_lookup(const FibDev &f, uint32_t ip)
{
    uint32_t e;
    if (f.d16) {
        e = f.d16[ip >> 16];
        if (e & 1u)
            e = f.pages[(e >> 1) * 256u + ((ip >> 8) & 0xffu)];
    } else
        e = f.t24[ip >> 8];
    if (e & 1u)
        e = f.t8[(e >> 1) * 256u + (ip & 0xffu)];
    return e >> 1;
}

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

// the low k bytes of v at byte offset o, little-endian; a byte at or past len is not written
__device__ __forceinline__ void st_bytes(uint8_t *s, uint64_t len, uint64_t o, uint32_t v, uint32_t k)
{
    for (uint32_t j = 0; j < k; j++) {
        uint64_t x = o + j;
        if (x >= o && x < len)
            s[x] = (uint8_t)(v >> (8 * j));
    }
}

// whole [o, o + k) inside the slab
__device__ __forceinline__ bool inside(uint64_t len, uint64_t o, uint32_t k) { return o < len && len - o >= k; }

__device__ __forceinline__ uint64_t frame_off(const FwdArgs &a, uint64_t i)
{
    return (a.offsets ? a.offsets[i] : i * a.stride) + a.data_off;
}

// the ptype node's p_nxt[type] == ip4_input (lib/cnet/ptype/ptype.c:32-46)
__device__ __forceinline__ bool ptype_is_ip4_input(uint32_t pt)
{
    pt &= 0xffffu;
    return pt == 0x0211u || pt == 0x0111u || pt == 0x0231u || pt == 0x0291u;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        v += __shfl_xor(v, s, 64);
    return v;
}

// bits [lo, hi) of a 64-lane mask; lo and hi may lie outside [0, 64]
__device__ __forceinline__ unsigned long long lanes_below(int k)
{
    return k <= 0 ? 0ull : k >= 64 ? ~0ull : (1ull << k) - 1ull;
}
__device__ __forceinline__ uint32_t count_in(unsigned long long m, int lo, int hi)
{
    return (uint32_t)__popcll(m & lanes_below(hi) & ~lanes_below(lo));
}

__global__ __launch_bounds__(FWD_BLOCK) void ip4_forward_kernel(FwdArgs a)
{
    __shared__ unsigned long long s_ball[FWD_BLOCK / 64u];
    __shared__ uint16_t s_list[FWD_BLOCK]; // per burst: the threads of its taken frames, in order
    __shared__ uint8_t s_hit[FWD_BLOCK];   // per compacted entry: ARP hit on dst
    __shared__ uint32_t s_gw[FWD_BLOCK];   // per compacted entry: its gateway's ARP object, or none
    __shared__ uint32_t s_stat[3];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    if (t < 3)
        s_stat[t] = 0;
    const uint32_t arp_cap = a.img[0], rt_cap = a.img[1];
    const uint32_t *const arp = a.img + FWD_IMG_HDR, *const rt = arp + 2u * (size_t)arp_cap;
    const uint32_t *const nif = rt + 2u * (size_t)rt_cap;
    const bool slot = t < a.per;          // the pass has a frame, and an entry, for this thread
    const uint32_t lb = t / a.burst;      // its burst within the pass
    const uint32_t seg = lb * a.burst;    // the burst's first thread
    const uint32_t pos = t - seg;
    uint32_t cnt[3] = {0, 0, 0};

    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint64_t base = tile * a.per;
        // ---- pass 1: flags, ranks, the compacted lists
        const uint64_t i1 = base + t;
        const bool live = slot && i1 < a.n;
        bool taken = false;
        if (live) {
            if (a.sel)
                taken = a.sel[i1] != 0;
            else {
                const uint32_t nh = a.nh[i1];
                taken = nh != CNDP_NH_INVALID && (nh >> 24) == 1u && ptype_is_ip4_input(a.ptype[i1]);
            }
        }
        const unsigned long long bal = __ballot(taken);
        if (lane == 0)
            s_ball[wv] = bal;
        if (live && !taken) {
            a.fwd_edge[i1] = (uint16_t)CNDP_FWD_EDGE_NONE;
            if (a.arp_idx)
                a.arp_idx[i1] = CNDP_FWD_NONE;
            if (a.bin_of)
                a.bin_of[i1] = (uint16_t)(a.n_bins + 1u);
        }
        __syncthreads();
        uint32_t rank = 0, C = 0;
        if (slot) {
#pragma unroll
            for (uint32_t w = 0; w < FWD_BLOCK / 64u; w++) {
                const unsigned long long m = s_ball[w];
                const int w0 = (int)(w * 64u);
                C += count_in(m, (int)seg - w0, (int)(seg + a.burst) - w0);
                rank += count_in(m, (int)seg - w0, (int)t - w0);
            }
        }
        if (taken)
            s_list[seg + rank] = (uint16_t)t; // rank < C <= burst: inside the burst's own segment
        __syncthreads();

        // ---- pass 2: thread t is entry `pos` of burst lb's compacted list
        const bool valid = slot && pos < C;
        const bool quad = valid && pos < (C & ~3u); // the 4-wide loop; else the 1-wide loop
        const uint32_t q0 = t - (pos & 3u);         // the group's lane 0
        uint64_t i = 0, f = 0;
        uint32_t key = 0, a_idx = CNDP_FWD_NONE;
        bool a_hit = false;
        if (valid) {
            i = base + s_list[t];
            f = frame_off(a, i);
            const uint64_t m = f + CNDP_RXMETA_L2(a.rxmeta[i]); // pktmbuf_mtod after eth_rx's adj_offset
            uint32_t w[3];
            rd_words<3>(a.slab, a.slab_len, m + 8u, w); // ttl, proto, checksum | src | dst
            // ipv4_adjust_cksum (cnet_ipv4.h:159-170)
            const uint32_t ttl = (w[0] - 1u) & 0xffu;
            const int32_t c = (int32_t)((w[0] >> 16) ^ 0xffffu) + (int32_t)0xfffe; // htobe16(0xFEFF)
            const uint32_t ck = ~(uint32_t)(c + (c >> 16)) & 0xffffu;
            if (m + 8u >= m && m + 8u < a.slab_len)
                a.slab[m + 8u] = (uint8_t)ttl;
            const uint64_t mc = m + 10u;
            if (mc >= m && inside(a.slab_len, mc, 2) && (((uintptr_t)a.slab + mc) & 1u) == 0)
                *(uint16_t *)(a.slab + mc) = (uint16_t)ck;
            else if (mc >= m)
                st_bytes(a.slab, a.slab_len, mc, ck, 2);
            key = __builtin_bswap32(w[2]); // be32toh(hdr->dst_addr)
            a_idx = fib_lookup(a.arp, key) & 0xffffffu;
            a_hit = a_idx < arp_cap && (arp[2u * (size_t)a_idx] & FWD_SET);
        }
        s_hit[t] = a_hit;
        __syncthreads();
        // a group with any direct hit resolves only those (ip4_forward.c:134-160)
        bool group_hit = a_hit;
        if (quad)
            group_hit = s_hit[q0] | s_hit[q0 + 1] | s_hit[q0 + 2] | s_hit[q0 + 3];
        uint32_t r_nif = 0, g_idx = CNDP_FWD_NONE;
        bool g_hit = false;
        if (valid && !group_hit) {
            const uint32_t r_idx = fib_lookup(a.rt, key) & 0xffffffu;
            if (r_idx < rt_cap) {
                const uint32_t gw = rt[2u * (size_t)r_idx], rw = rt[2u * (size_t)r_idx + 1u];
                if (rw & FWD_SET) { // a frame without a route object has no gateway: a miss
                    r_nif = rw & 0xffu;
                    g_idx = fib_lookup(a.arp, gw) & 0xffffffu; // gateway.s_addr as stored (:166,178,295)
                    g_hit = g_idx < arp_cap && (arp[2u * (size_t)g_idx] & FWD_SET);
                }
            }
        }
        s_gw[t] = g_hit ? g_idx : CNDP_FWD_NONE;
        __syncthreads();
        if (valid) {
            uint32_t edge = CNDP_FWD_EDGE_ARP_REQUEST, ha = CNDP_FWD_NONE, out_nif = 0;
            if (a_hit) {
                ha = a_idx;
                out_nif = (arp[2u * (size_t)a_idx] >> 16) & 0xffu;
                cnt[CNDP_FWD_STAT_DIRECT]++;
            } else if (g_hit) {
                // lanes 1-3 of a group read arp_fib[0] (:190,196,202); without one, their own
                ha = g_idx;
                if (quad && t != q0 && s_gw[q0] != CNDP_FWD_NONE)
                    ha = s_gw[q0];
                out_nif = r_nif;
                cnt[CNDP_FWD_STAT_GATEWAY]++;
            } else
                cnt[CNDP_FWD_STAT_ARP_REQUEST]++;
            if (ha != CNDP_FWD_NONE) {
                edge = out_nif + CNDP_FWD_EDGE_OUTPUT;
                const uint32_t h0 = arp[2u * (size_t)ha], h1 = arp[2u * (size_t)ha + 1u];
                const uint32_t m0 = nif[2u * out_nif], m1 = nif[2u * out_nif + 1u];
                // d_addr at +0, s_addr at +6
                const uint32_t d0 = (h0 & 0xffffu) | h1 << 16, d1 = h1 >> 16 | m0 << 16;
                const uint32_t d2 = m0 >> 16 | m1 << 16;
                const uintptr_t p = (uintptr_t)a.slab + f;
                if (inside(a.slab_len, f, 12) && (p & 3u) == 0) {
                    uint32_t *o = (uint32_t *)p;
                    o[0] = d0;
                    o[1] = d1;
                    o[2] = d2;
                } else if (inside(a.slab_len, f, 12) && (p & 1u) == 0) {
                    uint16_t *o = (uint16_t *)p;
                    o[0] = (uint16_t)d0;
                    o[1] = (uint16_t)(d0 >> 16);
                    o[2] = (uint16_t)d1;
                    o[3] = (uint16_t)(d1 >> 16);
                    o[4] = (uint16_t)d2;
                    o[5] = (uint16_t)(d2 >> 16);
                } else {
                    st_bytes(a.slab, a.slab_len, f, d0, 4);
                    if (f + 4u >= f)
                        st_bytes(a.slab, a.slab_len, f + 4u, d1, 4);
                    if (f + 8u >= f)
                        st_bytes(a.slab, a.slab_len, f + 8u, d2, 4);
                }
            }
            a.fwd_edge[i] = (uint16_t)edge;
            if (a.arp_idx)
                a.arp_idx[i] = ha;
            if (a.bin_of)
                a.bin_of[i] = (uint16_t)(ha != CNDP_FWD_NONE ? out_nif : a.n_bins);
        }
        // the next pass writes s_ball before its first barrier; every read of it lies
        // before the second barrier above, and s_list / s_hit / s_gw are written only
        // after the next pass's first barrier
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t s = wave_sum(cnt[k]);
        if (s && lane == 0)
            atomicAdd(&s_stat[k], s);
    }
    __syncthreads();
    if (a.stats && t < 3 && s_stat[t])
        atomicAdd(&a.stats[t], (unsigned long long)s_stat[t]);
}

// ---------------------------------------------------------------------------
// host side: the object image's device mirror and the FIB views
// ---------------------------------------------------------------------------
struct FwdDev {
    int dev;
    int cus;
    uint32_t *img; // img_words of the table, allocated on the first call
    uint64_t gen;  // table generation mirrored (0 = none)
    hipEvent_t ev; // end of the last call's kernel
    hipStream_t last;
    int have_last;
};

static void fwd_dev_release(void *p)
{
    FwdDev *d = (FwdDev *)p;
    if (hipSetDevice(d->dev) == hipSuccess) {
        (void)hipDeviceSynchronize();
        if (d->img)
            (void)hipFree(d->img);
        if (d->ev)
            (void)hipEventDestroy(d->ev);
    }
    free(d);
}

static int fwd_dev_init(FwdDev *d)
{
    HIP_TRY(hipDeviceGetAttribute(&d->cus, hipDeviceAttributeMultiprocessorCount, d->dev));
    HIP_TRY(hipEventCreateWithFlags(&d->ev, hipEventDisableTiming));
    return 0;
}

static int fwd_dev_get(struct cndp_fwd_tbl *t, int dev, FwdDev **out)
{
    FwdDev *d = (FwdDev *)t->dev;
    if (d && d->dev != dev)
        return -EINVAL; // one table, one device
    if (!d) {
        d = (FwdDev *)calloc(1, sizeof(*d));
        if (!d)
            return -ENOMEM;
        d->dev = dev;
        int r = fwd_dev_init(d);
        if (r) {
            fwd_dev_release(d);
            return r;
        }
        t->dev = d;
        t->dev_release = fwd_dev_release;
    }
    *out = d;
    return 0;
}

// Sync a FIB's mirror on `s` and take a view of its buffers: read under dev_lock
// with `views` held until the launch is enqueued, so a sync on another thread
// that replaces a buffer retires it instead of freeing it (fib_internal.h).
static int fib_acquire(struct cndp_tbl *t, hipStream_t s, FibDev *v)
{
    int r = cndp_tbl_dev_sync(t, s);
    if (r)
        return r;
    pthread_mutex_lock(&t->dev_lock);
    const bool dir = t->dev_dir16 && t->dev_pages;
    v->t24 = (const uint32_t *)t->dev_tbl24;
    v->t8 = (const uint32_t *)t->dev_tbl8;
    v->d16 = dir ? (const uint32_t *)t->dev_dir16 : nullptr;
    v->pages = dir ? (const uint32_t *)t->dev_pages : nullptr;
    r = v->t24 && v->t8 ? 0 : -EIO;
    if (!r)
        __atomic_add_fetch(&t->views, 1u, __ATOMIC_RELAXED);
    pthread_mutex_unlock(&t->dev_lock);
    return r;
}
static inline void fib_release(struct cndp_tbl *t) { __atomic_sub_fetch(&t->views, 1u, __ATOMIC_RELEASE); }

static int fwd_mirror(FwdDev *d, struct cndp_fwd_tbl *t, hipStream_t s)
{
    if (d->gen == t->gen)
        return 0;
    size_t lo = t->d_lo, hi = t->d_hi;
    if (!d->img) {
        HIP_TRY(hipMalloc((void **)&d->img, t->img_words * 4u));
        lo = 0;
        hi = t->img_words;
    }
    if (hi > lo) {
        HIP_TRY(hipMemcpyAsync(d->img + lo, t->img + lo, (hi - lo) * 4u, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s)); // the host table may change after we return
    }
    t->d_lo = SIZE_MAX;
    t->d_hi = 0;
    d->gen = t->gen;
    return 0;
}

static int fwd_launch(FwdDev *d, const FwdArgs &a, hipStream_t s)
{
    const uint64_t cap = (uint64_t)d->cus * FWD_BLOCKS_PER_CU;
    const uint32_t grid = (uint32_t)(a.tiles < cap ? a.tiles : cap);
    hipLaunchKernelGGL(ip4_forward_kernel, dim3(grid), dim3(FWD_BLOCK), 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// fwd_dev_begin under t->lock: the device, the wait for a reader on another
// stream, the image's mirror, both FIB mirrors synced and their views taken
static int fwd_begin_locked(struct cndp_fwd_tbl *t, int dev, hipStream_t s, FwdDev **out, FibDev *arp, FibDev *rt)
{
    HIP_TRY(hipSetDevice(dev));
    FwdDev *d = NULL;
    int r = fwd_dev_get(t, dev, &d);
    if (r)
        return r;
    if (d->have_last && d->last != s)
        HIP_TRY(hipStreamWaitEvent(s, d->ev, 0));
    if ((r = fwd_mirror(d, t, s)))
        return r;
    struct cndp_tbl *ta = &t->arp_fib->t, *tr = &t->rt4_fib->t;
    if ((r = fib_acquire(ta, s, arp)))
        return r;
    if ((r = fib_acquire(tr, s, rt))) {
        fib_release(ta);
        return r;
    }
    *out = d;
    return 0;
}

// fwd_dev_end under t->lock: the views dropped, the reader's end recorded
static int fwd_end_locked(struct cndp_fwd_tbl *t, hipStream_t s, int launched)
{
    FwdDev *d = (FwdDev *)t->dev;
    fib_release(&t->rt4_fib->t);
    fib_release(&t->arp_fib->t);
    if (!launched)
        return 0;
    HIP_TRY(hipEventRecord(d->ev, s));
    d->last = s;
    d->have_last = 1;
    return 0;
}

extern "C" int fwd_dev_begin(struct cndp_fwd_tbl *t, int dev, void *stream, const uint32_t **img,
                             struct fwd_fibv *arp, struct fwd_fibv *rt)
{
    pthread_mutex_lock(&t->lock);
    FwdDev *d = NULL;
    const int r = fwd_begin_locked(t, dev, (hipStream_t)stream, &d, arp, rt);
    if (r) {
        pthread_mutex_unlock(&t->lock);
        return r;
    }
    *img = d->img;
    return 0;
}

extern "C" int fwd_dev_end(struct cndp_fwd_tbl *t, void *stream, int launched)
{
    const int r = fwd_end_locked(t, (hipStream_t)stream, launched);
    pthread_mutex_unlock(&t->lock);
    return r;
}

extern "C" int fwd_dev_check(struct cndp_fwd_tbl *t, int dev)
{
    pthread_mutex_lock(&t->lock);
    const FwdDev *d = (const FwdDev *)t->dev;
    const int r = d && d->dev != dev ? -EINVAL : 0; // one table, one device
    pthread_mutex_unlock(&t->lock);
    return r;
}

static int fwd_run(FwdDev *d, const struct cndp_batch *b, uint32_t burst, const struct cndp_fwd_io *io,
                   const FibDev &arp, const FibDev &rt, hipStream_t s)
{
    FwdArgs a;
    a.slab = (uint8_t *)b->slab;
    a.slab_len = b->slab_len;
    a.stride = b->stride;
    a.offsets = b->offsets;
    a.data_off = b->data_off;
    a.n = b->n;
    a.nh = b->nh;
    a.ptype = b->ptype;
    a.rxmeta = b->rxmeta;
    a.sel = io->sel;
    a.fwd_edge = io->fwd_edge;
    a.arp_idx = io->arp_idx;
    a.bin_of = io->bin_of;
    a.n_bins = io->n_bins;
    a.stats = (unsigned long long *)io->stats;
    a.img = d->img;
    a.arp = arp;
    a.rt = rt;
    a.burst = burst;
    a.per = FWD_BLOCK / burst * burst;
    a.tiles = ((uint64_t)b->n + a.per - 1u) / a.per;
    return fwd_launch(d, a, s);
}

extern "C" int cndp_gpu_ip4_forward(cndp_gpu_ctx_t *ctx, cndp_fwd_tbl_t *tbl, const struct cndp_batch *b,
                                    uint32_t burst, const struct cndp_fwd_io *io, void *stream)
{
    if (!ctx || !tbl || !b || !io || burst < 1u || burst > 256u)
        return -EINVAL;
    if (b->n && (!b->slab || !b->nh || !b->rxmeta || !io->fwd_edge || (!io->sel && !b->ptype)))
        return -EINVAL;
    const int dev = cndp_gpu_device(ctx);
    HIP_TRY(hipSetDevice(dev));
    pthread_mutex_lock(&tbl->lock);
    int r = 0;
    if (io->bin_of && ((int64_t)io->n_bins <= (int64_t)fwd_max_netif(tbl) || io->n_bins > 65533u))
        r = -EINVAL;
    FwdDev *d = NULL;
    FibDev arp, rt;
    if (!r)
        r = fwd_begin_locked(tbl, dev, (hipStream_t)stream, &d, &arp, &rt);
    if (!r) {
        if (b->n)
            r = fwd_run(d, b, burst, io, arp, rt, (hipStream_t)stream);
        const int e = fwd_end_locked(tbl, (hipStream_t)stream, b->n && !r);
        r = r ? r : e;
    }
    pthread_mutex_unlock(&tbl->lock);
    return r;
}

// cndp_tcp.hip -- tcp_input's lookup, checksum and segment record on MI355X
// (include/cndp_tcp.h).
//
// Two kernels per call, no host round trip between them:
//   tcp_demux_kernel  one frame per lane.  The table's TCP image (pcb_internal.h:
//                     an exact 4-tuple hash, a port directory, per-port wildcard
//                     runs) is staged in LDS once per block and answered by the
//                     same pcb_tcp_lookup() the host uses, so a frame of an
//                     established connection costs a probe or two whatever the
//                     number of connections on its port.  Every hit is appended
//                     to the block's segment of a device worklist (an LDS
//                     counter, one atomic per wave, one count per block); an entry
//                     carries the segment's byte offset, its length and the folded
//                     pseudo-header sum, so the second kernel starts its loads
//                     from the entry alone.
//   tcp_cksum_kernel  the same grid, block b reading demux block b's segment: a
//                     16-lane group per TCP segment, 16-byte aligned loads with
//                     the head and tail masked, per-lane byte sums, a cross-lane
//                     reduction, then the reference's own folds.  A segment that
//                     fails gets the drop values written over its outputs.
// Every frame read is bounded by slab_len; no load leaves the slab.
//
// The TCP image's device mirror is one buffer guarded by an event.  Every reader
// -- cndp_gpu_tcp_input here, the mbuf queue's CNDP_MQ_TCP_INPUT kernel in
// cndp_gpu.hip -- brackets its launch with pcb_tdev_begin / pcb_tdev_end
// (pcb_internal.h).
//
// The byte readers and the checksum arithmetic are those of cndp_l4.hip, kept as
// a copy so that translation unit stays as it is.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pcb_internal.h"

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            fprintf(stderr, "cndp_tcp: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),   \
                    __FILE__, __LINE__);                                                         \
            return e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? -ENODEV : -EIO;       \
        }                                                                                        \
    } while (0)

// The image can take 120 KiB of the CU's 160 KiB of LDS (4096 connections), so
// one block per CU is all that fits then, and the block is what sets occupancy:
// 1024 lanes = 16 waves = 4 per SIMD with the largest image; an image of 80 KiB
// or less (up to about 3300 connections on a few ports) lets two blocks share a CU, 8 waves per SIMD,
// the most the CU holds.  __launch_bounds__(1024) keeps the kernels at or under
// the 128 VGPRs that 4 waves per SIMD allow.
#define TCP_BLOCK 1024u
#define TCP_LDS_MAX (160u * 1024u - 256u) // the block's static LDS comes out of the same 160 KiB
#define TCP_BLOCKS_PER_CU 2u
#define TCP_WL_BADOFF 0x80000000u // in an entry's third word: the frame's edge is the rx_badoff drop

#define EDGE_SEG CNDP_L4_EDGE(CNDP_L4_NODE_TCP_INPUT, CNDP_TCP_INPUT_SEGMENT)
#define EDGE_DROP CNDP_L4_EDGE(CNDP_L4_NODE_TCP_INPUT, CNDP_TCP_INPUT_PKT_DROP)
#define EDGE_PUNT CNDP_L4_EDGE(CNDP_L4_NODE_TCP_INPUT, CNDP_TCP_INPUT_PKT_PUNT)
#define EDGE_TAKE CNDP_L4_EDGE(CNDP_L4_NODE_IP4_PROTO, CNDP_IP4_PROTO_TCP)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct TcpArgs {
    const uint8_t *slab;
    uint64_t slab_len;
    uint64_t stride;
    const uint64_t *offsets;
    uint32_t data_off;
    uint32_t n;
    const uint32_t *rxmeta;
    const uint8_t *sel;
    uint8_t *l4edge;
    uint32_t *pcb;
    uint32_t *ports;
    u32x4 *seg;
    uint16_t *bin_of;
    uint32_t n_bins;
    unsigned long long *stats;
    const uint32_t *img; // device mirror of the table's TCP image
    // worklist of the frames whose checksum is to be verified: one segment of
    // wl_seg entries per demux block, its length in wl_cnt[block].  An entry is
    // { frame index, byte offset low, byte offset high | TCP_WL_BADOFF,
    //   bytes to sum | folded pseudo-header sum << 16 }, offset and bytes
    // already cut to the slab.
    u32x4 *wl;
    uint32_t *wl_cnt;
    uint32_t wl_seg;
};

__device__ __forceinline__ uint32_t bswap16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

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

__device__ __forceinline__ uint64_t frame_off(const TcpArgs &a, uint32_t i)
{
    return (a.offsets ? a.offsets[i] : (uint64_t)i * a.stride) + a.data_off;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        v += __shfl_xor(v, s, 64);
    return v;
}

// per-lane counters -> one global atomic per block and counter (s_stat zeroed
// by the caller before a barrier)
__device__ __forceinline__ void add_stats(unsigned long long *stats, uint32_t (&c)[4], uint32_t *s_stat)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t t = wave_sum(c[k]);
        if (t && (threadIdx.x & 63u) == 0)
            atomicAdd(&s_stat[k], t);
    }
    __syncthreads();
    if (stats && threadIdx.x < 4 && s_stat[threadIdx.x])
        atomicAdd(&stats[threadIdx.x], (unsigned long long)s_stat[threadIdx.x]);
}

extern __shared__ uint32_t tcp_lds[];

__global__ __launch_bounds__(TCP_BLOCK) void tcp_demux_kernel(TcpArgs a)
{
    const uint32_t words = a.img[3];
    __shared__ uint32_t s_stat[4], s_wl;
    if (threadIdx.x < 4)
        s_stat[threadIdx.x] = 0;
    if (threadIdx.x == 0)
        s_wl = 0;
    for (uint32_t k = threadIdx.x; k < words; k += TCP_BLOCK)
        tcp_lds[k] = a.img[k];
    __syncthreads();
    const uint32_t flags = tcp_lds[2];
    u32x4 *const wl = a.wl + (size_t)blockIdx.x * a.wl_seg;

    const uint32_t lane = threadIdx.x & 63u;
    uint32_t cnt[4] = {0, 0, 0, 0};
    const uint64_t step = (uint64_t)gridDim.x * TCP_BLOCK;
    for (uint64_t base = (uint64_t)blockIdx.x * TCP_BLOCK; base < a.n; base += step) {
        const uint64_t i64 = base + threadIdx.x;
        const bool live = i64 < a.n;
        const uint32_t i = (uint32_t)i64;
        bool taken = false;
        if (live)
            taken = a.sel ? a.sel[i] != 0 : a.l4edge[i] == EDGE_TAKE;
        uint32_t edge = CNDP_L4_EDGE_NONE, pcb = CNDP_PCB_NONE, ports = 0;
        uint32_t bin = a.n_bins + 1u;
        u32x4 seg = {0u, 0u, 0u, 0u}, ent = {0u, 0u, 0u, 0u};
        bool need = false;
        if (taken) {
            const uint32_t rx = a.rxmeta[i];
            const uint32_t l2 = CNDP_RXMETA_L2(rx), l3 = CNDP_RXMETA_L3(rx);
            const uint64_t m = frame_off(a, i) + l2; // pktmbuf_mtod after eth_rx's adj_offset
            uint32_t ip[5], th[5];
            rd_words<5>(a.slab, a.slab_len, m, ip);
            rd_words<5>(a.slab, a.slab_len, m + l3, th);
            const uint32_t faddr = ip[3], laddr = ip[4];
            ports = th[0]; // stored before the lookup
            const uint32_t hit = pcb_tcp_lookup(tcp_lds, laddr, faddr, th[0] >> 16, th[0] & 0xffffu);
            const uint32_t ihl = (ip[0] & 0xfu) * 4u, tot = bswap16(ip[0] >> 16);
            if (hit == CNDP_PCB_NONE) {
                if (flags & PCB_F_PUNT)
                    edge = EDGE_PUNT;
                else {
                    edge = EDGE_DROP;
                    bin = a.n_bins;
                }
                cnt[CNDP_TCP_STAT_NOMATCH]++;
            } else if (tot < ihl) { // __ipv4_udptcp_cksum sums to 0, which fails the verify
                edge = EDGE_DROP;
                bin = a.n_bins;
                cnt[CNDP_TCP_STAT_CKSUM]++;
            } else {
                // what stands if the checksum verifies; tcp_cksum_kernel counts it,
                // or writes the drop values over it
                need = true;
                pcb = hit;
                const uint32_t offset = (th[3] & 0xf0u) >> 2;
                uint32_t wlflag = 0;
                if (offset < 20u || offset > tot) { // rx_badoff
                    edge = EDGE_DROP;
                    bin = a.n_bins;
                    wlflag = TCP_WL_BADOFF;
                } else {
                    edge = EDGE_SEG;
                    bin = hit;
                    const uint32_t fl = (th[3] >> 8) & 0x3fu;
                    const uint32_t synfin = (fl & 1u) + ((fl >> 1) & 1u); // tcp_syn_fin_cnt[flags & SYN_FIN]
                    const uint32_t len = (tot - (offset + l3) + synfin) & 0xffffu;
                    seg.x = __builtin_bswap32(th[1]);
                    seg.y = __builtin_bswap32(th[2]);
                    seg.z = bswap16(th[3] >> 16) | bswap16(th[4] >> 16) << 16;
                    seg.w = len | fl << 16 | offset << 24;
                }
                // the bytes to sum, cut to the slab: past it they read as zero and add nothing
                const uint32_t L = tot - ihl;
                uint64_t ub = m + l3, ue = ub + L;
                if (ue > a.slab_len || ue < ub)
                    ue = a.slab_len;
                if (ub > ue)
                    ub = ue;
                uint32_t ph = (ip[3] & 0xffffu) + (ip[3] >> 16) + (ip[4] & 0xffffu) + (ip[4] >> 16) +
                              (((ip[2] >> 8) & 0xffu) << 8) + bswap16(L);
                ph = (ph >> 16) + (ph & 0xffffu);
                ph = (ph >> 16) + (ph & 0xffffu);
                ent.x = i;
                ent.y = (uint32_t)ub;
                ent.z = (uint32_t)(ub >> 32) | wlflag; // slab_len < 2^63: the top bit is free
                ent.w = (uint32_t)(ue - ub) | (ph & 0xffffu) << 16;
            }
        }
        if (live) {
            if (taken)
                a.l4edge[i] = (uint8_t)edge;
            if (a.pcb)
                a.pcb[i] = pcb;
            if (a.ports)
                a.ports[i] = ports;
            if (a.seg)
                a.seg[i] = seg;
            if (a.bin_of)
                a.bin_of[i] = (uint16_t)bin;
        }
        // worklist append: one (LDS) atomic per wave, ballot + prefix for the lanes
        const unsigned long long mask = __ballot(need);
        if (mask) {
            const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
            uint32_t at = 0;
            if (lane == leader)
                at = atomicAdd(&s_wl, (uint32_t)__popcll(mask));
            at = __shfl(at, (int)leader, 64);
            if (need) // at most one entry per frame the block looks at: < wl_seg
                wl[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = ent;
        }
    }
    add_stats(a.stats, cnt, s_stat); // its barrier also orders the block's s_wl updates
    if (threadIdx.x == 0)
        a.wl_cnt[blockIdx.x] = s_wl;
}

// dword at address y of a segment occupying [lo, hi): bytes outside read as zero
__device__ __forceinline__ uint32_t mask_dword(uint32_t d, uintptr_t y, uintptr_t lo, uintptr_t hi)
{
    uint32_t mk = 0xffffffffu;
    if (lo > y) {
        uintptr_t k = lo - y;
        mk = k >= 4 ? 0u : mk << (8u * (uint32_t)k);
    }
    if (hi < y + 4) {
        uintptr_t k = hi > y ? hi - y : 0;
        mk &= k == 0 ? 0u : 0xffffffffu >> (8u * (4u - (uint32_t)k));
    }
    return d & mk;
}

__global__ __launch_bounds__(TCP_BLOCK) void tcp_cksum_kernel(TcpArgs a)
{
    // block b takes the segment demux block b filled
    __shared__ uint32_t s_stat[4];
    if (threadIdx.x < 4)
        s_stat[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t total = a.wl_cnt[blockIdx.x];
    const u32x4 *const wl = a.wl + (size_t)blockIdx.x * a.wl_seg;
    const uint32_t gl = threadIdx.x & 15u; // lane within the 16-lane group
    const uint32_t grp = threadIdx.x >> 4;
    const uint32_t ngrp = TCP_BLOCK / 16u;
    const uint32_t wave_first = grp & ~3u; // the wave's four groups stay in step for the shuffles
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t k0 = wave_first; k0 < total; k0 += ngrp) {
        const uint32_t k = k0 + (grp & 3u);
        const bool valid = k < total;
        u32x4 e = {0u, 0u, 0u, 0u};
        uint32_t se = 0, so = 0; // sums of the bytes at even / odd addresses
        uintptr_t lo = 0;
        if (valid) {
            e = wl[k]; // the group's 16 lanes read one entry: a broadcast
            const uint64_t ub = (uint64_t)(e.z & ~TCP_WL_BADOFF) << 32 | e.y;
            const uintptr_t P = (uintptr_t)a.slab, Pend = P + a.slab_len;
            lo = P + ub; // ub + bytes <= slab_len: the demux kernel cut them
            const uintptr_t hi = lo + (e.w & 0xffffu);
            const uintptr_t A = lo & ~(uintptr_t)15;
            const uint64_t nch = hi > lo ? (hi - A + 15u) / 16u : 0;
            for (uint64_t c = gl; c < nch; c += 16) {
                const uintptr_t X = A + 16u * c;
                if (X >= P && X + 16 <= Pend) {
                    u32x4 v = __builtin_nontemporal_load((const u32x4 *)X);
                    uint32_t d[4] = {v.x, v.y, v.z, v.w};
                    if (X < lo || X + 16 > hi) {
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            d[q] = mask_dword(d[q], X + 4u * q, lo, hi);
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        se = __builtin_amdgcn_sad_u8(d[q] & 0x00ff00ffu, 0u, se);
                        so = __builtin_amdgcn_sad_u8((d[q] >> 8) & 0x00ff00ffu, 0u, so);
                    }
                } else { // a chunk that straddles the slab's own edge
                    const uintptr_t x0 = X > lo ? X : lo, x1 = X + 16 < hi ? X + 16 : hi;
                    for (uintptr_t x = x0; x < x1; x++) {
                        const uint32_t bv = *(const uint8_t *)x;
                        if (x & 1u)
                            so += bv;
                        else
                            se += bv;
                    }
                }
            }
        }
        // words are little-endian pairs counted from the segment's first byte
        uint32_t S = (lo & 1u) ? so + (se << 8) : se + (so << 8);
#pragma unroll
        for (int s = 8; s >= 1; s >>= 1)
            S += __shfl_xor(S, s, 64);
        if (valid && gl == 0) {
            // cne_raw_cksum's reduce, + cne_ipv4_phdr_cksum (folded by the demux
            // kernel), + __ipv4_udptcp_cksum's fold
            S = (S >> 16) + (S & 0xffffu);
            S = (S >> 16) + (S & 0xffffu);
            S &= 0xffffu;
            uint32_t c = S + (e.w >> 16);
            c = ((c >> 16) + (c & 0xffffu)) & 0xffffu;
            const uint32_t i = e.x;
            if (c == 0xffffu)
                cnt[(e.z & TCP_WL_BADOFF) ? CNDP_TCP_STAT_BADOFF : CNDP_TCP_STAT_SEGMENT]++;
            else { // verify < 0: pkt_drop before m->userptr is set
                a.l4edge[i] = EDGE_DROP;
                if (a.pcb)
                    a.pcb[i] = CNDP_PCB_NONE;
                if (a.seg)
                    a.seg[i] = u32x4{0u, 0u, 0u, 0u};
                if (a.bin_of)
                    a.bin_of[i] = (uint16_t)a.n_bins;
                cnt[CNDP_TCP_STAT_CKSUM]++;
            }
        }
    }
    add_stats(a.stats, cnt, s_stat);
}

// ---------------------------------------------------------------------------
// host side: the table's device mirror
// ---------------------------------------------------------------------------
struct TcpDev {
    int dev;
    int cus;
    uint32_t *img;
    uint32_t img_cap; // words
    uint64_t gen;     // table generation mirrored (0 = none)
    u32x4 *wl;
    uint64_t wl_cap;
    uint32_t *cnt; // one count per demux block, cus * TCP_BLOCKS_PER_CU of them
    hipEvent_t ev; // end of the last call's kernels
    hipStream_t last;
    int have_last;
};

static void tcp_dev_release(void *p)
{
    TcpDev *d = (TcpDev *)p;
    if (hipSetDevice(d->dev) == hipSuccess) {
        (void)hipDeviceSynchronize();
        if (d->img)
            (void)hipFree(d->img);
        if (d->wl)
            (void)hipFree(d->wl);
        if (d->cnt)
            (void)hipFree(d->cnt);
        if (d->ev)
            (void)hipEventDestroy(d->ev);
    }
    free(d);
}

static int tcp_dev_init(TcpDev *d)
{
    HIP_TRY(hipDeviceGetAttribute(&d->cus, hipDeviceAttributeMultiprocessorCount, d->dev));
    HIP_TRY(hipMalloc((void **)&d->cnt, (size_t)d->cus * TCP_BLOCKS_PER_CU * sizeof(uint32_t)));
    HIP_TRY(hipEventCreateWithFlags(&d->ev, hipEventDisableTiming));
    // more than the 64 KiB a kernel gets by default; a refusal shows as that launch's error
    (void)hipFuncSetAttribute((const void *)tcp_demux_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)TCP_LDS_MAX);
    (void)hipGetLastError();
    return 0;
}

static int tcp_dev_get(struct cndp_pcb_tbl *t, int dev, TcpDev **out)
{
    TcpDev *d = (TcpDev *)t->tdev;
    if (d && d->dev != dev)
        return -EINVAL; // one table, one device
    if (!d) {
        d = (TcpDev *)calloc(1, sizeof(*d));
        if (!d)
            return -ENOMEM;
        d->dev = dev;
        int r = tcp_dev_init(d);
        if (r) {
            tcp_dev_release(d);
            return r;
        }
        t->tdev = d;
        t->tdev_release = tcp_dev_release;
    }
    *out = d;
    return 0;
}

// pcb_tdev_begin under t->lock: the device, the host image, the wait for a
// reader on another stream, the mirror brought up to date
static int tcp_begin_locked(struct cndp_pcb_tbl *t, int dev, hipStream_t s, TcpDev **out)
{
    HIP_TRY(hipSetDevice(dev));
    TcpDev *d = NULL;
    int r = tcp_dev_get(t, dev, &d);
    if (r)
        return r;
    if ((r = pcb_tcp_image(t)))
        return r;
    if (d->have_last && d->last != s)
        HIP_TRY(hipStreamWaitEvent(s, d->ev, 0));
    if (d->gen != t->timg_gen) {
        if (d->img_cap < t->timg_words) {
            if (d->img)
                HIP_TRY(hipFree(d->img)); // waits for the kernels still reading it
            d->img = NULL;
            d->img_cap = 0;
            HIP_TRY(hipMalloc((void **)&d->img, (size_t)t->timg_words * 4u));
            d->img_cap = t->timg_words;
        }
        HIP_TRY(hipMemcpyAsync(d->img, t->timg, (size_t)t->timg_words * 4u, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s)); // the host table may change after we return
        d->gen = t->timg_gen;
    }
    *out = d;
    return 0;
}

// pcb_tdev_end under t->lock: the reader's end recorded
static int tcp_end_locked(struct cndp_pcb_tbl *t, hipStream_t s, int launched)
{
    TcpDev *d = (TcpDev *)t->tdev;
    if (!launched || !d)
        return 0;
    HIP_TRY(hipEventRecord(d->ev, s));
    d->last = s;
    d->have_last = 1;
    return 0;
}

extern "C" int pcb_tdev_begin(struct cndp_pcb_tbl *t, int dev, void *stream, const uint32_t **img)
{
    pthread_mutex_lock(&t->lock);
    TcpDev *d = NULL;
    const int r = tcp_begin_locked(t, dev, (hipStream_t)stream, &d);
    if (r) {
        pthread_mutex_unlock(&t->lock);
        return r;
    }
    *img = d->img;
    return 0;
}

extern "C" int pcb_tdev_end(struct cndp_pcb_tbl *t, void *stream, int launched)
{
    const int r = tcp_end_locked(t, (hipStream_t)stream, launched);
    pthread_mutex_unlock(&t->lock);
    return r;
}

extern "C" int pcb_tdev_check(struct cndp_pcb_tbl *t, int dev)
{
    pthread_mutex_lock(&t->lock);
    const TcpDev *d = (const TcpDev *)t->tdev;
    const int r = d && d->dev != dev ? -EINVAL : 0; // one table, one device
    pthread_mutex_unlock(&t->lock);
    return r;
}

static int tcp_run(TcpDev *d, struct cndp_pcb_tbl *t, const struct cndp_batch *b,
                   const struct cndp_tcp_io *io, hipStream_t s)
{
    const uint32_t lds = t->timg_words * 4u;
    if (lds > TCP_LDS_MAX)
        return -E2BIG; // cannot happen within CNDP_PCB_MAX_ENTRIES (pcb_internal.h)
    uint32_t per_cu = TCP_LDS_MAX / lds; // lds >= the header
    per_cu = per_cu < 1u ? 1u : per_cu > TCP_BLOCKS_PER_CU ? TCP_BLOCKS_PER_CU : per_cu;
    const uint64_t want = ((uint64_t)b->n + TCP_BLOCK - 1u) / TCP_BLOCK;
    const uint64_t cap = (uint64_t)d->cus * per_cu;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    // a block looks at ceil(want / grid) tiles of TCP_BLOCK frames: its worklist segment
    const uint32_t seg = (uint32_t)((want + grid - 1u) / grid) * TCP_BLOCK;
    if (d->wl_cap < (uint64_t)grid * seg) {
        if (d->wl)
            HIP_TRY(hipFree(d->wl));
        d->wl = NULL;
        d->wl_cap = 0;
        HIP_TRY(hipMalloc((void **)&d->wl, (size_t)grid * seg * sizeof(u32x4)));
        d->wl_cap = (uint64_t)grid * seg;
    }
    TcpArgs a;
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
    a.ports = io->ports;
    a.seg = (u32x4 *)io->seg;
    a.bin_of = io->bin_of;
    a.n_bins = io->n_bins;
    a.stats = (unsigned long long *)io->stats;
    a.img = d->img;
    a.wl = d->wl;
    a.wl_cnt = d->cnt;
    a.wl_seg = seg;

    hipLaunchKernelGGL(tcp_demux_kernel, dim3(grid), dim3(TCP_BLOCK), lds, s, a);
    HIP_TRY(hipGetLastError());
    // the same grid, reading each segment's count on the device
    hipLaunchKernelGGL(tcp_cksum_kernel, dim3(grid), dim3(TCP_BLOCK), 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int cndp_gpu_tcp_input(cndp_gpu_ctx_t *ctx, cndp_pcb_tbl_t *tbl, const struct cndp_batch *b,
                                  const struct cndp_tcp_io *io, void *stream)
{
    if (!ctx || !tbl || !b || !io)
        return -EINVAL;
    if (b->n && (!b->slab || !b->rxmeta || !io->l4edge || ((uintptr_t)io->seg & 15u) || (b->slab_len >> 63)))
        return -EINVAL;
    const int dev = cndp_gpu_device(ctx);
    HIP_TRY(hipSetDevice(dev));
    pthread_mutex_lock(&tbl->lock);
    int r = 0;
    if (io->bin_of && (io->n_bins < tbl->count || io->n_bins > 65533u))
        r = -EINVAL;
    TcpDev *d = NULL;
    if (!r)
        r = tcp_begin_locked(tbl, dev, (hipStream_t)stream, &d);
    if (!r) {
        if (b->n)
            r = tcp_run(d, tbl, b, io, (hipStream_t)stream);
        const int e = tcp_end_locked(tbl, (hipStream_t)stream, b->n && !r);
        r = r ? r : e;
    }
    pthread_mutex_unlock(&tbl->lock);
    return r;
}

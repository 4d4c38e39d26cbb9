// cndp_l4.hip -- ip4_proto + udp_input on MI355X (include/cndp_l4.h).
//
// Two kernels per call, no host round trip between them:
//   l4_demux_kernel  one frame per lane.  The table image (pcb_internal.h) is
//                    staged in LDS once per block; a lane hashes its local port
//                    into the port directory and walks only that port's run, so
//                    the work per frame does not grow with other ports' sockets.
//                    Frames whose PCB asks for a checksum verify are appended to
//                    the block's segment of a device worklist, one LDS atomic per
//                    wave (ballot + prefix).
//   l4_cksum_kernel  the same grid, block b reading the count of demux block b's
//                    worklist segment from device memory: a 16-lane group per
//                    datagram, 16-byte aligned loads with the head and tail
//                    masked, per-lane integer byte sums, a cross-lane reduction,
//                    then the reference's own folds.
// Every frame read is bounded by slab_len; no load leaves the slab.
//
// The image's device mirror is one buffer guarded by an event.  Every reader --
// cndp_gpu_udp_input here, the mbuf queue's CNDP_MQ_UDP_INPUT kernel in
// cndp_gpu.hip -- brackets its launch with pcb_dev_begin / pcb_dev_end
// (pcb_internal.h).
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
            fprintf(stderr, "cndp_l4: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),    \
                    __FILE__, __LINE__);                                                         \
            return e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? -ENODEV : -EIO;       \
        }                                                                                        \
    } while (0)

#define L4_BLOCK 256u
#define L4_LDS_MAX (160u * 1024u)
#define L4_BLOCKS_PER_CU 8u // most blocks per CU the demux grid asks for

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct L4Args {
    const uint8_t *slab;
    uint64_t slab_len;
    uint64_t stride;
    const uint64_t *offsets;
    uint32_t data_off;
    uint32_t n;
    const uint32_t *nh;
    const uint32_t *ptype;
    const uint32_t *rxmeta;
    const uint8_t *sel;
    uint8_t *l4edge;
    uint32_t *pcb;
    uint32_t *ports;
    uint16_t *payload_off;
    uint16_t *bin_of;
    uint32_t n_bins;
    unsigned long long *stats;
    const uint32_t *img; // device mirror of the table image
    // worklist of frame indices that need a checksum verify: one segment of
    // wl_seg entries per demux block (filled through an LDS counter, so no
    // global atomic is contended), its length in wl_cnt[block]
    uint32_t *wl;
    uint32_t *wl_cnt;
    uint32_t wl_seg;
};

__device__ __forceinline__ uint32_t bswap16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

// N little-endian dwords at byte offset o of the slab, bytes at or past len read
// as zero.  Away from the slab's edges: aligned dword loads plus a byte shift
// (frame bytes sit at 2-byte alignment, the IP header at +14).
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

__device__ __forceinline__ uint64_t frame_off(const L4Args &a, uint32_t i)
{
    return (a.offsets ? a.offsets[i] : (uint64_t)i * a.stride) + a.data_off;
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

extern __shared__ uint32_t l4_lds[];

__global__ __launch_bounds__(L4_BLOCK) void l4_demux_kernel(L4Args a)
{
    const uint32_t n_ent = a.img[0], H = a.img[1], flags = a.img[2], words = a.img[3];
    __shared__ uint32_t s_stat[4], s_wl;
    if (threadIdx.x < 4)
        s_stat[threadIdx.x] = 0;
    if (threadIdx.x == 0)
        s_wl = 0;
    for (uint32_t k = PCB_IMG_HDR + threadIdx.x; k < words; k += L4_BLOCK)
        l4_lds[k - PCB_IMG_HDR] = a.img[k];
    __syncthreads();
    uint32_t *const wl = a.wl + (size_t)blockIdx.x * a.wl_seg;
    const uint32_t *t_laddr = l4_lds, *t_faddr = t_laddr + n_ent, *t_ports = t_faddr + n_ent;
    const uint32_t *t_slots = t_ports + n_ent;
    const uint16_t *t_idxf = (const uint16_t *)(t_slots + H);

    const uint32_t lane = threadIdx.x & 63u;
    uint32_t cnt[4] = {0, 0, 0, 0};
    const uint64_t step = (uint64_t)gridDim.x * L4_BLOCK;
    for (uint64_t base = (uint64_t)blockIdx.x * L4_BLOCK; base < a.n; base += step) {
        const uint64_t i64 = base + threadIdx.x;
        const bool live = i64 < a.n;
        const uint32_t i = (uint32_t)i64;
        bool taken = false;
        uint32_t rx = 0;
        if (live) {
            if (a.sel)
                taken = a.sel[i] != 0;
            else {
                uint32_t nh = a.nh[i];
                taken = nh != CNDP_NH_INVALID && (nh >> 24) == 2u && ptype_is_ip4_input(a.ptype[i]);
            }
            rx = a.rxmeta[i];
        }
        uint32_t edge = CNDP_L4_EDGE_NONE, pcb = CNDP_PCB_NONE, ports = 0, poff = 0;
        uint32_t bin = a.n_bins + 1u;
        bool need = false;
        if (taken) {
            const uint32_t l2 = CNDP_RXMETA_L2(rx), l3 = CNDP_RXMETA_L3(rx), l4 = CNDP_RXMETA_L4(rx);
            const uint64_t m = frame_off(a, i) + l2; // pktmbuf_mtod after eth_rx's adj_offset
            uint32_t ip[5];
            rd_words<5>(a.slab, a.slab_len, m, ip);
            const uint32_t proto = (ip[2] >> 8) & 0xffu;
            if (proto != 17u) { // ip4_proto: proto_nxt[]
                if (proto == 6u && (flags & PCB_F_TCP))
                    edge = CNDP_L4_EDGE(CNDP_L4_NODE_IP4_PROTO, CNDP_IP4_PROTO_TCP);
                else {
                    edge = CNDP_L4_EDGE(CNDP_L4_NODE_IP4_PROTO, CNDP_IP4_PROTO_DROP);
                    bin = a.n_bins;
                    cnt[CNDP_L4_STAT_PROTO_DROP]++;
                }
            } else { // udp_input_lookup
                uint32_t u[2];
                rd_words<2>(a.slab, a.slab_len, m + l3, u);
                const uint32_t faddr = ip[3], laddr = ip[4];
                const uint32_t fport = u[0] & 0xffffu, lport = u[0] >> 16;
                ports = u[0];
                uint32_t bestw = 3, bestj = 0;
                uint32_t h = pcb_port_hash(lport, H);
                for (;;) {
                    const uint32_t s = t_slots[h];
                    if (!(s & PCB_SLOT_VALID))
                        break;
                    if (((s >> 12) & 0xffffu) == lport) {
                        for (uint32_t j = s & 0xfffu; j < n_ent; j++) {
                            const uint32_t pp = t_ports[j];
                            if ((pp >> 16) != lport)
                                break;
                            const uint32_t el = t_laddr[j], ef = t_faddr[j];
                            uint32_t w = 0;
                            if (el != 0) {
                                if (laddr == 0)
                                    w++;
                                else if (el != laddr)
                                    continue;
                            } else if (laddr != 0)
                                w++;
                            if (ef != 0) {
                                if (faddr == 0)
                                    w++;
                                else if (ef != faddr || (pp & 0xffffu) != fport)
                                    continue;
                            } else if (faddr != 0)
                                w++;
                            if (w < bestw) { // the run is in index order: first of the fewest wildcards
                                bestw = w;
                                bestj = j;
                                if (w == 0)
                                    break;
                            }
                        }
                        break;
                    }
                    h = (h + 1u) & (H - 1u);
                }
                if (bestw == 3) {
                    if (flags & PCB_F_PUNT)
                        edge = CNDP_L4_EDGE(CNDP_L4_NODE_UDP_INPUT, CNDP_UDP_INPUT_PKT_PUNT);
                    else {
                        edge = CNDP_L4_EDGE(CNDP_L4_NODE_UDP_INPUT, CNDP_UDP_INPUT_PKT_DROP);
                        bin = a.n_bins;
                    }
                    cnt[CNDP_L4_STAT_NOMATCH]++;
                } else {
                    const uint32_t idf = t_idxf[bestj];
                    bool ok = true;
                    if ((idf & PCB_IDXF_CKSUM) && (u[1] >> 16) != 0) {
                        // __ipv4_udptcp_cksum: total_length < header length sums to 0, which fails
                        const uint32_t ihl = (ip[0] & 0xfu) * 4u, tot = bswap16(ip[0] >> 16);
                        if (tot < ihl)
                            ok = false;
                        else
                            need = true; // verdict (and its count) from l4_cksum_kernel
                    }
                    if (ok) {
                        edge = CNDP_L4_EDGE(CNDP_L4_NODE_UDP_INPUT, CNDP_UDP_INPUT_CHNL_RECV);
                        pcb = idf & PCB_IDXF_IDX;
                        bin = pcb;
                        poff = l2 + l3 + l4;
                        if (!need)
                            cnt[CNDP_L4_STAT_RECV]++;
                    } else {
                        edge = CNDP_L4_EDGE(CNDP_L4_NODE_UDP_INPUT, CNDP_UDP_INPUT_PKT_DROP);
                        bin = a.n_bins;
                        cnt[CNDP_L4_STAT_CKSUM]++;
                    }
                }
            }
        }
        if (live) {
            a.l4edge[i] = (uint8_t)edge;
            if (a.pcb)
                a.pcb[i] = pcb;
            if (a.ports)
                a.ports[i] = ports;
            if (a.payload_off)
                a.payload_off[i] = (uint16_t)poff;
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
                wl[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = i;
        }
    }
    add_stats(a.stats, cnt, s_stat); // its barrier also orders the block's s_wl updates
    if (threadIdx.x == 0)
        a.wl_cnt[blockIdx.x] = s_wl;
}

// dword at address y of a datagram occupying [lo, hi): bytes outside read as zero
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

__global__ __launch_bounds__(L4_BLOCK) void l4_cksum_kernel(L4Args a)
{
    // block b takes the segment demux block b filled
    __shared__ uint32_t s_stat[4];
    if (threadIdx.x < 4)
        s_stat[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t total = a.wl_cnt[blockIdx.x];
    const uint32_t *const wl = a.wl + (size_t)blockIdx.x * a.wl_seg;
    const uint32_t gl = threadIdx.x & 15u; // lane within the 16-lane group
    const uint32_t grp = threadIdx.x >> 4;
    const uint32_t ngrp = L4_BLOCK / 16u;
    const uint32_t wave_first = grp & ~3u; // the wave's four groups stay in step for the shuffles
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t k0 = wave_first; k0 < total; k0 += ngrp) {
        const uint32_t k = k0 + (grp & 3u);
        const bool valid = k < total;
        uint32_t i = 0, ip[5] = {0, 0, 0, 0, 0}, L = 0;
        uint32_t se = 0, so = 0; // sums of the bytes at even / odd addresses
        uintptr_t lo = 0;
        if (valid) {
            i = wl[k];
            const uint32_t rx = a.rxmeta[i];
            const uint64_t m = frame_off(a, i) + CNDP_RXMETA_L2(rx);
            rd_words<5>(a.slab, a.slab_len, m, ip);
            L = bswap16(ip[0] >> 16) - (ip[0] & 0xfu) * 4u; // the demux kernel checked tot >= ihl
            uint64_t ub = m + CNDP_RXMETA_L3(rx), ue = ub + L;
            if (ue > a.slab_len)
                ue = a.slab_len; // bytes past the slab read as zero: they add nothing
            if (ub > ue)
                ub = ue;
            const uintptr_t P = (uintptr_t)a.slab, Pend = P + a.slab_len;
            lo = P + ub;
            const uintptr_t hi = P + ue;
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
        // words are little-endian pairs counted from the datagram's first byte
        uint32_t S = (lo & 1u) ? so + (se << 8) : se + (so << 8);
#pragma unroll
        for (int s = 8; s >= 1; s >>= 1)
            S += __shfl_xor(S, s, 64);
        if (valid && gl == 0) {
            // cne_raw_cksum's reduce, + cne_ipv4_phdr_cksum, + __ipv4_udptcp_cksum's fold
            S = (S >> 16) + (S & 0xffffu);
            S = (S >> 16) + (S & 0xffffu);
            S &= 0xffffu;
            uint32_t ph = (ip[3] & 0xffffu) + (ip[3] >> 16) + (ip[4] & 0xffffu) + (ip[4] >> 16) +
                          (((ip[2] >> 8) & 0xffu) << 8) + bswap16(L & 0xffffu);
            ph = (ph >> 16) + (ph & 0xffffu);
            ph = (ph >> 16) + (ph & 0xffffu);
            ph &= 0xffffu;
            uint32_t c = S + ph;
            c = ((c >> 16) + (c & 0xffffu)) & 0xffffu;
            if (c == 0xffffu)
                cnt[CNDP_L4_STAT_RECV]++;
            else { // verify < 0: pkt_drop, userptr left unset
                a.l4edge[i] = CNDP_L4_EDGE(CNDP_L4_NODE_UDP_INPUT, CNDP_UDP_INPUT_PKT_DROP);
                if (a.pcb)
                    a.pcb[i] = CNDP_PCB_NONE;
                if (a.payload_off)
                    a.payload_off[i] = 0;
                if (a.bin_of)
                    a.bin_of[i] = (uint16_t)a.n_bins;
                cnt[CNDP_L4_STAT_CKSUM]++;
            }
        }
    }
    add_stats(a.stats, cnt, s_stat);
}

// ---------------------------------------------------------------------------
// host side: the table's device mirror
// ---------------------------------------------------------------------------
struct L4Dev {
    int dev;
    int cus;
    uint32_t *img;
    uint32_t img_cap; // words
    uint64_t gen;     // table generation mirrored (0 = none)
    uint32_t *wl;
    uint64_t wl_cap;
    uint32_t *cnt; // one count per demux block (each block writes its own), cus * L4_BLOCKS_PER_CU of them
    hipEvent_t ev; // end of the last call's kernels
    hipStream_t last;
    int have_last;
};

static void l4_dev_release(void *p)
{
    L4Dev *d = (L4Dev *)p;
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

static int l4_dev_init(L4Dev *d)
{
    HIP_TRY(hipDeviceGetAttribute(&d->cus, hipDeviceAttributeMultiprocessorCount, d->dev));
    HIP_TRY(hipMalloc((void **)&d->cnt, (size_t)d->cus * L4_BLOCKS_PER_CU * sizeof(uint32_t)));
    HIP_TRY(hipEventCreateWithFlags(&d->ev, hipEventDisableTiming));
    // a table of thousands of distinct ports stages more than the 64 KiB a
    // kernel gets by default; a refusal shows as that launch's error
    (void)hipFuncSetAttribute((const void *)l4_demux_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)L4_LDS_MAX);
    (void)hipGetLastError();
    return 0;
}

static int l4_dev_get(struct cndp_pcb_tbl *t, int dev, L4Dev **out)
{
    L4Dev *d = (L4Dev *)t->dev;
    if (d && d->dev != dev)
        return -EINVAL; // one table, one device
    if (!d) {
        d = (L4Dev *)calloc(1, sizeof(*d));
        if (!d)
            return -ENOMEM;
        d->dev = dev;
        int r = l4_dev_init(d);
        if (r) {
            l4_dev_release(d);
            return r;
        }
        t->dev = d;
        t->dev_release = l4_dev_release;
    }
    *out = d;
    return 0;
}

// pcb_dev_begin under t->lock: the device, the host image, the wait for a
// reader on another stream, the mirror brought up to date
static int l4_begin_locked(struct cndp_pcb_tbl *t, int dev, hipStream_t s, L4Dev **out)
{
    HIP_TRY(hipSetDevice(dev));
    L4Dev *d = NULL;
    int r = l4_dev_get(t, dev, &d);
    if (r)
        return r;
    if ((r = pcb_image(t)))
        return r;
    if (d->have_last && d->last != s)
        HIP_TRY(hipStreamWaitEvent(s, d->ev, 0));
    if (d->gen != t->img_gen) {
        if (d->img_cap < t->img_words) {
            if (d->img)
                HIP_TRY(hipFree(d->img)); // waits for the kernels still reading it
            d->img = NULL;
            d->img_cap = 0;
            HIP_TRY(hipMalloc((void **)&d->img, (size_t)t->img_words * 4u));
            d->img_cap = t->img_words;
        }
        HIP_TRY(hipMemcpyAsync(d->img, t->img, (size_t)t->img_words * 4u, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s)); // the host table may change after we return
        d->gen = t->img_gen;
    }
    *out = d;
    return 0;
}

// pcb_dev_end under t->lock: the reader's end recorded
static int l4_end_locked(struct cndp_pcb_tbl *t, hipStream_t s, int launched)
{
    L4Dev *d = (L4Dev *)t->dev;
    if (!launched || !d)
        return 0;
    HIP_TRY(hipEventRecord(d->ev, s));
    d->last = s;
    d->have_last = 1;
    return 0;
}

extern "C" int pcb_dev_begin(struct cndp_pcb_tbl *t, int dev, void *stream, const uint32_t **img)
{
    pthread_mutex_lock(&t->lock);
    L4Dev *d = NULL;
    const int r = l4_begin_locked(t, dev, (hipStream_t)stream, &d);
    if (r) {
        pthread_mutex_unlock(&t->lock);
        return r;
    }
    *img = d->img;
    return 0;
}

extern "C" int pcb_dev_end(struct cndp_pcb_tbl *t, void *stream, int launched)
{
    const int r = l4_end_locked(t, (hipStream_t)stream, launched);
    pthread_mutex_unlock(&t->lock);
    return r;
}

extern "C" int pcb_dev_check(struct cndp_pcb_tbl *t, int dev)
{
    pthread_mutex_lock(&t->lock);
    const L4Dev *d = (const L4Dev *)t->dev;
    const int r = d && d->dev != dev ? -EINVAL : 0; // one table, one device
    pthread_mutex_unlock(&t->lock);
    return r;
}

static int l4_run(L4Dev *d, struct cndp_pcb_tbl *t, const struct cndp_batch *b,
                  const struct cndp_l4_io *io, hipStream_t s)
{
    // demux grid: sized from the CU count and the LDS the table image takes
    const uint32_t lds = (t->img_words - PCB_IMG_HDR) * 4u;
    uint32_t per_cu = lds ? L4_LDS_MAX / lds : L4_BLOCKS_PER_CU;
    per_cu = per_cu < 1u ? 1u : per_cu > L4_BLOCKS_PER_CU ? L4_BLOCKS_PER_CU : per_cu;
    const uint64_t want = ((uint64_t)b->n + L4_BLOCK - 1u) / L4_BLOCK;
    const uint64_t cap = (uint64_t)d->cus * per_cu;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    // a block looks at ceil(want / grid) tiles of L4_BLOCK frames: its worklist segment
    const uint32_t seg = (uint32_t)((want + grid - 1u) / grid) * L4_BLOCK;
    if (d->wl_cap < (uint64_t)grid * seg) {
        if (d->wl)
            HIP_TRY(hipFree(d->wl));
        d->wl = NULL;
        d->wl_cap = 0;
        HIP_TRY(hipMalloc((void **)&d->wl, (size_t)grid * seg * 4u));
        d->wl_cap = (uint64_t)grid * seg;
    }
    L4Args a;
    a.slab = (const uint8_t *)b->slab;
    a.slab_len = b->slab_len;
    a.stride = b->stride;
    a.offsets = b->offsets;
    a.data_off = b->data_off;
    a.n = b->n;
    a.nh = b->nh;
    a.ptype = b->ptype;
    a.rxmeta = b->rxmeta;
    a.sel = io->sel;
    a.l4edge = io->l4edge;
    a.pcb = io->pcb;
    a.ports = io->ports;
    a.payload_off = io->payload_off;
    a.bin_of = io->bin_of;
    a.n_bins = io->n_bins;
    a.stats = (unsigned long long *)io->stats;
    a.img = d->img;
    a.wl = d->wl;
    a.wl_cnt = d->cnt;
    a.wl_seg = seg;

    hipLaunchKernelGGL(l4_demux_kernel, dim3(grid), dim3(L4_BLOCK), lds, s, a);
    HIP_TRY(hipGetLastError());
    // the same grid, reading each segment's count on the device: an empty worklist
    // costs a launch that exits at once, never a second pass over the frames
    hipLaunchKernelGGL(l4_cksum_kernel, dim3(grid), dim3(L4_BLOCK), 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int cndp_gpu_udp_input(cndp_gpu_ctx_t *ctx, cndp_pcb_tbl_t *tbl, const struct cndp_batch *b,
                                  const struct cndp_l4_io *io, void *stream)
{
    if (!ctx || !tbl || !b || !io)
        return -EINVAL;
    if (b->n && (!b->slab || !b->nh || !b->rxmeta || !io->l4edge || (!io->sel && !b->ptype)))
        return -EINVAL;
    const int dev = cndp_gpu_device(ctx);
    HIP_TRY(hipSetDevice(dev));
    pthread_mutex_lock(&tbl->lock);
    int r = 0;
    if (io->bin_of && (io->n_bins < tbl->count || io->n_bins > 65533u))
        r = -EINVAL;
    L4Dev *d = NULL;
    if (!r)
        r = l4_begin_locked(tbl, dev, (hipStream_t)stream, &d);
    if (!r) {
        if (b->n)
            r = l4_run(d, tbl, b, io, (hipStream_t)stream);
        const int e = l4_end_locked(tbl, (hipStream_t)stream, b->n && !r);
        r = r ? r : e;
    }
    pthread_mutex_unlock(&tbl->lock);
    return r;
}

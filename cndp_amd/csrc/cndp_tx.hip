// cndp_tx.hip -- udp_output + ip4_output on MI355X (include/cndp_tx.h).
//
// Four kernels per call, no host round trip between them.  Block b of the first
// and third owns the frames [b * chunk, (b + 1) * chunk), chunk a multiple of
// TX_BLOCK, one frame per lane and TX_BLOCK frames per pass:
//   tx_resolve_kernel  the PCB word (the table's transmit image, staged in LDS),
//                      the headroom tests and the route lookup on the source
//                      address: how far the frame gets and on which netif, kept
//                      as two bytes per frame; the block's sum per netif of what
//                      its frames add to ip_ident.
//   tx_scan_kernel     one thread per netif walks the blocks in order: every
//                      block's sums become the counters at its first frame, the
//                      totals go back to the table's counters.
//   tx_write_kernel    per pass a segmented exclusive sum keyed by netif: lanes
//                      of a wave compare keys lane by lane (readlane), waves hand
//                      their per-netif totals on through LDS, passes through a
//                      running LDS counter -- additions only, in index order, no
//                      atomic decides a value.  Then the headers: all 42 (34)
//                      bytes are built in registers, the IPv4 checksum summed
//                      from them, shifted once to the address's alignment and
//                      stored as aligned dwords, with byte stores at the ends and
//                      around the bytes the reference leaves alone.  The ARP
//                      lookup on the destination; edge, bin, counters.  A frame
//                      that needs an L4 checksum is appended to the block's
//                      worklist segment with its byte offset, length and folded
//                      pseudo-header sum.
//   tx_cksum_kernel    TX_CK_SPLIT blocks read write block b's segment: 16 lanes per
//                      datagram, 16-byte aligned loads with the head and tail
//                      masked, even / odd byte sums, the reference's folds, the
//                      complement, 0 -> 0xFFFF for UDP, the two bytes stored.
// Every frame read and write is bounded by slab_len.
//
// The FIB views and the byte-sum loop are those of cndp_fwd.hip / cndp_tcp.hip,
// kept as copies so those translation units stay as they are.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "tx_internal.h"

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            fprintf(stderr, "cndp_tx: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),    \
                    __FILE__, __LINE__);                                                         \
            return e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? -ENODEV : -EIO;       \
        }                                                                                        \
    } while (0)

// 256-lane blocks, three a CU: 12 waves a CU at the write kernel's 105 VGPRs
// (16 would fit) and 23 KiB of LDS a block.  More blocks would mean more rows
// for the scan to walk; the checksum kernel, which has no order to keep, splits
// each block's worklist segment over TX_CK_SPLIT blocks of its own instead.
#define TX_BLOCK 256u
#define TX_BLOCKS_PER_CU 3u
#define TX_WAVES (TX_BLOCK / 64u)
#define TX_CK_SPLIT 8u
#define TX_SCAN_BATCH 16u

// how far a frame gets is the high byte of its state (TXS_*, tx_internal.h); the low byte is the netif

#define TXWL_UDP 0x100u  // in an entry's fourth word: a computed 0 goes out as 0xFFFF
#define TXWL_ZERO 0x200u // total_length < 20: __ipv4_udptcp_cksum returns 0

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// one FIB's device mirror: the /16 directory in front of tbl24 when it has one
struct FibDev {
    const uint32_t *t24, *t8, *d16, *pages;
};

struct TxArgs {
    uint8_t *slab;
    uint64_t slab_len;
    uint64_t stride;
    const uint64_t *offsets;
    uint32_t data_off;
    uint32_t n;
    uint32_t mode;
    const uint8_t *sel;
    const uint32_t *pcb, *faddr, *laddr, *ports;
    const uint16_t *len;
    uint16_t *tx_edge;
    uint16_t *bin_of;
    uint32_t n_bins;
    unsigned long long *stats;
    const uint32_t *ximg; // device mirror of the PCB table's transmit image (tx_internal.h)
    const uint32_t *img;  // device mirror of the forwarding table's object image (fwd_internal.h)
    FibDev arp, rt;
    uint16_t *state; // per frame: TXS_* << 8 | netif
    uint32_t *bsum;  // [grid][256]: a block's sums, then the counters at its first frame
    uint16_t *ident; // [256]: the table's counters
    // worklist of the datagrams to checksum: one segment of `chunk` entries per
    // write block, its length in wl_cnt[block].  An entry is { L4 byte offset
    // low, high, bytes to sum | folded pseudo-header sum << 16, the checksum
    // field's offset from the L4 start | TXWL_* }, offset and bytes cut to the slab.
    u32x4 *wl;
    uint32_t *wl_cnt;
    uint32_t chunk; // frames per block, a multiple of TX_BLOCK
    uint32_t grid;
};

__device__ __forceinline__ uint32_t bswap16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

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

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        v += __shfl_xor(v, s, 64);
    return v;
}

__device__ __forceinline__ uint32_t reduce16(uint32_t s) // __cne_raw_cksum_reduce
{
    s = (s >> 16) + (s & 0xffffu);
    s = (s >> 16) + (s & 0xffffu);
    return s & 0xffffu;
}

// what the frame adds to its netif's ip_ident: total_length as a little-endian host loads it
__device__ __forceinline__ uint32_t ident_step(const TxArgs &a, uint32_t len)
{
    return bswap16((len + (a.mode == CNDP_TX_UDP ? 28u : 20u)) & 0xffffu);
}

__device__ __forceinline__ void stage_pcb(const TxArgs &a, uint32_t *s_pcb, uint32_t count)
{
    for (uint32_t k = threadIdx.x; k < count; k += TX_BLOCK)
        s_pcb[k] = a.ximg[TXI_HDR + k];
}

__global__ __launch_bounds__(TX_BLOCK) void tx_resolve_kernel(TxArgs a)
{
    __shared__ uint32_t s_pcb[CNDP_PCB_MAX_ENTRIES];
    __shared__ uint32_t s_sum[CNDP_FWD_NETIFS];
    const uint32_t t = threadIdx.x;
    uint32_t count = a.ximg[0];
    count = count > CNDP_PCB_MAX_ENTRIES ? CNDP_PCB_MAX_ENTRIES : count;
    stage_pcb(a, s_pcb, count);
    if (t < CNDP_FWD_NETIFS)
        s_sum[t] = 0;
    __syncthreads();
    const uint32_t rt_cap = a.img[1];
    const uint32_t *const rt = a.img + FWD_IMG_HDR + 2u * (size_t)a.img[0];
    const uint64_t beg = (uint64_t)blockIdx.x * a.chunk;
    const uint64_t end = beg + a.chunk < a.n ? beg + a.chunk : a.n;
    for (uint64_t i = beg + t; i < end; i += TX_BLOCK) {
        uint32_t st = TXS_NONE, nif = 0;
        uint32_t w = 0;
        if (!a.sel || a.sel[i]) {
            const uint32_t p = a.pcb[i];
            if (p < count) // CNDP_PCB_NONE is above every count
                w = s_pcb[p];
        }
        if (w & TXW_LIVE) {
            uint32_t h = a.data_off;
            if (a.mode == CNDP_TX_UDP && h < 8u)
                st = TXS_DROP_NOUDP;
            else {
                if (a.mode == CNDP_TX_UDP)
                    h -= 8u;
                if (h < 20u)
                    st = TXS_DROP_UDP;
                else {
                    h -= 20u;
                    const uint32_t ri = fib_lookup(a.rt, __builtin_bswap32(a.laddr[i])) & 0xffffffu;
                    uint32_t rw = 0;
                    if (ri < rt_cap)
                        rw = rt[2u * (size_t)ri + 1u];
                    if (!(rw & FWD_SET))
                        st = TXS_DROP_NOROUTE;
                    else if (h < 14u)
                        st = TXS_DROP_IP;
                    else {
                        st = TXS_OUT;
                        nif = rw & 0xffu;
                        atomicAdd(&s_sum[nif], ident_step(a, a.len[i])); // a sum: the order adds nothing
                    }
                }
            }
        }
        a.state[i] = (uint16_t)(st << 8 | nif);
    }
    __syncthreads();
    if (t < CNDP_FWD_NETIFS)
        a.bsum[(size_t)blockIdx.x * CNDP_FWD_NETIFS + t] = s_sum[t];
}

__global__ __launch_bounds__(CNDP_FWD_NETIFS) void tx_scan_kernel(TxArgs a)
{
    const uint32_t k = threadIdx.x;
    uint32_t run = a.ident[k];
    // a batch of rows loaded at once: the loads of a batch do not wait for each other
    for (uint32_t b0 = 0; b0 < a.grid; b0 += TX_SCAN_BATCH) {
        uint32_t v[TX_SCAN_BATCH];
#pragma unroll
        for (uint32_t j = 0; j < TX_SCAN_BATCH; j++)
            v[j] = b0 + j < a.grid ? a.bsum[(size_t)(b0 + j) * CNDP_FWD_NETIFS + k] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < TX_SCAN_BATCH; j++) {
            if (b0 + j < a.grid)
                a.bsum[(size_t)(b0 + j) * CNDP_FWD_NETIFS + k] = run;
            run += v[j];
        }
    }
    a.ident[k] = (uint16_t)run;
}

// Bytes [s, e) of the 44-byte image W, except [hs, he), to slab offsets o0 + index
// (o0 may lie "before" the slab as a wrapped value when the image's first bytes
// are not stored).  The image is shifted once to the alignment of its address;
// an aligned dword that lies wholly inside the bytes to store and inside the
// slab is one dword store, any other one goes byte by byte.
__device__ __forceinline__ void st_image(uint8_t *slab, uint64_t len, uint64_t o0, const uint32_t (&W)[11],
                                         int s, int e, int hs, int he)
{
    const uint32_t sh = (uint32_t)(((uintptr_t)slab + o0) & 3u);
    uint32_t V[12];
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const uint32_t lo = k > 0 ? W[k - 1] : 0u, hi = k < 11 ? W[k] : 0u;
        V[k] = sh ? __builtin_amdgcn_alignbyte(hi, lo, 4u - sh) : hi;
    }
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const int i0 = 4 * k - (int)sh; // the image index of the dword's first byte
        if (i0 + 4 <= s || i0 >= e)
            continue;
        const uint64_t x = o0 + (uint64_t)(int64_t)i0;
        const bool whole = i0 >= s && i0 + 4 <= e && (i0 + 4 <= hs || i0 >= he);
        if (whole && x < len && len - x >= 4u)
            *(uint32_t *)(slab + x) = V[k];
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int idx = i0 + j;
                const uint64_t xb = x + (uint64_t)j;
                if (idx >= s && idx < e && !(idx >= hs && idx < he) && xb < len)
                    slab[xb] = (uint8_t)(V[k] >> (8 * j));
            }
        }
    }
}

__global__ __launch_bounds__(TX_BLOCK) void tx_write_kernel(TxArgs a)
{
    __shared__ uint32_t s_pcb[CNDP_PCB_MAX_ENTRIES];
    __shared__ uint32_t s_run[CNDP_FWD_NETIFS];            // the counters at the pass's first frame
    __shared__ uint32_t s_wtot[TX_WAVES][CNDP_FWD_NETIFS]; // per wave of the pass: its frames' sum per netif
    __shared__ uint32_t s_mac[2u * CNDP_FWD_NETIFS];
    __shared__ uint32_t s_stat[CNDP_TX_NSTATS], s_wl;
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t count = a.ximg[0];
    count = count > CNDP_PCB_MAX_ENTRIES ? CNDP_PCB_MAX_ENTRIES : count;
    stage_pcb(a, s_pcb, count);
    const uint32_t arp_cap = a.img[0], rt_cap = a.img[1];
    const uint32_t *const arp = a.img + FWD_IMG_HDR;
    const uint32_t *const nifs = arp + 2u * (size_t)arp_cap + 2u * (size_t)rt_cap;
    for (uint32_t k = t; k < 2u * CNDP_FWD_NETIFS; k += TX_BLOCK)
        s_mac[k] = nifs[k];
    for (uint32_t k = t; k < TX_WAVES * CNDP_FWD_NETIFS; k += TX_BLOCK)
        (&s_wtot[0][0])[k] = 0;
    if (t < CNDP_FWD_NETIFS)
        s_run[t] = a.bsum[(size_t)blockIdx.x * CNDP_FWD_NETIFS + t];
    if (t < CNDP_TX_NSTATS)
        s_stat[t] = 0;
    if (t == 0)
        s_wl = 0;
    __syncthreads();
    u32x4 *const wl = a.wl + (size_t)blockIdx.x * a.chunk;
    const bool udp_mode = a.mode == CNDP_TX_UDP;
    const int img_end = udp_mode ? 42 : 34;
    uint32_t cnt[CNDP_TX_NSTATS] = {0, 0, 0, 0, 0, 0};
    const uint64_t beg = (uint64_t)blockIdx.x * a.chunk;
    const uint64_t end = beg + a.chunk < a.n ? beg + a.chunk : a.n;
    for (uint64_t base_i = beg; base_i < end; base_i += TX_BLOCK) {
        const uint64_t i = base_i + t;
        const bool live = i < end;
        uint32_t st = TXS_NONE, nif = 0, len = 0;
        if (live) {
            const uint32_t sw = a.state[i];
            st = sw >> 8;
            nif = sw & 0xffu;
            if (st != TXS_NONE)
                len = a.len[i];
        }
        // ---- packet_id: the netif's counter plus every earlier frame's step
        const uint32_t key = st == TXS_OUT ? nif : 0xffffffffu;
        const uint32_t step = st == TXS_OUT ? ident_step(a, len) : 0u;
        uint32_t pre = 0;
        bool last = true; // no later lane of the wave has this netif
#pragma unroll
        for (int j = 0; j < 64; j++) {
            const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, j);
            const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)step, j);
            if (kj == key) {
                if ((uint32_t)j < lane)
                    pre += sj;
                if ((uint32_t)j > lane)
                    last = false;
            }
        }
        if (st == TXS_OUT && last)
            s_wtot[wv][nif] = pre + step;
        __syncthreads();
        uint32_t id = 0;
        if (st == TXS_OUT) {
            id = s_run[nif] + pre;
            for (uint32_t w = 0; w < wv; w++)
                id += s_wtot[w][nif];
            id &= 0xffffu;
        }
        __syncthreads();
        if (t < CNDP_FWD_NETIFS) {
            uint32_t tot = 0;
#pragma unroll
            for (uint32_t w = 0; w < TX_WAVES; w++) {
                tot += s_wtot[w][t];
                s_wtot[w][t] = 0;
            }
            s_run[t] += tot;
        }
        __syncthreads(); // the next pass writes s_wtot before its first barrier

        // ---- the headers
        uint32_t edge = CNDP_TX_EDGE_NONE, bin = a.n_bins + 1u;
        bool need = false;
        u32x4 ent = {0u, 0u, 0u, 0u};
        if (st != TXS_NONE) {
            edge = CNDP_TX_EDGE_PKT_DROP;
            const uint32_t p = a.pcb[i]; // the resolve kernel saw this index inside the image
            const uint32_t w = p < count ? s_pcb[p] : 0u;
            const uint32_t proto = w & 0xffu;
            const uint32_t src = a.laddr[i], dst = a.faddr[i];
            const uint64_t fb = a.offsets ? a.offsets[i] : i * a.stride;
            // image index 0 is where the Ethernet header starts (or would)
            const uint64_t o0 = fb + a.data_off - (uint64_t)img_end;
            const uint32_t udp_len = (len + 8u) & 0xffffu;
            const uint32_t total = (len + (udp_mode ? 28u : 20u)) & 0xffffu;
            uint32_t U0 = 0, U1 = 0;
            if (udp_mode) {
                const uint32_t pp = a.ports[i];
                U0 = pp >> 16 | pp << 16; // src_port = lport, dst_port = fport
                U1 = bswap16(udp_len);    // dgram_len, dgram_cksum = 0
            }
            const uint32_t I0 = 0x45u | ((w >> 16) & 0xffu) << 8 | bswap16(total) << 16;
            const uint32_t I1 = bswap16(id); // packet_id, fragment_offset = 0
            uint32_t I2 = ((w >> 8) & 0xffu) | proto << 8;
            int s0 = 0, e0 = 0, hs = 0, he = 0;
            uint32_t d0 = 0, d1 = 0; // d_addr
            if (st == TXS_DROP_NOUDP)
                cnt[CNDP_TX_STAT_DROP_HEADROOM]++;
            else if (st == TXS_DROP_UDP) {
                cnt[CNDP_TX_STAT_DROP_HEADROOM]++;
                s0 = 34;
                e0 = img_end;
            } else if (st == TXS_DROP_NOROUTE || st == TXS_DROP_IP) {
                cnt[st == TXS_DROP_IP ? CNDP_TX_STAT_DROP_HEADROOM : CNDP_TX_STAT_DROP_NOROUTE]++;
                s0 = 14;
                e0 = img_end;
                hs = 18; // packet_id is not written before the route is known
                he = 20;
            } else {
                const uint32_t hsum = (I0 & 0xffffu) + (I0 >> 16) + I1 + I2 + (src & 0xffffu) + (src >> 16) +
                                      (dst & 0xffffu) + (dst >> 16);
                I2 |= (~reduce16(hsum) & 0xffffu) << 16;
                s0 = 6;
                e0 = img_end;
                const bool l4ck = proto == 17u ? (w & TXW_CKSUM) != 0 : proto == 6u;
                if (proto != 17u && proto != 6u)
                    cnt[CNDP_TX_STAT_DROP_PROTO]++;
                else {
                    const uint32_t ai = fib_lookup(a.arp, __builtin_bswap32(dst)) & 0xffffffu;
                    uint32_t h0 = 0;
                    if (ai < arp_cap)
                        h0 = arp[2u * (size_t)ai];
                    if (h0 & FWD_SET) {
                        d0 = h0 & 0xffffu;
                        d1 = arp[2u * (size_t)ai + 1u];
                        s0 = 0;
                        edge = nif + CNDP_TX_EDGE_OUTPUT; // the route's netif, not the ARP entry's
                        bin = nif;
                        cnt[CNDP_TX_STAT_SENT]++;
                    } else {
                        edge = CNDP_TX_EDGE_ARP_REQUEST;
                        bin = a.n_bins;
                        cnt[CNDP_TX_STAT_ARP_REQUEST]++;
                    }
                    if (l4ck) {
                        need = true;
                        cnt[CNDP_TX_STAT_CKSUM]++;
                        uint64_t l4 = fb + a.data_off - (udp_mode ? 8u : 0u);
                        uint32_t flags = (proto == 17u ? 6u | TXWL_UDP : 16u), bytes = 0, ph = 0;
                        if (total < 20u)
                            flags |= TXWL_ZERO;
                        else {
                            const uint32_t l4_len = total - 20u;
                            ph = reduce16((src & 0xffffu) + (src >> 16) + (dst & 0xffffu) + (dst >> 16) +
                                          (proto << 8) + bswap16(l4_len));
                            bytes = l4_len;
                        }
                        if (l4 >= a.slab_len) { // nothing to read, nowhere to store
                            l4 = a.slab_len;
                            bytes = 0;
                        } else if (a.slab_len - l4 < bytes)
                            bytes = (uint32_t)(a.slab_len - l4);
                        ent.x = (uint32_t)l4;
                        ent.y = (uint32_t)(l4 >> 32);
                        ent.z = bytes | ph << 16;
                        ent.w = flags;
                    }
                }
            }
            if (e0 > s0) {
                const uint32_t m0 = s_mac[2u * nif], m1 = s_mac[2u * nif + 1u];
                uint32_t W[11];
                W[0] = d0 | d1 << 16;
                W[1] = d1 >> 16 | m0 << 16;
                W[2] = m0 >> 16 | m1 << 16;
                W[3] = 0x0008u | I0 << 16;
                W[4] = I0 >> 16 | I1 << 16;
                W[5] = I1 >> 16 | I2 << 16;
                W[6] = I2 >> 16 | src << 16;
                W[7] = src >> 16 | dst << 16;
                W[8] = dst >> 16 | U0 << 16;
                W[9] = U0 >> 16 | U1 << 16;
                W[10] = U1 >> 16;
                st_image(a.slab, a.slab_len, o0, W, s0, e0, hs, he);
            }
        }
        if (live) {
            a.tx_edge[i] = (uint16_t)edge;
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
            if (need) // at most one entry per frame of the block: < chunk
                wl[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = ent;
        }
    }
#pragma unroll
    for (int k = 0; k < CNDP_TX_NSTATS; k++) {
        const uint32_t s = wave_sum(cnt[k]);
        if (s && lane == 0)
            atomicAdd(&s_stat[k], s);
    }
    __syncthreads(); // also orders the block's s_wl updates
    if (a.stats && t < CNDP_TX_NSTATS && s_stat[t])
        atomicAdd(&a.stats[t], (unsigned long long)s_stat[t]);
    if (t == 0)
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

__global__ __launch_bounds__(TX_BLOCK) void tx_cksum_kernel(TxArgs a)
{
    // TX_CK_SPLIT blocks share the segment of one write block, its entries dealt round robin
    const uint32_t seg = blockIdx.x / TX_CK_SPLIT;
    const uint32_t total = a.wl_cnt[seg];
    const u32x4 *const wl = a.wl + (size_t)seg * a.chunk;
    const uint32_t gl = threadIdx.x & 15u; // lane within the 16-lane group
    const uint32_t grp = (blockIdx.x % TX_CK_SPLIT) * (TX_BLOCK / 16u) + (threadIdx.x >> 4);
    const uint32_t ngrp = TX_CK_SPLIT * (TX_BLOCK / 16u);
    const uint32_t wave_first = grp & ~3u; // the wave's four groups stay in step for the shuffles
    for (uint32_t k0 = wave_first; k0 < total; k0 += ngrp) {
        const uint32_t k = k0 + (grp & 3u);
        const bool valid = k < total;
        u32x4 e = {0u, 0u, 0u, 0u};
        uint32_t se = 0, so = 0; // sums of the bytes at even / odd addresses
        uintptr_t lo = 0;
        if (valid) {
            e = wl[k]; // the group's 16 lanes read one entry: a broadcast
            const uint64_t ub = (uint64_t)e.y << 32 | e.x;
            const uintptr_t P = (uintptr_t)a.slab, Pend = P + a.slab_len;
            lo = P + ub; // ub + bytes <= slab_len: the write kernel cut them
            const uintptr_t hi = lo + (e.z & 0xffffu);
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
            // cne_raw_cksum's reduce, + cne_ipv4_phdr_cksum (folded by the write
            // kernel), __ipv4_udptcp_cksum's fold, cne_ipv4_udptcp_cksum's complement
            uint32_t c = reduce16(S) + (e.z >> 16);
            c = ((c >> 16) + (c & 0xffffu)) & 0xffffu;
            if (e.w & TXWL_ZERO)
                c = 0;
            c = ~c & 0xffffu;
            if (c == 0 && (e.w & TXWL_UDP))
                c = 0xffffu;
            const uint64_t ub = (uint64_t)e.y << 32 | e.x;
            const uint64_t x = ub + (e.w & 0xffu);
            if (x < a.slab_len && a.slab_len - x >= 2u && (((uintptr_t)a.slab + x) & 1u) == 0)
                *(uint16_t *)(a.slab + x) = (uint16_t)c;
            else {
                if (x < a.slab_len)
                    a.slab[x] = (uint8_t)c;
                if (x + 1u < a.slab_len)
                    a.slab[x + 1u] = (uint8_t)(c >> 8);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host side: the two tables' device mirrors
// ---------------------------------------------------------------------------
struct TxFwdDev {
    int dev;
    int cus;
    uint32_t *img; // the forwarding table's object image, copied whole when it changed
    uint64_t gen;  // table generation mirrored (0 = none)
    uint16_t *ident; // two sets of counters: the current one is `cur`; a reader that leaves the new
    int cur;         // counters in the other one (TX_DEV_MOVED, the mbuf queue's kernels) swaps them
    int have_ident;
    uint16_t *state;
    uint64_t state_cap;
    uint32_t *bsum; // cus * TX_BLOCKS_PER_CU rows
    u32x4 *wl;
    uint64_t wl_cap;
    uint32_t *cnt;
    hipEvent_t ev; // end of the last call's kernels
    hipStream_t last;
    int have_last;
};

struct TxPcbDev {
    int dev;
    uint32_t *img; // TXI_WORDS(max) words
    uint64_t gen;
    hipEvent_t ev;
    hipStream_t last;
    int have_last;
};

static void tx_fwd_release(void *p)
{
    TxFwdDev *d = (TxFwdDev *)p;
    if (hipSetDevice(d->dev) == hipSuccess) {
        (void)hipDeviceSynchronize();
        void *bufs[] = {d->img, d->ident, d->state, d->bsum, d->wl, d->cnt};
        for (void *b : bufs)
            if (b)
                (void)hipFree(b);
        if (d->ev)
            (void)hipEventDestroy(d->ev);
    }
    free(d);
}

static void tx_pcb_release(void *p)
{
    TxPcbDev *d = (TxPcbDev *)p;
    if (hipSetDevice(d->dev) == hipSuccess) {
        (void)hipDeviceSynchronize();
        if (d->img)
            (void)hipFree(d->img);
        if (d->ev)
            (void)hipEventDestroy(d->ev);
    }
    free(d);
}

// lock held: wait for the table's last call and read the counters back
static int tx_ident_pull(struct cndp_fwd_tbl *t)
{
    TxFwdDev *d = (TxFwdDev *)t->xdev;
    if (!d || !d->have_ident)
        return 0;
    HIP_TRY(hipSetDevice(d->dev));
    if (d->have_last)
        HIP_TRY(hipEventSynchronize(d->ev));
    HIP_TRY(hipMemcpy(t->ident, d->ident + d->cur * CNDP_FWD_NETIFS, sizeof(t->ident), hipMemcpyDeviceToHost));
    t->ident_dev_new = 0;
    return 0;
}

static int tx_fwd_init(TxFwdDev *d)
{
    HIP_TRY(hipDeviceGetAttribute(&d->cus, hipDeviceAttributeMultiprocessorCount, d->dev));
    const size_t rows = (size_t)d->cus * TX_BLOCKS_PER_CU;
    HIP_TRY(hipMalloc((void **)&d->ident, 2u * CNDP_FWD_NETIFS * sizeof(uint16_t)));
    HIP_TRY(hipMalloc((void **)&d->bsum, rows * CNDP_FWD_NETIFS * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&d->cnt, rows * sizeof(uint32_t)));
    HIP_TRY(hipEventCreateWithFlags(&d->ev, hipEventDisableTiming));
    return 0;
}

static int tx_fwd_get(struct cndp_fwd_tbl *t, int dev, TxFwdDev **out)
{
    TxFwdDev *d = (TxFwdDev *)t->xdev;
    if (d && d->dev != dev)
        return -EINVAL; // one table, one device
    if (!d) {
        d = (TxFwdDev *)calloc(1, sizeof(*d));
        if (!d)
            return -ENOMEM;
        d->dev = dev;
        int r = tx_fwd_init(d);
        if (r) {
            tx_fwd_release(d);
            return r;
        }
        t->xdev = d;
        t->xdev_release = tx_fwd_release;
        t->xdev_ident_pull = tx_ident_pull;
    }
    *out = d;
    return 0;
}

static int tx_pcb_get(struct cndp_pcb_tbl *t, int dev, TxPcbDev **out)
{
    TxPcbDev *d = (TxPcbDev *)t->xdev;
    if (d && d->dev != dev)
        return -EINVAL;
    if (!d) {
        d = (TxPcbDev *)calloc(1, sizeof(*d));
        if (!d)
            return -ENOMEM;
        d->dev = dev;
        hipError_t e = hipMalloc((void **)&d->img, TXI_WORDS(t->max) * sizeof(uint32_t));
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&d->ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            tx_pcb_release(d);
            return -EIO;
        }
        t->xdev = d;
        t->xdev_release = tx_pcb_release;
    }
    *out = d;
    return 0;
}

// Sync a FIB's mirror on `s` and take a view of its buffers: read under dev_lock
// with `views` held until the launches are enqueued, so a sync on another thread
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

// the tables' images and counters as the host has them now, on the device
static int tx_mirror(TxFwdDev *fd, TxPcbDev *pd, struct cndp_fwd_tbl *ft, struct cndp_pcb_tbl *pt, hipStream_t s)
{
    int r = tx_pcb_image(pt);
    if (r)
        return r;
    bool copied = false;
    if (pd->gen != pt->ximg_gen) {
        HIP_TRY(hipMemcpyAsync(pd->img, pt->ximg, TXI_WORDS(pt->count) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        copied = true;
    }
    if (fd->gen != ft->gen) {
        if (!fd->img)
            HIP_TRY(hipMalloc((void **)&fd->img, ft->img_words * 4u));
        HIP_TRY(hipMemcpyAsync(fd->img, ft->img, ft->img_words * 4u, hipMemcpyHostToDevice, s));
        copied = true;
    }
    if (!fd->have_ident || ft->ident_host_new) {
        HIP_TRY(hipMemcpyAsync(fd->ident + fd->cur * CNDP_FWD_NETIFS, ft->ident, sizeof(ft->ident),
                               hipMemcpyHostToDevice, s));
        copied = true;
    }
    if (copied)
        HIP_TRY(hipStreamSynchronize(s)); // the host tables may change after we return
    pd->gen = pt->ximg_gen;
    fd->gen = ft->gen;
    fd->have_ident = 1;
    ft->ident_host_new = 0;
    return 0;
}

// the reader protocol of tx_internal.h, with both locks held
static int tx_begin_locked(TxFwdDev *fd, TxPcbDev *pd, struct cndp_fwd_tbl *ft, struct cndp_pcb_tbl *pt, hipStream_t s,
                           struct tx_dev_view *v)
{
    if (fd->have_last && fd->last != s)
        HIP_TRY(hipStreamWaitEvent(s, fd->ev, 0));
    if (pd->have_last && pd->last != s)
        HIP_TRY(hipStreamWaitEvent(s, pd->ev, 0));
    int r = tx_mirror(fd, pd, ft, pt, s);
    if (r)
        return r;
    FibDev arp, rt;
    struct cndp_tbl *ta = &ft->arp_fib->t, *tr = &ft->rt4_fib->t;
    r = fib_acquire(ta, s, &arp);
    if (r)
        return r;
    r = fib_acquire(tr, s, &rt);
    if (r) {
        fib_release(ta);
        return r;
    }
    v->ximg = pd->img;
    v->img = fd->img;
    v->arp = {arp.t24, arp.t8, arp.d16, arp.pages};
    v->rt = {rt.t24, rt.t8, rt.d16, rt.pages};
    v->ident_in = fd->ident + fd->cur * CNDP_FWD_NETIFS;
    v->ident_out = fd->ident + (fd->cur ^ 1) * CNDP_FWD_NETIFS;
    v->cus = fd->cus;
    return 0;
}

extern "C" int tx_dev_begin(struct cndp_fwd_tbl *ft, struct cndp_pcb_tbl *pt, int dev, void *stream,
                            struct tx_dev_view *v)
{
    pthread_mutex_lock(&ft->lock);
    pthread_mutex_lock(&pt->lock);
    TxFwdDev *fd = NULL;
    TxPcbDev *pd = NULL;
    int r = tx_fwd_get(ft, dev, &fd);
    if (!r)
        r = tx_pcb_get(pt, dev, &pd);
    if (!r)
        r = tx_begin_locked(fd, pd, ft, pt, (hipStream_t)stream, v);
    if (r) {
        pthread_mutex_unlock(&pt->lock);
        pthread_mutex_unlock(&ft->lock);
    }
    return r;
}

static int tx_end_locked(TxFwdDev *fd, TxPcbDev *pd, struct cndp_fwd_tbl *ft, hipStream_t s, int launched)
{
    if (launched == TX_DEV_NONE)
        return 0;
    if (launched == TX_DEV_MOVED)
        fd->cur ^= 1;
    ft->ident_dev_new = 1;
    fd->last = pd->last = s;
    fd->have_last = pd->have_last = 1;
    HIP_TRY(hipEventRecord(fd->ev, s));
    HIP_TRY(hipEventRecord(pd->ev, s));
    return 0;
}

extern "C" int tx_dev_end(struct cndp_fwd_tbl *ft, struct cndp_pcb_tbl *pt, void *stream, int launched)
{
    fib_release(&ft->rt4_fib->t);
    fib_release(&ft->arp_fib->t);
    const int r = tx_end_locked((TxFwdDev *)ft->xdev, (TxPcbDev *)pt->xdev, ft, (hipStream_t)stream, launched);
    pthread_mutex_unlock(&pt->lock);
    pthread_mutex_unlock(&ft->lock);
    return r;
}

extern "C" int tx_dev_check(struct cndp_fwd_tbl *ft, struct cndp_pcb_tbl *pt, int dev)
{
    pthread_mutex_lock(&ft->lock);
    pthread_mutex_lock(&pt->lock);
    const TxFwdDev *fd = (const TxFwdDev *)ft->xdev;
    const TxPcbDev *pd = (const TxPcbDev *)pt->xdev;
    const int r = (fd && fd->dev != dev) || (pd && pd->dev != dev) ? -EINVAL : 0;
    pthread_mutex_unlock(&pt->lock);
    pthread_mutex_unlock(&ft->lock);
    return r;
}

// between tx_dev_begin and tx_dev_end: *launched says whether the kernels were enqueued
static int tx_run(TxFwdDev *fd, const struct tx_dev_view *v, const struct cndp_batch *b, uint32_t mode,
                  const struct cndp_tx_io *io, hipStream_t s, int *launched)
{
    *launched = TX_DEV_NONE;
    if (b->n == 0)
        return 0;
    // blocks own contiguous runs of whole passes
    const uint64_t passes = ((uint64_t)b->n + TX_BLOCK - 1u) / TX_BLOCK;
    const uint64_t cap = (uint64_t)fd->cus * TX_BLOCKS_PER_CU;
    const uint64_t per = (passes + cap - 1u) / cap;
    const uint32_t grid = (uint32_t)((passes + per - 1u) / per); // <= cap, no empty block
    const uint64_t chunk = per * TX_BLOCK;                       // <= n rounded up: < 2^32 + TX_BLOCK
    if (chunk > 0xffffffffull)
        return -EINVAL;
    if (fd->state_cap < b->n) {
        if (fd->state)
            HIP_TRY(hipFree(fd->state)); // waits for the kernels still using it
        fd->state = NULL;
        fd->state_cap = 0;
        HIP_TRY(hipMalloc((void **)&fd->state, (size_t)b->n * sizeof(uint16_t)));
        fd->state_cap = b->n;
    }
    if (fd->wl_cap < (uint64_t)grid * chunk) {
        if (fd->wl)
            HIP_TRY(hipFree(fd->wl));
        fd->wl = NULL;
        fd->wl_cap = 0;
        HIP_TRY(hipMalloc((void **)&fd->wl, (size_t)grid * chunk * sizeof(u32x4)));
        fd->wl_cap = (uint64_t)grid * chunk;
    }
    TxArgs a;
    a.slab = (uint8_t *)b->slab;
    a.slab_len = b->slab_len;
    a.stride = b->stride;
    a.offsets = b->offsets;
    a.data_off = b->data_off;
    a.n = b->n;
    a.mode = mode;
    a.sel = io->sel;
    a.pcb = io->pcb;
    a.faddr = io->faddr;
    a.laddr = io->laddr;
    a.ports = io->ports;
    a.len = io->len;
    a.tx_edge = io->tx_edge;
    a.bin_of = io->bin_of;
    a.n_bins = io->n_bins;
    a.stats = (unsigned long long *)io->stats;
    a.ximg = v->ximg;
    a.img = v->img;
    a.arp = {v->arp.t24, v->arp.t8, v->arp.d16, v->arp.pages};
    a.rt = {v->rt.t24, v->rt.t8, v->rt.d16, v->rt.pages};
    a.state = fd->state;
    a.bsum = fd->bsum;
    a.ident = v->ident_in; // advanced in place
    a.wl = fd->wl;
    a.wl_cnt = fd->cnt;
    a.chunk = (uint32_t)chunk;
    a.grid = grid;

    hipLaunchKernelGGL(tx_resolve_kernel, dim3(grid), dim3(TX_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tx_scan_kernel, dim3(1), dim3(CNDP_FWD_NETIFS), 0, s, a);
    hipLaunchKernelGGL(tx_write_kernel, dim3(grid), dim3(TX_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tx_cksum_kernel, dim3(grid * TX_CK_SPLIT), dim3(TX_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fprintf(stderr, "cndp_tx: launch failed: %s\n", hipGetErrorString(e));
        return -EIO;
    }
    *launched = TX_DEV_INPLACE;
    return 0;
}

extern "C" int cndp_gpu_ip4_output(cndp_gpu_ctx_t *ctx, cndp_fwd_tbl_t *ft, cndp_pcb_tbl_t *pt,
                                   const struct cndp_batch *b, uint32_t mode, const struct cndp_tx_io *io,
                                   void *stream)
{
    if (!ctx || !ft || !pt || !b || !io || mode > CNDP_TX_IP4)
        return -EINVAL;
    if (b->n && (!b->slab || !io->pcb || !io->faddr || !io->laddr || !io->len || !io->tx_edge ||
                 (mode == CNDP_TX_UDP && !io->ports) || (b->slab_len >> 63)))
        return -EINVAL;
    const int dev = cndp_gpu_device(ctx);
    HIP_TRY(hipSetDevice(dev));
    if (io->bin_of) {
        pthread_mutex_lock(&ft->lock);
        const bool bad = (int64_t)io->n_bins <= (int64_t)fwd_max_netif(ft) || io->n_bins > 65533u;
        pthread_mutex_unlock(&ft->lock);
        if (bad)
            return -EINVAL;
    }
    struct tx_dev_view v;
    int r = tx_dev_begin(ft, pt, dev, stream, &v);
    if (r)
        return r;
    int launched = TX_DEV_NONE;
    r = tx_run((TxFwdDev *)ft->xdev, &v, b, mode, io, (hipStream_t)stream, &launched);
    const int r2 = tx_dev_end(ft, pt, stream, launched);
    return r ? r : r2;
}

// cndp_acl.hip -- cndpfwd's ACL forwarding mode on MI355X (include/cndp_acl.h):
// validate_ipv4_pkt, the classify, the permit / deny decision, the destination
// port and MAC_SWAP of acl_fwd_test, one frame per lane.
//
// One kernel per call:
//   acl_fwd_kernel  A lane reads what the rule looks at and nothing else: frame
//                   bytes 5, 14-17 and 26-33.  A frame that starts on a 16-byte
//                   boundary (packed slots, the UMEM stride) is read as two
//                   16-byte loads and a dword, one on a 4-byte boundary as six
//                   dwords, any other by bounded byte loads.
//                   The image (acl_internal.h) is a tuple space: one descriptor
//                   per (src_msk, dst_msk) pair in use, ascending by the lowest
//                   rule index of the group.  The group loop runs on a
//                   wave-uniform counter, so the descriptor's words are scalar
//                   loads; the image pointer is a restrict kernel argument so
//                   that the stores of the outputs do not stand in their way.
//                   A lane probes a group's hash table with 16-byte gathers
//                   into the image, which stays L2-resident (the default set is
//                   266 KiB, 100000 /32:/32 rules 4 MiB); a lane stops when its
//                   best match lies below the next group's lowest index, the
//                   loop when every lane of the wave has.  The groups are taken
//                   four at a time, their first slots fetched together: the
//                   default set is 4 groups, so a frame waits for one round of
//                   gathers away from a collision.
//                   The image is not staged in LDS: the default set's is already
//                   larger than a CU's 160 KiB.
//                   Outputs leave as coalesced stores of one element per lane.
//                   A forwarded frame's MACs are swapped as k_mac_swap does it:
//                   three dwords when the frame is 4-byte aligned, else bytes.
//                   Counters: a ballot per verdict per wave, an LDS add per
//                   wave, one global add per block and counter.
// Every frame read is bounded by slab_len; no load or store leaves the slab.
//
// The image's device mirror is one buffer, overwritten in place by a rebuild and
// guarded by an event.  Every reader -- cndp_gpu_acl_fwd here, the mbuf queue's
// CNDP_MQ_ACL_FWD kernel in cndp_gpu.hip -- brackets its launch with
// acl_dev_begin / acl_dev_end (acl_internal.h).
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "acl_internal.h"

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            fprintf(stderr, "cndp_acl: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),   \
                    __FILE__, __LINE__);                                                         \
            return e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? -ENODEV : -EIO;       \
        }                                                                                        \
    } while (0)

#define ACL_BLOCK 256u
#define ACL_BLOCKS_PER_CU 8u
#define ACL_AHEAD 4u // groups whose first slot is in flight at once

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct AclArgs {
    uint8_t *slab;
    uint64_t slab_len;
    uint64_t stride;
    const uint64_t *offsets;
    uint32_t data_off;
    uint32_t n;
    const uint8_t *sel;
    const uint16_t *len;
    uint32_t *result;
    uint8_t *verdict;
    uint8_t *tx_lport;
    uint16_t *bin_of;
    unsigned long long *stats;
    uint64_t m0, m1, m2, m3; // lport_mask
    uint32_t in_lport;
    uint32_t n_bins;
    uint32_t mode;
    uint32_t swap;
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

// Of the frame at slab offset at: byte 5, and bytes 14-17, 26-29 and 30-33 as
// little-endian loads would give them.
__device__ __forceinline__ void rd_fields(const uint8_t *s, uint64_t len, uint64_t at, uint32_t &dmac5, uint32_t &w0,
                                          uint32_t &src, uint32_t &dst)
{
    const uintptr_t p = (uintptr_t)s + at;
    if (at < len && len - at >= 36u && !(p & 3u)) { // bytes at .. at + 35 lie inside the slab
        uint32_t d1, d3, d4, d6, d7, d8;
        if (!(p & 15u)) {
            const u32x4 a = *(const u32x4 *)p, b = *(const u32x4 *)(p + 16u);
            d1 = a.y, d3 = a.w, d4 = b.x, d6 = b.z, d7 = b.w;
            d8 = *(const uint32_t *)(p + 32u);
        } else {
            const uint32_t *q = (const uint32_t *)p;
            d1 = q[1], d3 = q[3], d4 = q[4], d6 = q[6], d7 = q[7], d8 = q[8];
        }
        dmac5 = (d1 >> 8) & 0xffu;
        w0 = __builtin_amdgcn_alignbyte(d4, d3, 2);
        src = __builtin_amdgcn_alignbyte(d7, d6, 2);
        dst = __builtin_amdgcn_alignbyte(d8, d7, 2);
    } else {
        dmac5 = rd_byte(s, len, at, 5);
        w0 = rd_le32(s, len, at, 14);
        src = rd_le32(s, len, at, 26);
        dst = rd_le32(s, len, at, 30);
    }
}

__global__ __launch_bounds__(ACL_BLOCK) void acl_fwd_kernel(AclArgs a, const uint32_t *__restrict__ img)
{
    __shared__ uint32_t s_stat[CNDP_ACL_NSTATS];
    if (threadIdx.x < CNDP_ACL_NSTATS)
        s_stat[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ng = img[1];
    const uint64_t step = (uint64_t)gridDim.x * ACL_BLOCK;
    for (uint64_t base = (uint64_t)blockIdx.x * ACL_BLOCK; base < a.n; base += step) {
        const uint64_t i64 = base + threadIdx.x;
        const bool live = i64 < a.n;
        const uint32_t i = (uint32_t)i64;
        const bool taken = live && (!a.sel || a.sel[i] != 0);
        uint64_t at = 0;
        uint32_t dmac5 = 0, w0 = 0, src = 0, dst = 0;
        bool len_ok = true;
        if (taken) {
            at = (a.offsets ? a.offsets[i] : (uint64_t)i * a.stride) + a.data_off;
            if (a.len)
                len_ok = a.len[i] >= 20u;
            rd_fields(a.slab, a.slab_len, at, dmac5, w0, src, dst);
        }
        const bool act = taken && !acl_prefilter(w0, len_ok);
        src = __builtin_bswap32(src);
        dst = __builtin_bswap32(dst);
        uint32_t best = 0;
        // g0 and k are wave-uniform: the descriptors are read once per wave.  The first slots of
        // ACL_AHEAD groups are fetched before any of them is looked at, so a frame that walks
        // four groups waits for one round of gathers, not four; the best match is a minimum
        // over the groups, so fetching a group that the early stop would have skipped changes
        // nothing but traffic.
        for (uint32_t g0 = 0; g0 < ng; g0 += ACL_AHEAD) {
            const uint32_t *d0 = img + ACL_HDR_WORDS + g0 * ACL_DESC_WORDS;
            const bool go = act && !acl_done(d0, best);
            if (!__ballot(go))
                break; // no lane of the wave can still improve: the groups ascend
            uint32_t h[ACL_AHEAD], s0[ACL_AHEAD], s1[ACL_AHEAD], v[ACL_AHEAD];
#pragma unroll
            for (uint32_t k = 0; k < ACL_AHEAD; k++) {
                // Every lane loads, whatever `go` says, and a k past the last group repeats the
                // last one: a load under a condition would be waited for on its own.  Any h
                // gives a slot inside the group's table.
                const uint32_t *d = img + ACL_HDR_WORDS + (g0 + k < ng ? g0 + k : ng - 1u) * ACL_DESC_WORDS;
                h[k] = acl_hash(src & d[0], dst & d[1]);
                acl_slot(img, d, h[k], &s0[k], &s1[k], &v[k]);
            }
#pragma unroll
            for (uint32_t k = 0; k < ACL_AHEAD; k++) {
                // selects, not branches, around what the first slots gave: a slot used only
                // under a condition would have its load moved there, behind the wait
                const uint32_t *d = img + ACL_HDR_WORDS + (g0 + k < ng ? g0 + k : ng - 1u) * ACL_DESC_WORDS;
                const uint32_t ks = src & d[0], kd = dst & d[1];
                const bool on = g0 + k < ng && go && !acl_done(d, best);
                const bool hit = !v[k] || (s0[k] == ks && s1[k] == kd);
                uint32_t e = v[k];
                if (on && !hit) // another key sits in the first slot: walk on
                    e = acl_probe_on(img, d, ks, kd, h[k]);
                best = on ? acl_better(best, e) : best;
            }
        }
        const uint32_t res = act ? acl_userdata(best) : 0u;
        const uint32_t v = !taken ? CNDP_ACL_NONE : !act ? CNDP_ACL_PREFILTER : acl_decide(res, a.mode);
        uint32_t tx = CNDP_ACL_LPORT_NONE;
        if (v == CNDP_ACL_FORWARD) {
            tx = acl_tx_lport(dmac5, a.m0, a.m1, a.m2, a.m3, a.in_lport);
            // act => byte 14 was read inside the slab, so at + 12 <= slab_len; tested all the same
            if (a.swap && at < a.slab_len && a.slab_len - at >= 12u) {
                uint8_t *p = a.slab + at;
                if ((((uintptr_t)p) & 3u) == 0) {
                    uint32_t *q = (uint32_t *)p;
                    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
                    q[0] = __builtin_amdgcn_alignbyte(d2, d1, 2); // bytes 6..9
                    q[1] = (d2 >> 16) | (d0 << 16);               // bytes 10, 11, 0, 1
                    q[2] = __builtin_amdgcn_alignbyte(d1, d0, 2); // bytes 2..5
                } else {
                    for (int k = 0; k < 6; k++) {
                        const uint8_t t = p[k];
                        p[k] = p[6 + k];
                        p[6 + k] = t;
                    }
                }
            }
        }
        if (live) {
            if (a.result)
                a.result[i] = res;
            a.verdict[i] = (uint8_t)v;
            if (a.tx_lport)
                a.tx_lport[i] = (uint8_t)tx;
            if (a.bin_of)
                a.bin_of[i] = (uint16_t)(v == CNDP_ACL_FORWARD ? tx : v == CNDP_ACL_DENY ? a.n_bins : a.n_bins + 1u);
        }
#pragma unroll
        for (uint32_t k = 0; k < CNDP_ACL_NSTATS; k++) {
            const unsigned long long m = __ballot(v == k + 1u);
            if (m && lane == 0)
                atomicAdd(&s_stat[k], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    if (a.stats && threadIdx.x < CNDP_ACL_NSTATS && s_stat[threadIdx.x])
        atomicAdd(&a.stats[threadIdx.x], (unsigned long long)s_stat[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// host side: the image's device mirror
// ---------------------------------------------------------------------------
struct AclDev {
    int dev;
    int cus;
    uint32_t *img;    // room for cap_words, allocated on the first call
    size_t cap_words;
    uint64_t gen;     // table generation mirrored (0 = none)
    hipEvent_t ev;    // end of the last call's kernel
    hipStream_t last;
    int have_last;
};

static void acl_dev_release(void *p)
{
    AclDev *d = (AclDev *)p;
    if (hipSetDevice(d->dev) == hipSuccess) {
        (void)hipDeviceSynchronize();
        if (d->img)
            (void)hipFree(d->img);
        if (d->ev)
            (void)hipEventDestroy(d->ev);
    }
    free(d);
}

static int acl_dev_init(AclDev *d)
{
    HIP_TRY(hipDeviceGetAttribute(&d->cus, hipDeviceAttributeMultiprocessorCount, d->dev));
    HIP_TRY(hipEventCreateWithFlags(&d->ev, hipEventDisableTiming));
    return 0;
}

static int acl_dev_get(struct cndp_acl_tbl *t, int dev, AclDev **out)
{
    AclDev *d = (AclDev *)t->dev;
    if (d && d->dev != dev)
        return -EINVAL; // one table, one device
    if (!d) {
        d = (AclDev *)calloc(1, sizeof(*d));
        if (!d)
            return -ENOMEM;
        d->dev = dev;
        int r = acl_dev_init(d);
        if (r) {
            acl_dev_release(d);
            return r;
        }
        t->dev = d;
        t->dev_release = acl_dev_release;
    }
    *out = d;
    return 0;
}

static int acl_mirror(AclDev *d, struct cndp_acl_tbl *t, hipStream_t s)
{
    if (d->gen == t->gen)
        return 0;
    if (t->img_words > d->cap_words) {
        if (d->img) {
            HIP_TRY(hipDeviceSynchronize()); // a kernel of an earlier call may still read the old one
            HIP_TRY(hipFree(d->img));
            d->img = NULL;
            d->cap_words = 0;
            d->gen = 0;
        }
        HIP_TRY(hipMalloc((void **)&d->img, t->img_words * sizeof(uint32_t)));
        d->cap_words = t->img_words;
    }
    d->gen = 0; // until the copy has landed the mirror holds no generation
    HIP_TRY(hipMemcpyAsync(d->img, t->img, t->img_words * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s)); // the host image may be rebuilt after we return
    d->gen = t->gen;
    return 0;
}

// acl_dev_begin under t->lock: the device, the wait for a reader on another stream, the mirror
static int acl_begin_locked(struct cndp_acl_tbl *t, int dev, hipStream_t s, AclDev **out)
{
    if (!t->img)
        return -ENOENT;
    HIP_TRY(hipSetDevice(dev));
    AclDev *d = NULL;
    int r = acl_dev_get(t, dev, &d);
    if (r)
        return r;
    if (d->have_last && d->last != s)
        HIP_TRY(hipStreamWaitEvent(s, d->ev, 0));
    *out = d;
    return acl_mirror(d, t, s);
}

extern "C" int acl_dev_begin(struct cndp_acl_tbl *t, int dev, void *stream, const uint32_t **img, int *cus)
{
    pthread_mutex_lock(&t->lock);
    AclDev *d = NULL;
    const int r = acl_begin_locked(t, dev, (hipStream_t)stream, &d);
    if (r) {
        pthread_mutex_unlock(&t->lock);
        return r;
    }
    *img = d->img;
    if (cus)
        *cus = d->cus;
    return 0;
}

static int acl_end_locked(AclDev *d, hipStream_t s)
{
    HIP_TRY(hipEventRecord(d->ev, s));
    d->last = s;
    d->have_last = 1;
    return 0;
}

extern "C" int acl_dev_end(struct cndp_acl_tbl *t, void *stream, int launched)
{
    const int r = launched ? acl_end_locked((AclDev *)t->dev, (hipStream_t)stream) : 0;
    pthread_mutex_unlock(&t->lock);
    return r;
}

static int acl_launch(int cus, const uint32_t *img, const struct cndp_batch *b, uint32_t mode, uint32_t flags,
                      const struct cndp_acl_io *io, hipStream_t s)
{
    AclArgs a;
    a.slab = (uint8_t *)(uintptr_t)b->slab;
    a.slab_len = b->slab_len;
    a.stride = b->stride;
    a.offsets = b->offsets;
    a.data_off = b->data_off;
    a.n = b->n;
    a.sel = io->sel;
    a.len = io->len;
    a.result = io->result;
    a.verdict = io->verdict;
    a.tx_lport = io->tx_lport;
    a.bin_of = io->bin_of;
    a.stats = (unsigned long long *)io->stats;
    a.m0 = io->lport_mask[0];
    a.m1 = io->lport_mask[1];
    a.m2 = io->lport_mask[2];
    a.m3 = io->lport_mask[3];
    a.in_lport = io->in_lport;
    a.n_bins = io->n_bins;
    a.mode = mode;
    a.swap = flags & CNDP_ACL_F_MAC_SWAP;

    const uint64_t want = ((uint64_t)b->n + ACL_BLOCK - 1u) / ACL_BLOCK;
    const uint64_t cap = (uint64_t)cus * ACL_BLOCKS_PER_CU;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    hipLaunchKernelGGL(acl_fwd_kernel, dim3(grid), dim3(ACL_BLOCK), 0, s, a, img);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int cndp_gpu_acl_fwd(cndp_gpu_ctx_t *ctx, cndp_acl_tbl_t *t, const struct cndp_batch *b, uint32_t mode,
                                uint32_t flags, const struct cndp_acl_io *io, void *stream)
{
    if (!ctx || !t)
        return -EINVAL;
    int r = acl_io_check(b, mode, flags, io);
    if (r)
        return r;
    const uint32_t *img = NULL;
    int cus = 0;
    if ((r = acl_dev_begin(t, cndp_gpu_device(ctx), stream, &img, &cus)))
        return r;
    if (b->n)
        r = acl_launch(cus, img, b, mode, flags, io, (hipStream_t)stream);
    const int e = acl_dev_end(t, stream, b->n && !r);
    return r ? r : e;
}

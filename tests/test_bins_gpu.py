"""Bin counters and the stable partition away from n_bins = 64.

Every classify kernel keeps its own LDS counters, zeroed and flushed by loops
bounded by n_bins + 2; the speculation passes move counts between bins with
signed deltas; cndp_gpu_bin_partition keeps per-tile counters for up to
CNDP_PART_BINS_MAX + 2 bins.  Here they run at n_bins from 0 to their caps --
fewer bins than a wave, more than a block has threads, next hops past n_bins
(the overflow bin), counters that start non-zero -- against the oracle at the
same n_bins, and the partition runs on constructed inputs against numpy's
stable argsort.  No bin id passed anywhere is n_bins + 2 or more."""
import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd import pktgen
from oracle import oracle as O

from helpers import CNET_DEF, assert_same, cnet_fibs, l3fwd_fib, l3fwd_oracle_tables, oracle_classify
from test_gpu_parity import _cnet_edge, _gtp_mix, _rewrite_setup

pytestmark = pytest.mark.gpu

MODES = {"l3fwd": N.CNDP_MODE_L3FWD, "hash": N.CNDP_MODE_HASH, "cnet": N.CNDP_MODE_CNET}
OMODE = {N.CNDP_MODE_L3FWD: O.MODE_L3FWD, N.CNDP_MODE_HASH: O.MODE_HASH, N.CNDP_MODE_CNET: O.MODE_CNET}
CLS_NB = [0, 1, 7, 63, 65, 1023, 1024]
ALL = ("nh", "hash", "queue", "edge", "bins", "ptype")
ALL_CNET = ALL + ("rxmeta",)


# ---------------------------------------------------------------------------
# a. the partition on constructed inputs
# ---------------------------------------------------------------------------
PART_N = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4 * 1024 + 1, 70001]
PART_NB = [0, 1, 62, 63, 64, 1022, 1023, 1024, 1025, 4095, N.CNDP_PART_BINS_MAX]
GUARD, SENT = 16, 0x5A5A5A5A


def patterns(n, nb, seed):
    """{name: bin ids}, every id < nb + 2."""
    T = nb + 2
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    p = {f"const{v}": np.full(n, v, np.int64) for v in sorted({0, max(nb - 1, 0), nb, nb + 1})}
    p["mod"] = i % T                                       # 64 different bins a wave: 64 leader turns
    p["descending"] = (nb + 1) - i * T // max(n, 1)
    p["two_by_lane"] = np.where(i & 1, T - 1, nb // 2)
    p["uniform"] = rng.integers(0, T, n)
    p["heavy"] = np.where(rng.random(n) < 0.9, T // 3, rng.integers(0, T, n))
    p["extra_only"] = nb + rng.integers(0, 2, n)
    for b in p.values():
        assert b.shape == (n,) and (n == 0 or (0 <= b.min() and b.max() < T))
    return p


def partition_raw(cl, bt, n, nb, stream=None):
    """cndp_gpu_bin_partition into sentinel-filled arrays with guard words past
    their ends; returns the device tensors (no synchronisation)."""
    dev = bt.device
    start = torch.full((nb + 3 + GUARD,), SENT, dtype=torch.int32, device=dev)
    order = torch.full((n + GUARD,), SENT, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = cl._L.cndp_gpu_bin_partition(cl.h, bt.data_ptr() or None, n, nb, start.data_ptr(), order.data_ptr(),
                                      stream or None)
    assert rc == 0, f"cndp_gpu_bin_partition(n={n}, n_bins={nb}) returned {rc}"
    return start, order


def check_partition(b, nb, start, order, what=""):
    n = len(b)
    start, order = start.cpu().numpy().view(np.uint32), order.cpu().numpy().view(np.uint32)
    assert (start[nb + 3:] == SENT).all() and (order[n:] == SENT).all(), f"{what}: guard words written"
    counts = np.bincount(b, minlength=nb + 2)
    assert len(counts) == nb + 2
    assert np.array_equal(start[:nb + 3], np.concatenate([[0], np.cumsum(counts)])), f"{what}: bin_start"
    assert start[nb + 2] == n
    if n == 0:
        assert (order == SENT).all(), f"{what}: order written for an empty batch"
    else:
        assert np.array_equal(order[:n], np.argsort(b, kind="stable")), f"{what}: order"


def partition_case(cl, b, nb, dev, what=""):
    bt = torch.from_numpy(b.astype(np.uint16).view(np.int16)).to(dev)
    start, order = partition_raw(cl, bt, len(b), nb)
    torch.cuda.synchronize()
    check_partition(b, nb, start, order, what)


@pytest.fixture(scope="module")
def part(gpu):
    from cndp_amd.classify import Classifier
    cl = Classifier(0)
    yield cl
    cl.close()


@pytest.mark.parametrize("nb", PART_NB)
def test_partition_constructed(part, gpu, nb):
    """Every size around a wave, a 256-thread chunk and a 1024-frame tile (the
    scan carries across 1024-word chunks from nb + 2 = 1025 words on, and at
    70001 frames for every nb > 13), every pattern, against numpy."""
    for n in PART_N:
        for name, b in patterns(n, nb, seed=n + 7 * nb).items():
            partition_case(part, b, nb, gpu, f"n={n} n_bins={nb} {name}")


def test_partition_scratch_regrowth(gpu):
    """One context: the scratch grows from nothing, grows again, and is then
    reused by smaller calls."""
    from cndp_amd.classify import Classifier
    cl = Classifier(0)
    try:
        cap = N.CNDP_PART_BINS_MAX
        for k, (n, nb) in enumerate(((5003, 64), (70001, cap), (1, 0), (5003, 1024), (70001, cap))):
            pats = patterns(n, nb, seed=k)
            for name in ("uniform", "mod"):
                partition_case(cl, pats[name], nb, gpu, f"call {k}: n={n} n_bins={nb} {name}")
    finally:
        cl.close()


def test_partition_on_side_stream(part, gpu):
    """bin_of produced by torch ops on a non-default stream, the partition
    enqueued behind them on that stream with no synchronisation in between."""
    n, nb = 70001, 1024
    src = torch.from_numpy(np.random.default_rng(3).integers(0, 1 << 30, n)).to(gpu)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        start = torch.full((nb + 3 + GUARD,), SENT, dtype=torch.int32, device=gpu)
        order = torch.full((n + GUARD,), SENT, dtype=torch.int32, device=gpu)
        x = src
        for _ in range(40):                      # keep the stream busy past the host's call
            x = (x * 5 + 1) % (1 << 30)
        bt = (x % (nb + 2)).to(torch.int16)
        rc = part._L.cndp_gpu_bin_partition(part.h, bt.data_ptr(), n, nb, start.data_ptr(), order.data_ptr(),
                                            s.cuda_stream)
    assert rc == 0
    s.synchronize()
    x = src.cpu().numpy()
    for _ in range(40):
        x = (x * 5 + 1) % (1 << 30)
    check_partition(x % (nb + 2), nb, start, order, "side stream")
    torch.cuda.synchronize()


def test_partition_errors(part, gpu):
    L, h = part._L, part.h
    bt = torch.zeros(64, dtype=torch.int16, device=gpu)
    start = torch.zeros(N.CNDP_PART_BINS_MAX + 4, dtype=torch.int32, device=gpu)
    order = torch.zeros(64, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    EINVAL = -22
    assert L.cndp_gpu_bin_partition(h, bt.data_ptr(), 64, N.CNDP_PART_BINS_MAX + 1, start.data_ptr(),
                                    order.data_ptr(), None) == EINVAL
    assert L.cndp_gpu_bin_partition(h, bt.data_ptr(), 64, 64, None, order.data_ptr(), None) == EINVAL
    assert L.cndp_gpu_bin_partition(h, bt.data_ptr(), 64, 64, start.data_ptr(), None, None) == EINVAL
    assert L.cndp_gpu_bin_partition(h, None, 64, 64, start.data_ptr(), order.data_ptr(), None) == EINVAL
    assert L.cndp_gpu_bin_partition(h, None, 0, 64, start.data_ptr(), None, None) == 0     # n == 0 needs neither
    torch.cuda.synchronize()
    assert N.CNDP_PART_BINS_MAX >= N.CNDP_PCB_MAX_ENTRIES and N.CNDP_BINS_MAX == 1024


# ---------------------------------------------------------------------------
# b. classify counters against the oracle at the same n_bins
# ---------------------------------------------------------------------------
class Refs:
    """oracle_classify results, computed once per (frames, mode, n_bins)."""

    def __init__(self):
        self.memo = {}

    def __call__(self, name, fr, mode, nb, **kw):
        k = (name, mode, nb)
        if k not in self.memo:
            self.memo[k] = oracle_classify(OMODE[mode], fr, n_bins=nb, **kw)
        return self.memo[k]


L3_RETA = np.random.default_rng(12).integers(0, 1100, 512).astype(np.uint16)


@pytest.fixture(scope="module")
def l3(gpu):
    """l3fwd over 1024 next hops (every one of 1024 bins in use, and next hops
    past any smaller n_bins) and three batches of packed 64-B slots."""
    from cndp_amd.classify import Classifier
    routes = pktgen.l3fwd_routes(n_nh=1024)
    fib, vals = l3fwd_fib(routes)
    cl = Classifier(0)
    cl.set_fib(fib)
    frames = {"routed": pktgen.packed_ipv4(64 * 300 + 7, routes=routes, device=gpu, seed=31),
              "half": pktgen.packed_ipv4(64 * 300 + 7, routes=routes, device=gpu, seed=32, in_route_frac=0.5),
              "fuzz": pktgen.fuzz_frames(64 * 300 + 5, seed=33, slot=64, device=gpu)}
    yield cl, l3fwd_oracle_tables(vals), frames, Refs()
    cl.close()


@pytest.fixture(scope="module")
def l3_64(gpu):
    """l3fwd over the 64 next hops ip4_rewrite's table holds."""
    from cndp_amd.classify import Classifier
    fib, vals = l3fwd_fib()
    cl = Classifier(0)
    cl.set_fib(fib)
    yield cl, l3fwd_oracle_tables(vals)
    cl.close()


@pytest.fixture(scope="module")
def cnet(gpu):
    from cndp_amd.classify import Classifier
    fib, fib6, routes, v6, v4vals, v6vals = cnet_fibs()
    cl = Classifier(0)
    cl.set_fib(fib, fib6)
    t4 = O.dir24_8_build(v4vals, CNET_DEF, 256)
    t6 = O.trie_build(v6vals, CNET_DEF, 1 << 15)
    frames = {"imix": pktgen.imix(64 * 300 + 7, v4routes=routes, v6routes=v6, device=gpu, seed=5),
              "strided": pktgen.packed_ipv4(64 * 300 + 7, routes=routes, device=gpu, seed=6)}
    yield cl, routes, v6, t4, t6, frames, Refs()
    cl.close()


def run(cl, fr, mode, nb, bins=None, meta=True):
    if mode == N.CNDP_MODE_CNET:
        cl.set_tuning(cnet_spec=256)        # a fresh ptype-node state, like the oracle's
    out = cl.alloc_outputs(fr.n, nb, device=fr.slab.device, meta=meta)
    if bins is not None:
        out["bins"] = bins
    cl.classify(fr, mode, out=out)
    torch.cuda.synchronize()
    return out


def l3_variants():
    for bpc in (0, 1):
        for nt in (0, 1):
            yield dict(tile=0, nt=nt, blocks_per_cu=bpc)
        for bal in (0, 1, 2):
            for lnt in (0, 1):
                yield dict(tile=1, stream_bal=bal, load_nt=lnt, blocks_per_cu=bpc)


L3_DEFAULTS = dict(tile=1, nt=1, load_nt=1, stream_bal=0, blocks_per_cu=0)


def l3_ref(l3, mode, name, nb):
    cl, t4, frames, refs = l3
    kw = dict(reta=L3_RETA) if mode == N.CNDP_MODE_HASH else {}
    return refs(name, frames[name], mode, nb, tables4=t4, **kw)


@pytest.mark.parametrize("nb", CLS_NB)
@pytest.mark.parametrize("mode", ["l3fwd", "hash"])
def test_counters_l3fwd_hash(l3, gpu, mode, nb):
    """k_classify_fast and the wave-tile / streamed kernels, every schedule."""
    cl, t4, frames, refs = l3
    m = MODES[mode]
    ref = {name: l3_ref(l3, m, name, nb) for name in frames}
    # the inputs reach what they are here for
    bins = ref["routed"]["bins"]
    assert all(int(r["bins"].sum()) == frames[k].n for k, r in ref.items())
    if mode == "l3fwd":
        if nb == 1024:
            assert (bins[:1024] > 0).all()
        if nb <= 63:
            assert bins[nb + 1] > 0 and ref["half"]["bins"][nb] > 0 and ref["half"]["bins"][nb + 1] > 0
        assert ref["fuzz"]["bins"][nb] > 0              # pkt_cls's drops
    else:
        assert bins[nb + 1] > 0                       # queues up to 1099
        if nb == 1024:
            assert (bins[:1024] > 0).sum() > 200
    try:
        if mode == "hash":
            cl.set_rss(reta=L3_RETA)
        for v in l3_variants():
            cl.set_tuning(**{**L3_DEFAULTS, **v})
            for name, fr in frames.items():
                try:
                    assert_same(run(cl, fr, m, nb), ref[name], keys=ALL)
                except AssertionError as e:
                    raise AssertionError(f"{name} {v}: {e}") from None
    finally:
        cl.set_tuning(**L3_DEFAULTS)
        cl.set_rss()


@pytest.mark.parametrize("nb", CLS_NB)
def test_counters_cnet(cnet, gpu, nb):
    """k_cnet_general, k_cnet_defer and its tail: frames at offsets (IMIX) and
    at a stride, the static and the balanced schedule."""
    cl, routes, v6, t4, t6, frames, refs = cnet
    ref = {name: refs(name, fr, N.CNDP_MODE_CNET, nb, tables4=t4, tables6=t6) for name, fr in frames.items()}
    bins = ref["imix"]["bins"]
    assert int(bins.sum()) == frames["imix"].n and bins[nb] > 0 and bins[nb + 1] > 0
    if nb == 1024:
        assert (bins[:1024] > 0).sum() >= 1000
    try:
        for ct in (0, 1):
            for bal in (1, 2):
                cl.set_tuning(cnet_tile=ct, stream_bal=bal)
                for name, fr in frames.items():
                    try:
                        assert_same(run(cl, fr, N.CNDP_MODE_CNET, nb), ref[name], keys=ALL_CNET)
                    except AssertionError as e:
                        raise AssertionError(f"{name} cnet_tile={ct} stream_bal={bal}: {e}") from None
    finally:
        cl.set_tuning(cnet_tile=1, stream_bal=0, cnet_spec=256)


def _uniform_gtp(routes, gpu, seed):
    """test_cnet_speculation_uniform's batch: one low ptype byte, three edges."""
    fr = pktgen.packed_ipv4(30000, routes=routes, device=gpu, seed=seed)
    rows = fr.slab.view(fr.n, fr.stride)
    idx = torch.arange(fr.n, device=gpu)
    rows[:, 36] = 0x12
    for every, first, lo in ((997, 5, 0x68), (1499, 11, 0x4B)):   # 2152 GTP-U, 2123 GTP-C
        sel = (idx % every) == first
        rows[sel, 36] = 0x08
        rows[sel, 37] = lo
    return fr


@pytest.mark.parametrize("nb", [1, 65, 1024])
@pytest.mark.parametrize("burst", [256, 7])
def test_counters_speculation_uniform(cnet, gpu, burst, nb):
    """The speculation passes move counts between bins with signed deltas
    (k_spec_local's uniform pass over chained calls): the moved frames leave
    a next-hop bin, or the overflow bin, for an extra bin."""
    cl, routes, v6, t4, t6, _, _ = cnet
    fr = _uniform_gtp(routes, gpu, seed=burst + 7)
    pt = oracle_classify(O.MODE_CNET, fr, tables4=t4, tables6=t6, spec_burst=0)["ptype"] & 0xFFFF
    assert len({int(p) & 0xFF for p in pt}) == 1 and len({_cnet_edge(int(p)) for p in pt}) == 3
    cuts = (0, (fr.n // 3) // burst * burst, (2 * fr.n // 3) // burst * burst, fr.n)
    parts, st, moved = [], np.zeros(1, np.uint16), 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        p = pktgen.Frames(fr.slab[lo * fr.stride:hi * fr.stride], hi - lo, stride=fr.stride, data_off=fr.data_off)
        plain = oracle_classify(O.MODE_CNET, p, tables4=t4, tables6=t6, n_bins=nb, spec_burst=0)
        ref = oracle_classify(O.MODE_CNET, p, tables4=t4, tables6=t6, n_bins=nb, spec_burst=burst, spec_state=st)
        moved += int((plain["edge"] != ref["edge"]).sum())
        assert int(ref["bins"].sum()) == p.n
        parts.append((p, ref))
    assert moved > 0, "input does not exercise the quirk"
    try:
        for scan in (0, 1):
            cl.set_tuning(cnet_spec=burst, spec_scan=scan)      # also resets the node state
            acc = torch.zeros(nb + 2, dtype=torch.int64, device=gpu)
            for p, ref in parts:
                o = cl.alloc_outputs(p.n, nb, device=gpu, meta=True)
                cl.classify(p, N.CNDP_MODE_CNET, out=o)
                torch.cuda.synchronize()
                assert_same(o, ref, keys=ALL)
            cl.set_tuning(cnet_spec=burst, spec_scan=scan)      # the chain again, into one tensor
            for p, ref in parts:
                o = cl.alloc_outputs(p.n, nb, device=gpu)
                o["bins"] = acc
                cl.classify(p, N.CNDP_MODE_CNET, out=o)
            torch.cuda.synchronize()
            assert np.array_equal(acc.cpu().numpy().view(np.uint64), sum(r["bins"] for _, r in parts))
    finally:
        cl.set_tuning(cnet_spec=256, spec_scan=0)


@pytest.mark.parametrize("nb", [1, 65, 1024])
def test_counters_speculation_gtp_mix(cnet, gpu, nb):
    """A GTP mix with two single-type runs (test_cnet_speculation_local_and_full's
    batch): the local pass and the general resolution both move counts."""
    cl, routes, v6, t4, t6, _, _ = cnet
    fr = _gtp_mix(40000, routes, v6, gpu, seed=31)
    plain = oracle_classify(O.MODE_CNET, fr, tables4=t4, tables6=t6, n_bins=nb, spec_burst=0)
    pick = int(np.flatnonzero(plain["ptype"] == 0x0211)[0])
    off = fr.offsets.clone()
    for lo, hi in ((8192, 8192 + 3 * 1024), (20480, 20480 + 2 * 1024 + 100)):
        off[lo:hi] = off[pick]
    fr = pktgen.Frames(fr.slab, fr.n, offsets=off)
    plain = oracle_classify(O.MODE_CNET, fr, tables4=t4, tables6=t6, n_bins=nb, spec_burst=0)
    ref = oracle_classify(O.MODE_CNET, fr, tables4=t4, tables6=t6, n_bins=nb, spec_burst=256)
    assert (plain["edge"] != ref["edge"]).sum() > 0, "input does not exercise the quirk"
    assert not np.array_equal(plain["bins"], ref["bins"]), "no count moves between bins"
    try:
        for scan in (0, 1, 2):
            cl.set_tuning(cnet_spec=256, spec_scan=scan)
            out = cl.alloc_outputs(fr.n, nb, device=gpu, meta=True)
            cl.classify(fr, N.CNDP_MODE_CNET, out=out)
            torch.cuda.synchronize()
            assert_same(out, ref, keys=ALL)
    finally:
        cl.set_tuning(cnet_spec=256, spec_scan=0)


@pytest.mark.parametrize("nb", [0, 1, 65, 1024])
def test_counters_accumulate(l3, cnet, gpu, nb):
    """bins is +=: counters that start non-zero, and two calls into one tensor."""
    cl, t4, frames, refs = l3
    ccl, routes, v6, ct4, ct6, cframes, crefs = cnet
    pre = np.arange(nb + 2, dtype=np.int64) * 3 + 1
    try:
        for tile in (0, 1):
            cl.set_tuning(tile=tile)
            bins = torch.from_numpy(pre.copy()).to(gpu)
            want = pre.astype(np.uint64)
            for name in ("routed", "fuzz"):
                run(cl, frames[name], N.CNDP_MODE_L3FWD, nb, bins=bins)
                want = want + l3_ref(l3, N.CNDP_MODE_L3FWD, name, nb)["bins"]
                assert np.array_equal(bins.cpu().numpy().view(np.uint64), want), f"tile={tile} after {name}"
        for ct in (0, 1):
            ccl.set_tuning(cnet_tile=ct)
            bins = torch.from_numpy(pre.copy()).to(gpu)
            want = pre.astype(np.uint64)
            for name, fr in cframes.items():
                run(ccl, fr, N.CNDP_MODE_CNET, nb, bins=bins)
                want = want + crefs(name, fr, N.CNDP_MODE_CNET, nb, tables4=ct4, tables6=ct6)["bins"]
                assert np.array_equal(bins.cpu().numpy().view(np.uint64), want), f"cnet_tile={ct} after {name}"
    finally:
        cl.set_tuning(tile=1)
        ccl.set_tuning(cnet_tile=1, cnet_spec=256)


def test_no_counters_any_n_bins(l3, cnet, gpu):
    """Without bins, n_bins is not looked at (5000 here) and every other output
    is what it is with them; with bins, n_bins above CNDP_BINS_MAX is -EINVAL."""
    cl, t4, frames, refs = l3
    ccl, routes, v6, ct4, ct6, cframes, crefs = cnet
    keys = ("nh", "hash", "queue", "edge", "ptype")

    def no_bins(c, fr, mode):
        if mode == N.CNDP_MODE_CNET:
            c.set_tuning(cnet_spec=256)
        out = c.alloc_outputs(fr.n, 0, device=gpu, meta=True)
        out["bins"], out["n_bins"] = None, 5000
        c.classify(fr, mode, out=out)
        torch.cuda.synchronize()
        return out

    try:
        for tile in (0, 1):
            cl.set_tuning(tile=tile)
            for mode in (N.CNDP_MODE_L3FWD, N.CNDP_MODE_HASH):
                for name in ("routed", "fuzz"):
                    if mode == N.CNDP_MODE_HASH:
                        cl.set_rss(reta=L3_RETA)
                    assert_same(no_bins(cl, frames[name], mode), l3_ref(l3, mode, name, 1024), keys=keys)
                cl.set_rss()
        for ct in (0, 1):
            ccl.set_tuning(cnet_tile=ct)
            for name, fr in cframes.items():
                ref = crefs(name, fr, N.CNDP_MODE_CNET, 1024, tables4=ct4, tables6=ct6)
                assert_same(no_bins(ccl, fr, N.CNDP_MODE_CNET), ref, keys=keys + ("rxmeta",))
        for c, fr, mode in ((cl, frames["routed"], N.CNDP_MODE_L3FWD), (ccl, cframes["imix"], N.CNDP_MODE_CNET)):
            out = c.alloc_outputs(fr.n, N.CNDP_BINS_MAX + 1, device=gpu)
            with pytest.raises(OSError) as e:
                c.classify(fr, mode, out=out)
            assert e.value.errno == 22
            torch.cuda.synchronize()
            assert int(out["bins"].sum()) == 0
    finally:
        cl.set_tuning(tile=1)
        cl.set_rss()
        ccl.set_tuning(cnet_tile=1, cnet_spec=256)


@pytest.mark.parametrize("nb", [1, 1024])
def test_counters_host_path_chunked(l3, cnet, gpu, nb):
    """classify_host in 1024-frame chunks: the counters sum across chunks, on
    top of what the caller's array held."""
    cl, t4, frames, refs = l3
    ccl, routes, v6, ct4, ct6, cframes, crefs = cnet
    pre = np.arange(nb + 2, dtype=np.uint64) * 3 + 1
    try:
        for c in (cl, ccl):
            c.set_tuning(host_chunk=1024)
        fr = frames["half"]
        ref = l3_ref(l3, N.CNDP_MODE_L3FWD, "half", nb)
        out = {"nh": np.zeros(fr.n, np.uint32), "hash": np.zeros(fr.n, np.uint32), "queue": np.zeros(fr.n, np.uint16),
               "edge": np.zeros(fr.n, np.uint8), "bins": pre.copy()}
        got = cl.classify_host(fr.slab.cpu().numpy(), fr.n, N.CNDP_MODE_L3FWD, stride=64, n_bins=nb, out=out)
        assert_same(got, ref, keys=("nh", "hash", "queue", "edge"))
        assert np.array_equal(got["bins"], pre + ref["bins"])
        fr = cframes["imix"]
        ref = crefs("imix", fr, N.CNDP_MODE_CNET, nb, tables4=ct4, tables6=ct6)
        ccl.set_tuning(cnet_spec=256)
        got = ccl.classify_host(fr.slab.cpu().numpy(), fr.n, N.CNDP_MODE_CNET, stride=fr.stride,
                                offsets=fr.offsets.cpu().numpy().astype(np.uint64), data_off=fr.data_off, n_bins=nb)
        assert_same(got, ref)
    finally:
        for c in (cl, ccl):
            c.set_tuning(host_chunk=1 << 20)
        ccl.set_tuning(cnet_spec=256)


@pytest.mark.parametrize("nb", [1, 1024])
def test_counters_fused_rewrite(l3_64, gpu, nb):
    """cndp_gpu_classify_rewrite's fused kernel (n % 256 == 0, burst 256)."""
    cl, t4 = l3_64
    tbl = _rewrite_setup(cl)
    n = 256 * 75
    fr = pktgen.packed_ipv4(n, routes=pktgen.l3fwd_routes(), seed=n)
    ref = oracle_classify(O.MODE_L3FWD, fr, tables4=t4, n_bins=nb)
    assert int(ref["bins"].sum()) == n and ref["bins"][nb] > 0 and (nb > 1 or ref["bins"][nb + 1] > 0)
    host = fr.slab.numpy().copy()
    ref_tx = O.ip4_rewrite(host, n, ref["nh"], tbl, burst=256)
    try:
        for nt, wb in ((1, 2), (0, 0)):
            cl.set_tuning(nt=nt, rw_wb=wb)
            d = pktgen.Frames(fr.slab.to(gpu), n, stride=64)
            out = cl.alloc_outputs(n, nb, device=gpu, edge=False)
            out, tx = cl.classify_rewrite(d, out=out, burst=256)
            torch.cuda.synchronize()
            assert_same(out, ref, keys=("nh", "hash", "queue", "bins"))
            assert np.array_equal(tx.cpu().numpy().view(np.uint16), ref_tx)
            assert np.array_equal(d.slab.cpu().numpy(), host)
    finally:
        cl.set_tuning(nt=1, rw_wb=2)


# ---------------------------------------------------------------------------
# c. cndp_gpu_bin_ids in every mode
# ---------------------------------------------------------------------------
def bin_rule(mode, nh, edge, queue, nb):
    """next-hop bins [0, nb) for the forwarding edge (l3fwd: edge
    0, id nh & 0xffff; cnet: edge 1, id nh & 0xffffff), drops (l3fwd: edge 1 and
    pkt_cls's 0xFF; cnet: edge 0 and the ptype node's 0x80) at nb, everything
    else -- a next hop past nb too -- at nb + 1.  Hash mode counts RSS queues."""
    nh, edge, queue = nh.astype(np.int64), edge.astype(np.int64), queue.astype(np.int64)
    if mode == N.CNDP_MODE_HASH:
        return np.where(queue < nb, queue, nb + 1)
    if mode == N.CNDP_MODE_L3FWD:
        key, fwd, drop = nh & 0xFFFF, edge == 0, (edge == 1) | (edge == 0xFF)
    else:
        key, fwd, drop = nh & 0xFFFFFF, edge == 1, (edge == 0) | (edge == 0x80)
    return np.where(fwd, np.where(key < nb, key, nb + 1), np.where(drop, nb, nb + 1))


@pytest.mark.parametrize("nb", CLS_NB)
@pytest.mark.parametrize("mode", list(MODES))
def test_bin_ids_every_mode(l3, cnet, part, gpu, mode, nb):
    """The ids equal the rule applied to the oracle's outputs, their histogram
    equals the classify call's counters, and so do the partition's bin sizes."""
    m = MODES[mode]
    if mode == "cnet":
        cl, routes, v6, t4, t6, frames, refs = cnet
        cases = [(fr, refs(name, fr, m, nb, tables4=t4, tables6=t6)) for name, fr in frames.items()]
    else:
        cl, t4, frames, refs = l3
        cases = [(frames[name], l3_ref(l3, m, name, nb)) for name in ("half", "fuzz")]
    try:
        if mode == "hash":
            cl.set_rss(reta=L3_RETA)
        for k, (fr, ref) in enumerate(cases):
            want = bin_rule(m, ref["nh"], ref["edge"], ref["queue"], nb)
            assert np.array_equal(np.bincount(want, minlength=nb + 2).astype(np.uint64), ref["bins"])
            if k == 0 and mode != "hash":
                assert len(np.unique(want)) >= min(nb, 60) + 2
            out = run(cl, fr, m, nb)
            ids_t = cl.bin_ids(m, out, fr.n, nb)
            torch.cuda.synchronize()
            ids = ids_t.cpu().numpy().view(np.uint16).astype(np.int64)
            assert np.array_equal(ids, want)
            got_bins = out["bins"].cpu().numpy().view(np.uint64)
            assert np.array_equal(np.bincount(ids, minlength=nb + 2).astype(np.uint64), got_bins)
            start, order = partition_raw(part, ids_t, fr.n, nb)
            torch.cuda.synchronize()
            check_partition(ids, nb, start, order, f"{mode} n_bins={nb}")
            assert np.array_equal(np.diff(start.cpu().numpy().view(np.uint32)[:nb + 3]).astype(np.uint64), got_bins)
    finally:
        cl.set_rss()


def test_bin_ids_errors(l3, gpu):
    cl, t4, frames, refs = l3
    fr = frames["routed"]
    out = run(cl, fr, N.CNDP_MODE_L3FWD, 64)
    with pytest.raises(OSError) as e:
        cl.bin_ids(N.CNDP_MODE_L3FWD, out, fr.n, N.CNDP_BINS_MAX + 1)
    assert e.value.errno == 22

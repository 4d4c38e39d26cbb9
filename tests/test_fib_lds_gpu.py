"""CNDP_TUNE_FIB_LDS: the l3fwd streamed kernel that resolves the FIB down to
tbl24 from an LDS copy of the directory's near image (k_classify_stream_img)
against the oracle, bit for bit, beside the gathering kernel (fib_lds=0) on the
same frames -- packed 64-B slots; CNDP_STAT_FIB_LDS tells which kernel ran.

Sizes: 197 frames (3 tiles, fewer than a block's 8 waves, and a ragged tail of 5),
40,013 (at a block a CU every wave stays inside its three static tiles) and
600,007 (9,375 tiles: more than 24 a block on a 256-CU device, so tiles are
drawn from the LDS counter)."""
import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd import pktgen
from oracle import oracle as O

from helpers import L3FWD_DEF, assert_same, l3fwd_fib, oracle_classify

pytestmark = pytest.mark.gpu
SIZES = (197, 40013, 600007)
RW = N.IP4_LOOKUP_NEXT_REWRITE

# a /8 with a /12, /16, /17, /24, /25 and /32 nested in it, and two more /8s
NESTED = [(0x14000000, 8, 1), (0x14100000, 12, 2), (0x14100000, 16, 3), (0x14108000, 17, 4),
          (0x1410C800, 24, 5), (0x1410C880, 25, 6), (0x1410C881, 32, 7),
          (0x1E010000, 16, 8), (0x28020300, 24, 9)]


def boundaries(routes):
    out = []
    for ip, d, _ in routes:
        last = ip | ((1 << (32 - d)) - 1)
        out += [ip - 1, ip, ip + 1, last - 1, last, last + 1]
    return np.array([x & 0xFFFFFFFF for x in out], dtype=np.uint32)


def make(routes):
    from cndp_amd.classify import Classifier
    fib, vals = l3fwd_fib(routes)
    cl = Classifier(0)
    cl.set_fib(fib)
    return cl, fib


def tables(routes):
    return O.dir24_8_build([(ip, d, (RW << 16) | nh) for ip, d, nh in routes], L3FWD_DEF, 256)


def with_dsts(fr, dsts):
    """fr with its destination addresses replaced by dsts, cycled (the classify
    parse does not verify the header checksum; the oracle reads the same bytes)."""
    d = torch.from_numpy(np.resize(dsts, fr.n).astype(np.int64)).to(fr.slab.device)
    v = fr.slab.view(fr.n, 64)
    for k in range(4):
        v[:, 30 + k] = ((d >> (24 - 8 * k)) & 0xFF).to(torch.uint8)
    return fr


def check(cl, fr, t4, image: bool):
    """fib_lds 0 and 1 both equal the oracle; the counter moves only for 1, and only
    when the image is usable."""
    ref = oracle_classify(O.MODE_L3FWD, fr, tables4=t4)
    try:
        for lds in (0, 1):
            cl.set_tuning(fib_lds=lds)
            before = cl.stat(N.CNDP_STAT_FIB_LDS)
            out = cl.classify(fr, N.CNDP_MODE_L3FWD, n_bins=64)
            torch.cuda.synchronize()
            assert_same({k: v for k, v in out.items() if k != "n_bins"}, ref)
            assert cl.stat(N.CNDP_STAT_FIB_LDS) - before == (1 if lds and image else 0), lds
    finally:
        cl.set_tuning(fib_lds=1)
    return ref


@pytest.fixture(scope="module")
def l3(gpu):
    routes = pktgen.l3fwd_routes()
    cl, fib = make(routes)
    return cl, fib, tables(routes)


@pytest.mark.parametrize("n", SIZES)
def test_l3fwd_routes(l3, gpu, n):
    cl, fib, t4 = l3
    fr = pktgen.packed_ipv4(n, routes=pktgen.l3fwd_routes(), device=gpu, seed=60 + n % 7)
    ref = check(cl, fr, t4, True)
    assert ref["bins"].sum() == n
    assert fib.near_info()["fits"] == 1


@pytest.mark.parametrize("n", SIZES)
def test_nested_slash8_boundaries(gpu, n):
    cl, fib = make(NESTED)
    fr = pktgen.packed_ipv4(n, routes=NESTED, device=gpu, seed=3)
    rng = np.random.default_rng(n)
    dsts = np.concatenate([boundaries(NESTED), rng.integers(0x14100000, 0x14110000, 64, dtype=np.uint32),
                           rng.integers(0, 1 << 32, 64, dtype=np.uint32)])
    rng.shuffle(dsts)
    ref = check(cl, with_dsts(fr, dsts), tables(NESTED), True)
    assert len(np.unique(ref["nh"])) >= len(NESTED) + 1      # every route and the default answered
    cl.close()


@pytest.mark.parametrize("n", SIZES)
def test_fuzz_frames_mixed(l3, gpu, n):
    """Non-IPv4 frames and IPv4 with options between routed ones (the slow hash,
    lanes without a lookup), at every size."""
    cl, fib, t4 = l3
    fr = pktgen.fuzz_frames(n, seed=47 + n % 5, slot=64, device=gpu)
    check(cl, fr, t4, True)


def test_new_slash8_after_first_launch(gpu):
    """A /8 slot taken from the high-water mark after the image was first uploaded,
    most of whose entries are value 0 (next hop 0 on the rewrite edge, as
    l3fwd_routes() has): the device slot must hold those zeros, not what the
    allocation left there.  Eight new /8s, so slots far behind the first upload."""
    routes = [(0x0A000000, 16, 3)]
    cl, fib = make(routes)
    fr0 = pktgen.packed_ipv4(40013, routes=routes, device=gpu, seed=12)
    check(cl, with_dsts(fr0, boundaries(routes)), tables(routes), True)
    assert fib.near_info()["mid_hwm"] == 1
    for k in range(8):
        for r in (((20 + k) << 24, 8, 0), (((20 + k) << 24) | 0x100000, 16, 5 + k)):
            assert fib.add(r[0], r[1], (RW << 16) | r[2]) == 0
            routes.append(r)
    rng = np.random.default_rng(4)
    inside = np.concatenate([rng.integers((20 + k) << 24, (21 + k) << 24, 400, dtype=np.uint32) for k in range(8)])
    every16 = np.array([((20 + k) << 24) | (b << 16) | 7 for k in range(8) for b in range(256)], dtype=np.uint32)
    fr = with_dsts(pktgen.packed_ipv4(40013, routes=routes, device=gpu, seed=13),
                   np.concatenate([boundaries(routes), inside, every16]))
    ref = check(cl, fr, tables(routes), True)
    assert fib.near_info()["mid_hwm"] == 9
    assert (ref["nh"] == (RW << 16)).sum() > 2000          # the value-0 entries were asked for
    cl.close()


def test_over_cap_falls_back(gpu):
    """40 /24 routes in 40 different /8s: 1 + 40 + 40 KiB is over the 32-KiB cap."""
    routes = [(((50 + k) << 24) | (k << 16) | (k << 8), 24, k) for k in range(40)]
    cl, fib = make(routes)
    fr = with_dsts(pktgen.packed_ipv4(40013, routes=routes, device=gpu, seed=5),
                   np.concatenate([boundaries(routes), np.array([0x0A000001], dtype=np.uint32)]))
    check(cl, fr, tables(routes), False)
    info = fib.near_info()
    assert info["fits"] == 0 and info["kib"] == 81
    cl.close()


def test_churn_on_one_context(gpu):
    """Route changes between launches of one context: every pass equals the oracle
    over the then-current tables, through the image kernel."""
    routes = list(NESTED) + [(0x1410C900, 24, 10)]
    cl, fib = make(routes)
    rng = np.random.default_rng(9)

    def one_pass(rs):
        extra = [(0x1410C840, 26, 11), (0x1E010000, 16, 8), (0x28020300, 24, 9)]
        dsts = np.concatenate([boundaries(routes + extra), rng.integers(0x14000000, 0x15000000, 200, dtype=np.uint32)])
        fr = with_dsts(pktgen.packed_ipv4(40013, routes=NESTED, device=gpu, seed=8), dsts)
        check(cl, fr, tables(rs), True)

    def add(r):
        assert fib.add(r[0], r[1], (RW << 16) | r[2]) == 0
        routes.append(r)

    def delete(r):
        assert fib.delete(r[0], r[1]) == 0
        routes.remove(r)

    one_pass(routes)
    add((0x1410C840, 26, 11))               # a /26 inside the routed 20.16.200.0/24
    delete((0x28020300, 24, 9))             # 40.2/16 turns uniform again: its page is freed
    one_pass(routes)
    assert fib.near_info()["mid_used"] == 2
    delete((0x1E010000, 16, 8))             # the last route of 30/8: its /8 page is freed
    one_pass(routes)
    assert fib.near_info()["mid_used"] == 1
    add((0x1E010000, 16, 8))
    add((0x28020300, 24, 9))
    one_pass(routes)
    info = fib.near_info()
    assert info["mid_used"] == 3 and info["mid_hwm"] == 3     # freed slots reused
    cl.close()

"""cndpfwd's fwd and l3fwd modes on the GPU (cndp_gpu_cfwd,
include/cndp_cfwd.h): nh, tx_lport, echoed, bin_of, the counters and the WHOLE
slab must equal the Python restatement (tests/cfwd_ref.py, pinned to the
compiled reference FIB by tests/golden/cndpfwd_l3_ref.npz) for every frame.
Shapes are the smallest that can still go wrong: one lane, a wave and its
neighbours, a block and one more, a short last block of a fifth block; packed
64-byte slots and the UMEM stride (16-byte aligned frames, the wide path) and
odd byte offsets (the byte path); a slab that ends inside the last frame."""
import os

import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd import pktgen
from cndp_amd.cfwd import alloc_cfwd_outputs, l3fwd_fib, route_add
from cndp_amd.fib import Fib

import cfwd_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("nh", "tx_lport", "echoed", "bin_of", "stats")
DT = {"nh": np.uint64, "tx_lport": np.uint16, "echoed": np.uint8, "bin_of": np.uint16, "stats": np.uint64}
SIZES = (1, 63, 64, 65, 257, 1031)
KINDS = ("packed", "umem", "offsets")


@pytest.fixture(scope="module")
def cl(gpu):
    from cndp_amd.classify import Classifier
    c = Classifier(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fib(gpu):
    f = R.apply_ops(l3fwd_fib())
    yield f
    f.close()


@pytest.fixture(scope="module")
def routes():
    return R.routes_of(R.golden())


def to_frames(slab, n, lay, dev="cuda:0"):
    offs = None if lay["offsets"] is None else torch.from_numpy(lay["offsets"].astype(np.int64)).to(dev)
    return pktgen.Frames(torch.from_numpy(slab.copy()).to(dev), n, stride=lay["stride"], offsets=offs,
                         data_off=lay["data_off"])


def run(cl, fib, routes, slab, n, lay, mode, out=None, stats0=None, **kw):
    """One cndpfwd call against the restatement on the same bytes: outputs, the
    counters and the whole slab.  Returns (got, want, the result tensors)."""
    fr = to_frames(slab, n, lay)
    dev_kw = dict(kw)
    if kw.get("sel") is not None:
        dev_kw["sel"] = torch.from_numpy(np.ascontiguousarray(kw["sel"], np.uint8)).to(fr.slab.device)
    res = cl.cndpfwd(fr, mode, fib=fib, out=out, **dev_kw)
    torch.cuda.synchronize()
    got = {k: res[k].cpu().numpy().view(DT[k]).copy() for k in KEYS}
    want = R.cfwd_ref(slab, n, mode, routes=routes, stats=stats0, **kw, **lay)
    for k in KEYS:
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[0]}: got {got[k][bad[0]]} want {want[k][bad[0]]}"
    after = fr.slab.cpu().numpy()
    bad = np.nonzero(after != want["slab"])[0]
    assert len(bad) == 0, f"slab: {len(bad)} bytes differ, first at {bad[0]}"
    return got, want, res


def golden_rows(n, seed=1):
    """n frames to the golden file's first n addresses (hits through tbl24 and
    tbl8, deleted routes, near misses, misses, every port), p[5] over 0..8."""
    g = R.golden()
    return R.frames(g["addr"][:n], dmac5=np.arange(n) % 9, ttl=np.arange(n) % 256, seed=seed)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", (R.FWD, R.L3FWD))
def test_wave_and_block_edges(cl, fib, routes, mode, kind):
    for n in SIZES:
        slab, lay = R.layout(golden_rows(n, seed=n), kind, seed=n)
        _, want, _ = run(cl, fib, routes, slab, n, lay, mode, in_lport=3, lports=(0, 1, 3, 7, 255))
        if n >= 257:
            assert want["echoed"].any() and not want["echoed"].all()
            assert (len(np.unique(want["nh"])) > 20) if mode == R.L3FWD else not want["nh"].any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", (R.FWD, R.L3FWD))
def test_slab_ends_inside_the_last_frame(cl, fib, routes, mode, kind):
    n = 65
    slab, lay = R.layout(golden_rows(n, seed=7), kind, seed=7)
    last = int(R.frame_starts(n, **lay)[-1])
    for cut in (5, 11, 22, 24, 33):
        got, want, res = run(cl, fib, routes, slab, n, lay, mode, in_lport=1, lports=(0, 1, 2), slab_len=last + cut)
        assert np.array_equal(want["slab"][last + cut:], slab[last + cut:])     # nothing past the end is written
    # the last frame lies wholly past the end: it reads as zeros (0.0.0.0 is a miss; p[5] = 0)
    got, _, _ = run(cl, fib, routes, slab, n, lay, mode, in_lport=1, lports=(0, 1, 2), slab_len=last)
    assert got["tx_lport"][-1] == 0 and got["nh"][-1] == (R.DEFAULT_NH if mode == R.L3FWD else 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", (R.FWD, R.L3FWD))
def test_selection(cl, fib, routes, mode, kind):
    n = 257
    slab, lay = R.layout(golden_rows(n, seed=11), kind, seed=11)
    for sel in (np.zeros(n, np.uint8), np.ones(n, np.uint8), (np.arange(n) % 2).astype(np.uint8)):
        got, want, _ = run(cl, fib, routes, slab, n, lay, mode, in_lport=2, lports=(0, 2, 5), sel=sel)
        off = sel == 0
        assert (got["tx_lport"][off] == 0xFFFF).all() and (got["bin_of"][off] == 6).all() and not got["nh"][off].any()
        assert got["stats"].sum() == np.count_nonzero(sel)
        if not sel.any():
            assert np.array_equal(want["slab"], slab)                           # frames not taken stay as they were


@pytest.mark.parametrize("kind", ("packed", "offsets"))
def test_ttl_checksum_and_a_frame_that_is_not_ipv4(cl, fib, routes, kind):
    g = np.load(os.path.join(HERE, "golden", "ip4_fwd_cksum_ref.npz"))
    # TTL 0 and 1 with the four named checksums, then the golden file's carry cases
    ttl = np.concatenate([np.repeat([0, 1], 4), g["ttl"][:1023]]).astype(np.uint8)
    ck = np.concatenate([np.tile([0x0000, 0xFFFF, 0xFEFF, 0xFF00], 2), g["cksum"][:1023]]).astype(np.uint16)
    want_ttl = np.concatenate([np.repeat([255, 0], 4), g["ttl_out"][:1023]])
    want_ck = np.concatenate([R.adjust_cksum(ck[:8]), g["cksum_out"][:1023]])
    n = len(ttl)
    rows = R.frames(R.golden()["addr"][:n], ttl=ttl, ck=ck, seed=13)
    rows[::5, 12:14] = (0x08, 0x06)                                             # ARP: edited all the same
    rows[1::5, 14] = 0x60
    slab, lay = R.layout(rows, kind, seed=13)
    _, want, _ = run(cl, fib, routes, slab, n, lay, R.L3FWD, in_lport=0, lports=(0, 1))
    at = R.frame_starts(n, **lay)
    out = want["slab"]
    assert np.array_equal(out[at + 22], want_ttl)
    assert np.array_equal(out[at + 24].astype(np.int64) | out[at + 25].astype(np.int64) << 8, want_ck)


def test_golden_routes_ports_and_a_mask_without_port_0(cl, fib, routes):
    g = R.golden()
    n = 2048
    rows = R.frames(g["addr"], seed=17)
    lay = dict(stride=64, offsets=None, data_off=0)
    got, want, _ = run(cl, fib, routes, rows.reshape(-1), n, lay, R.L3FWD, in_lport=9, lports=(1, 7, 255))
    assert np.array_equal(got["nh"], g["nh"]), "differs from the next hops the reference recorded"
    rew = got["echoed"] == 0
    out = want["slab"].reshape(n, 64)
    assert np.array_equal(out[rew, :6], g["mac"][rew]) and np.array_equal(got["tx_lport"][rew], g["tx_port"][rew])
    assert set(g["tx_port"][rew].tolist()) == {1, 7, 255} and set(g["tx_port"][~rew].tolist()) == {0, 256, 0x7FFF}
    assert (got["tx_lport"][~rew] == 9).all()
    miss = g["nh"] == R.DEFAULT_NH
    assert miss.any() and not rew[miss].any()                                   # without port 0 a miss is echoed
    # tbl8 paths, and a deleted route's addresses answered by its parent
    deep = {k for k in routes if k[1] > 24}
    hit_deep = [i for i in range(n) if any((int(g["addr"][i]) & R.mask(d)) == p for p, d in deep)]
    gone = {(ip & R.mask(d), d) for ip, d, dele in zip(g["op_ip"].tolist(), g["op_depth"].tolist(), g["op_del"].tolist()) if dele}
    gone -= set(routes)
    fell = [i for i in range(n) if not miss[i] and any((int(g["addr"][i]) & R.mask(d)) == p for p, d in gone)]
    assert hit_deep and fell


def test_fwd_mode_ports_in_and_out_of_the_mask(cl, routes):
    n = 257
    rows = R.frames(np.zeros(n, np.uint32), dmac5=np.arange(n) % 256, seed=19)
    slab, lay = R.layout(rows, "umem", seed=19)
    got, _, _ = run(cl, None, routes, slab, n, lay, R.FWD, in_lport=4, lports=(0, 4, 63, 64, 200, 255))
    want_tx = [p if p in (0, 4, 63, 64, 200, 255) else 4 for p in (np.arange(n) % 256).tolist()]
    assert got["tx_lport"].tolist() == want_tx and got["stats"].tolist() == [7, n - 7]      # port 0 comes twice


def test_dir24_8_8b_fib_answers_as_the_dummy_one(cl, routes):
    wide = R.apply_ops(Fib("wide", N.CNE_FIB_DIR24_8, default_nh=R.DEFAULT_NH, max_routes=1 << 16,
                         nh_sz=N.CNE_FIB_DIR24_8_8B, num_tbl8=1024))
    g = R.golden()
    rows = R.frames(g["addr"][:1031], seed=23)
    got, _, _ = run(cl, wide, routes, rows.reshape(-1), 1031, dict(stride=64, offsets=None, data_off=0), R.L3FWD,
                    in_lport=0, lports=(0, 1, 7, 255))
    assert np.array_equal(got["nh"], g["nh"][:1031])
    narrow = Fib("narrow", N.CNE_FIB_DIR24_8, default_nh=0, max_routes=16, nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=16)
    fr = to_frames(rows.reshape(-1), 4, dict(stride=64, offsets=None, data_off=0))
    with pytest.raises(OSError) as e:                                           # 4-byte entries: refused
        cl.cndpfwd(fr, R.L3FWD, fib=narrow, lports=(0,))
    assert e.value.errno == 22
    with pytest.raises(OSError):                                                # L3FWD without a FIB
        cl.cndpfwd(fr, R.L3FWD, fib=None, lports=(0,))
    torch.cuda.synchronize()
    assert np.array_equal(fr.slab.cpu().numpy(), rows.reshape(-1))
    narrow.close()
    wide.close()


def test_bin_of_feeds_bin_partition(cl, fib, routes):
    g = R.golden()
    n = 1031
    rows = R.frames(g["addr"][:n], seed=29)
    fr = to_frames(rows.reshape(-1), n, dict(stride=64, offsets=None, data_off=0))
    sel = (np.arange(n) % 5 != 0).astype(np.uint8)
    kw = dict(in_lport=6, lports=(0, 1, 7))
    res = cl.cndpfwd(fr, R.L3FWD, fib=fib, sel=torch.from_numpy(sel).to("cuda:0"), **kw)
    want = R.cfwd_ref(rows.reshape(-1), n, R.L3FWD, routes=routes, sel=sel, stride=64, **kw)
    assert res["n_bins"] == want["n_bins"] == 8
    start, order = cl.bin_partition(res["bin_of"], res["n_bins"])
    torch.cuda.synchronize()
    bins = want["bin_of"].astype(np.int64)
    assert set(np.unique(bins)) == {0, 1, 6, 7, 8}                              # known ports, the echo port, not taken
    # the reference's per-port order: txbuff_add appends in burst order (main.c:298)
    assert np.array_equal(order.cpu().numpy(), np.argsort(bins, kind="stable"))
    assert np.array_equal(start.cpu().numpy()[:10], np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=9))]))


def test_mirror_sync_stats_and_n_zero(cl):
    """A route added between two calls takes effect in the second; a delete in
    the third; the counters add up over the calls; n == 0 launches nothing."""
    fib = l3fwd_fib("sync")
    mac1, mac2 = bytes.fromhex("02aa00000001"), bytes.fromhex("02bb00000002")
    dst = np.array([0x0A010203, 0x0A010281, 0x0B000001] * 22, np.uint32)[:65]
    rows = R.frames(dst, seed=31)
    lay = dict(stride=64, offsets=None, data_off=0)
    kw = dict(in_lport=0, lports=(0, 1))
    table = {}
    got1, _, res = run(cl, fib, table, rows.reshape(-1), 65, lay, R.L3FWD, **kw)
    assert (got1["nh"] == R.DEFAULT_NH).all() and got1["stats"].tolist() == [65, 0]
    route_add(fib, 0x0A010200, 24, mac1, 1)
    route_add(fib, 0x0A010281, 32, mac2, 2)                                     # behind the /24, through tbl8; port 2 is unknown
    table = {(0x0A010200, 24): R.nexthop(mac1, 1), (0x0A010281, 32): R.nexthop(mac2, 2)}
    got2, _, res = run(cl, fib, table, rows.reshape(-1), 65, lay, R.L3FWD, out=res, stats0=got1["stats"], **kw)
    assert got2["nh"][:3].tolist() == [R.nexthop(mac1, 1), R.nexthop(mac2, 2), R.DEFAULT_NH]
    assert got2["tx_lport"][:3].tolist() == [1, 0, 0] and got2["echoed"][:3].tolist() == [0, 1, 0]
    assert got2["stats"].tolist() == [65 + 43, 22]
    assert fib.delete(0x0A010281, 32) == 0
    del table[(0x0A010281, 32)]
    got3, _, res = run(cl, fib, table, rows.reshape(-1), 65, lay, R.L3FWD, out=res, stats0=got2["stats"], **kw)
    assert got3["nh"][1] == R.nexthop(mac1, 1) and got3["stats"].tolist() == [65 + 43 + 65, 22]
    before = {k: res[k].clone() for k in KEYS}
    for mode, f in ((R.FWD, None), (R.L3FWD, fib)):
        cl.cndpfwd(to_frames(rows.reshape(-1), 0, lay), mode, fib=f, out=alloc_cfwd_outputs(0, "cuda:0"), **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], res[k]) for k in KEYS)
    fib.close()
